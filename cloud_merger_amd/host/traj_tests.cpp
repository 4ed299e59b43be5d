// traj_tests.cpp — the host shell's rollout layer behind the plan layer: NodeConfig keys and the footprint lattice (CPU) and,
// with "gpu", one node that integrates map_tests' first frame with the cost layer, the plan and the rollout evaluated behind
// it in the frame epilogue, checked against scores worked out by hand and against what the library returns for the same frame.
//   traj_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys_and_lattice(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/traj.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.traj_nv == 0u && ref.traj_nw == 1u && ref.traj_steps == 1u && !ref.traj_allow_unknown);     // off by default
    CHECK(ref.traj_occ_scale == 1u && ref.traj_goal_scale == 1u && ref.traj_footprint[0] == 0.0f && ref.traj_footprint[1] == 0.0f && ref.traj_footprint[2] == 0.0f);
    CHECK(load_text(path, head + "traj 33 65 40 0.1\ntraj_limits 0.5 8 -0.8 0.8\ntraj_footprint -1 3.5 0.95\ntraj_scales 100 2\ntraj_allow_unknown 1\n", &c, &err));
    CHECK(c.traj_nv == 33u && c.traj_nw == 65u && c.traj_steps == 40u && c.traj_dt == 0.1f && c.traj_allow_unknown);
    CHECK(c.traj_limits[0] == 0.5f && c.traj_limits[1] == 8.0f && c.traj_limits[2] == -0.8f && c.traj_limits[3] == 0.8f);
    CHECK(c.traj_footprint[0] == -1.0f && c.traj_footprint[1] == 3.5f && c.traj_footprint[2] == 0.95f && c.traj_occ_scale == 100u && c.traj_goal_scale == 2u);
    CHECK(load_text(path, head + "traj 0 0 0 0   # nv 0 is off\ntraj_allow_unknown 0\n", &c, &err) && c.traj_nv == 0u && !c.traj_allow_unknown);
    CHECK(load_text(path, head + "traj 128 128 256 2.5\n", &c, &err) && c.traj_nv == 128u && c.traj_steps == 256u);
    CHECK(load_text(path, head + "traj_limits 1 1 0 0\ntraj_footprint 0 0 0\ntraj_scales 0 0\n", &c, &err) && c.traj_occ_scale == 0u);
    // rejected: counts beyond the library's, a dt that is no duration, missing values, limits the wrong way round, a footprint
    // that is no rectangle, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "traj 129 128 10 0.1\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "traj 3 0 10 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 0 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 257 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 10 0\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 10 -0.1\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 10 nan\n", &c, &err));
    CHECK(!load_text(path, head + "traj 3 3 10\n", &c, &err));
    CHECK(!load_text(path, head + "traj -1 3 10 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "traj_limits 1 0.5 0 0\n", &c, &err));
    CHECK(!load_text(path, head + "traj_limits 0 1 0.5 -0.5\n", &c, &err));
    CHECK(!load_text(path, head + "traj_limits 0 1 0\n", &c, &err));
    CHECK(!load_text(path, head + "traj_limits 0 inf 0 0\n", &c, &err));
    CHECK(!load_text(path, head + "traj_footprint 1 0 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "traj_footprint 0 1 -0.5\n", &c, &err));
    CHECK(!load_text(path, head + "traj_footprint 0 1\n", &c, &err));
    CHECK(!load_text(path, head + "traj_footprint 0 nan 1\n", &c, &err));
    CHECK(!load_text(path, head + "traj_scales 1\n", &c, &err));
    CHECK(!load_text(path, head + "traj_scales 1 x\n", &c, &err));
    CHECK(!load_text(path, head + "traj_allow_unknown 2\n", &c, &err));
    CHECK(!load_text(path, head + "traj_allow_unknown\n", &c, &err));

    // the lattice: at most half a cell between neighbours, the rectangle's corners on it, capped at CM_TRAJ_MAX_FOOT
    std::vector<float> xy;
    CHECK(!traj_footprint_lattice(0.0f, 0.0f, 0.0f, 0.1f, &xy) && xy.size() == 2 && xy[0] == 0.0f && xy[1] == 0.0f);
    CHECK(!traj_footprint_lattice(-0.25f, 0.25f, 0.25f, 0.5f, &xy) && xy.size() == 18);
    CHECK(xy[0] == -0.25f && xy[1] == -0.25f && xy[2] == -0.25f && xy[3] == 0.0f && xy[8] == 0.0f && xy[9] == 0.0f && xy[16] == 0.25f && xy[17] == 0.25f);
    CHECK(!traj_footprint_lattice(-0.3f, 0.3f, 0.25f, 0.5f, &xy) && xy.size() == 2 * 4 * 3);       // 0.6 m needs three gaps of at most 0.25 m
    CHECK(!traj_footprint_lattice(0.0f, 0.75f, 0.35f, 0.1f, &xy) && xy.size() == 2 * 16 * 15);     // 240 points: just under the cap
    CHECK(traj_footprint_lattice(-1.0f, 3.5f, 0.95f, 0.1f, &xy) && xy.size() == 2 * 24 * 10);      // 91 x 39 scaled by sqrt(256 / 3549)
    CHECK(xy[0] == -1.0f && xy[1] == -0.95f && xy[xy.size() - 2] == 3.5f && xy[xy.size() - 1] == 0.95f);
    CHECK(traj_footprint_lattice(0.0f, 100.0f, 0.0f, 0.1f, &xy) && xy.size() == 2 * CM_TRAJ_MAX_FOOT && xy[1] == 0.0f && xy[xy.size() - 2] == 100.0f);
    CHECK(traj_footprint_lattice(0.0f, 0.0f, 50.0f, 0.1f, &xy) && xy.size() == 2 * CM_TRAJ_MAX_FOOT && xy[0] == 0.0f && xy[1] == -50.0f);
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // plan_tests' node: a window of 6 x 4 cells of 0.5 m, the goal in window cell (0, 0), the vehicle in (3, 2) at the world's
    // origin, which is that cell's lower left corner. The cost table and the potential are plan_tests':
    //   255  92 152 254 152 254          0  465 1230    X    .    X
    //   255 255 152 254 255 255       1265 1730 1536    X    .    .
    //   255 (the two rows above)      2530 2995 2801 4066 5331 6596      (4066 + 5 * 253, then again)
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.map_cell = 0.5f;
    c.map_nx = 6;
    c.map_ny = 4;
    c.map_inscribed_radius = 0.0f;
    c.map_inflation_radius = 1.0f;
    c.map_cost_scaling = 1.0f;
    c.map_plan_neutral = 1;
    c.map_plan_factor_q8 = 256;
    c.map_plan_allow_unknown = true;
    c.map_has_goal = true;
    c.map_goal[0] = -1.25f;
    c.map_goal[1] = -0.75f;
    c.traj_nv = 2;                                     // v = 0 and 1 m/s, w = -pi / 2, 0 and pi / 2 rad/s, two steps of 0.5 s
    c.traj_nw = 3;
    c.traj_steps = 2;
    c.traj_dt = 0.5f;
    c.traj_limits[0] = 0.0f;
    c.traj_limits[1] = 1.0f;
    c.traj_limits[2] = -3.1415927f;
    c.traj_limits[3] = 3.1415927f;
    c.traj_occ_scale = 10;
    c.traj_goal_scale = 3;
    c.traj_allow_unknown = true;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    {
        // a layer the library refuses (such counts cannot come from a file, but can from code): the node does not start
        NodeConfig bad = c;
        bad.traj_steps = 300;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_traj_configure") != std::string::npos);
    }
    {
        // a footprint whose lattice the cap coarsens: the node starts and says so
        NodeConfig wide = c;
        wide.traj_footprint[0] = -5.0f;
        wide.traj_footprint[1] = 5.0f;
        wide.traj_footprint[2] = 5.0f;
        CloudMergerNode node(wide);
        CHECK(node.ok() && node.error().find("coarsened") != std::string::npos);
    }
    {
        // no goal: no plan, so no scores; then a goal outside the window: the frame stands, plan and scores are empty and
        // error() says why; then a goal inside it
        NodeConfig off = c;
        off.map_has_goal = false;
        CloudMergerNode node(off);
        CHECK(node.ok());
        node.set_transform(0, q, t);
        cm_result r{};
        float v = 7.0f, w = 7.0f;
        feed(node, pts, &r);
        CHECK(node.map_cost().size() == 24 && node.map_potential().empty() && node.traj_scores().empty() && !node.best_command(&v, &w) && v == 7.0f);
        CHECK(node.set_goal(40.0f, 0.0f) == CM_OK);
        feed(node, pts, &r);
        CHECK(node.map_cost().size() == 24 && node.map_potential().empty() && node.traj_scores().empty() && !node.best_command(&v, &w));
        CHECK(node.error().find("goal") != std::string::npos);
        CHECK(node.set_goal(-1.25f, -0.75f) == CM_OK);
        feed(node, pts, &r);
        CHECK(node.map_potential().size() == 24 && node.traj_scores().size() == 6 && node.best_command(&v, &w));
        // a vehicle outside the window cannot come from the node's own poses (the window follows them); one the map refuses
        // leaves the frame failed as before, and the scores empty
        float far[12] = {1, 0, 0, 3e38f, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(node.set_pose(far) == CM_OK);
        PointCloud2 m = xyzi_message(pts);
        CHECK(node.on_cloud(0, m) == CM_OK);
        CHECK(node.spin_once(&r) != CM_OK && node.traj_scores().empty() && !node.best_command(&v, &w));
        CHECK(node.error().find("vehicle") != std::string::npos);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(node.traj_scores().empty() && !node.best_command(nullptr, nullptr));
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);
    CHECK(node.map_potential().size() == 24 && node.map_path().size() == 5 && node.traj_scores().size() == 6);   // the epilogue's order: cost, plan, path, rollout
    if (node.traj_scores().size() != 6) { std::printf("  %s\n", node.error().c_str()); return; }
    const std::vector<cm_traj_score>& s = node.traj_scores();
    // v = 0: the three samples stand still in (3, 2): unknown and allowed, occ 0, pot 4066
    for (size_t j = 0; j < 3; ++j)
        CHECK(s[j].status == CM_TRAJ_VALID && s[j].bad_step == 0u && s[j].occ == 0u && s[j].pot_end == 4066u && s[j].total == 3u * 4066u &&
              s[j].end_x == 0.0f && s[j].end_y == 0.0f);
    // v = 1, w = 0 (entry 4): half a metre per step along +x, through (4, 2) into (5, 2)
    CHECK(s[4].status == CM_TRAJ_VALID && s[4].occ == 0u && s[4].pot_end == 6596u && s[4].total == 3u * 6596u && s[4].end_x == 1.0f && s[4].end_y == 0.0f);
    // v = 1, w = -pi / 2 (entry 3): +x into (4, 2), then a quarter turn later along -y: (1.0, 0) ... the first pose is (0.5, 0),
    // the second (0.5, -0.5) in (4, 1): unknown, allowed; pot(4, 1) is reached from (4, 2) only
    CHECK(s[3].status == CM_TRAJ_VALID && s[3].end_x == 0.5f && s[3].end_y == -0.5f && s[3].pot_end == 5331u + 5u * 253u);
    // v = 1, w = pi / 2 (entry 5): (0.5, 0), then (0.5, 0.5) in (4, 3), which the diagonal from (3, 2) reaches: no lethal cell
    // at that corner
    CHECK(s[5].status == CM_TRAJ_VALID && s[5].end_x == 0.5f && s[5].end_y == 0.5f && s[5].pot_end == 4066u + 7u * 253u);
    const cm_traj_info ti = node.traj_info();
    float bv = 7.0f, bw = 7.0f;
    CHECK(ti.best == 0u && ti.n_valid == 6u && ti.start[0] == 3u && ti.start[1] == 2u && node.best_command(&bv, &bw) && bv == 0.0f && bw == -3.1415927f);
    // what the library returns for the same frame on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 6, 4, c.map_z_band[0], c.map_z_band[1], 85, 40, -200, 350, -40, 85, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_plan_params pp{1, 256, CM_PLAN_ALLOW_UNKNOWN, 24};
        const cm_traj_params tp{2, 3, 2, 10, 3, CM_TRAJ_ALLOW_UNKNOWN};
        const cm_traj_window win{0.0f, 0.0f, 0.0f, 0.0f, 1.0f, -3.1415927f, 3.1415927f, 0.5f};
        const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, origin[2] = {0.0f, 0.0f};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK && cm_map_cost_configure(ctx, &cp) == CM_OK);
        CHECK(cm_map_traj_configure(ctx, &tp, origin, 1) == CM_BAD_ARG);                      // no plan layer yet
        CHECK(cm_map_plan_configure(ctx, &pp) == CM_OK && cm_map_traj_configure(ctx, &tp, origin, 1) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        cm_result r2{};
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
        CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_OK && cm_map_cost_update(ctx, nullptr) == CM_OK);
        cm_traj_info info{};
        CHECK(cm_map_traj_evaluate(ctx, &win, &info) == CM_BAD_ARG);                         // the potential is stale
        CHECK(cm_map_plan_update(ctx, -1.25f, -0.75f, nullptr, nullptr) == CM_OK);
        std::vector<cm_traj_score> got(7);
        std::memset(got.data(), 7, 7 * sizeof(cm_traj_score));
        CHECK(cm_map_traj_copy(ctx, got.data(), 6, nullptr) == CM_BAD_ARG);                  // stale until the evaluate
        CHECK(cm_map_traj_evaluate(ctx, &win, &info) == CM_OK && std::memcmp(&info, &ti, sizeof info) == 0);
        CHECK(cm_map_traj_copy(ctx, got.data(), 5, nullptr) == CM_CAPACITY && got[0].status == 0x07070707u);
        CHECK(cm_map_traj_copy(ctx, got.data(), 6, nullptr) == CM_OK && std::memcmp(got.data(), s.data(), 6 * sizeof(cm_traj_score)) == 0);
        CHECK(got[6].status == 0x07070707u);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing integrated, the tables stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.traj_scores().size() == 6 && node.best_command(nullptr, nullptr));
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys_and_lattice, test_node_on_gpu); }
