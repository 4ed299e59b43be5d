// plan_tests.cpp — the host shell's plan layer behind the cost layer: NodeConfig keys (CPU) and, with "gpu", one node that
// integrates map_tests' first frame with the cost layer and the plan updated behind it, checked against a potential and a path
// worked out by hand and against what the library returns for the same frame.
//   plan_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/plan.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.map_plan_neutral == 0u && ref.map_plan_factor_q8 == 205u && !ref.map_plan_allow_unknown && !ref.map_has_goal);   // off by default
    CHECK(load_text(path, head + "map_cell 0.1\nmap_size 100 80\nmap_inflation 0.35 1.05 3\nmap_plan 50 205\nmap_plan_allow_unknown 1\nmap_goal 4.5 -1.25\n", &c, &err));
    CHECK(c.map_plan_neutral == 50u && c.map_plan_factor_q8 == 205u && c.map_plan_allow_unknown && c.map_has_goal);
    CHECK(c.map_goal[0] == 4.5f && c.map_goal[1] == -1.25f);
    CHECK(load_text(path, head + "map_plan 0 0   # neutral 0 is off\nmap_plan_allow_unknown 0\n", &c, &err));
    CHECK(c.map_plan_neutral == 0u && !c.map_plan_allow_unknown && !c.map_has_goal);
    CHECK(load_text(path, head + "map_plan 255 256\n", &c, &err) && c.map_plan_neutral == 255u && c.map_plan_factor_q8 == 256u);
    CHECK(load_text(path, head + "map_plan 1 0\n", &c, &err) && c.map_plan_neutral == 1u && c.map_plan_factor_q8 == 0u);
    // rejected: a neutral or a factor beyond the library's range, missing values, a flag that is not 0 or 1, a goal that is
    // not a position
    CHECK(!load_text(path, head + "map_plan 256 205\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "map_plan 50 257\n", &c, &err));
    CHECK(!load_text(path, head + "map_plan 50\n", &c, &err));
    CHECK(!load_text(path, head + "map_plan\n", &c, &err));
    CHECK(!load_text(path, head + "map_plan -1 205\n", &c, &err));
    CHECK(!load_text(path, head + "map_plan_allow_unknown 2\n", &c, &err));
    CHECK(!load_text(path, head + "map_plan_allow_unknown\n", &c, &err));
    CHECK(!load_text(path, head + "map_goal 1\n", &c, &err));
    CHECK(!load_text(path, head + "map_goal nan 0\n", &c, &err));
    CHECK(!load_text(path, head + "map_goal 0 inf\n", &c, &err));
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
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
    c.map_goal[0] = -1.25f;                            // window cell (0, 0) under the identity pose: the anchor is (-3, -2)
    c.map_goal[1] = -0.75f;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    {
        // a layer the library refuses (a neutral beyond 255 cannot come from a file, but can from code): the node does not start
        NodeConfig bad = c;
        bad.map_plan_neutral = 300;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_plan_configure") != std::string::npos);
    }
    {
        // no goal: the cost layer alone, no tables of the plan; then a goal outside the window: the frame stands, the plan is
        // empty and error() says why; then a goal inside it
        NodeConfig off = c;
        off.map_has_goal = false;
        CloudMergerNode node(off);
        CHECK(node.ok());
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);
        CHECK(node.map_cost().size() == 24 && node.map_potential().empty() && node.map_path().empty());
        CHECK(node.set_goal(std::nanf(""), 0.0f) == CM_BAD_ARG && node.set_goal(40.0f, 0.0f) == CM_OK);
        feed(node, pts, &r);
        CHECK(node.map_cost().size() == 24 && node.map_potential().empty() && node.map_path().empty());
        CHECK(node.error().find("goal") != std::string::npos);
        CHECK(node.set_goal(-1.25f, -0.75f) == CM_OK);
        feed(node, pts, &r);
        CHECK(node.map_potential().size() == 24 && node.map_potential()[0] == 0u && node.map_path_info().status == CM_PATH_FOUND);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(node.map_potential().empty() && node.map_path().empty());
    // map_tests' first frame: the image is
    //   -1   0   0 100   0 100
    //   -1  -1   0 100  -1  -1
    //   -1 (the two rows above)
    // Cells of 0.5 m, radii 0 and 1.0, scaling 1: the table is 254, 152 (d2 1), 124 (2), 105 (3), 92 (4), so the cost table is
    //   255  92 152 254 152 254
    //   255 255 152 254 255 255
    //   255 (the two rows above)
    // With neutral 1, factor 256 and unknown cells allowed (255 counts as 252) a cell weighs 1 + cost:
    //   253  93 153   X 153   X
    //   253 253 153   X 253 253
    //   253 (the two rows above)
    // The goal is (0, 0). (1, 0) = 5 * 93; (2, 1) = 465 + 7 * 153 over the diagonal; (2, 2) = 1536 + 5 * 253; the vehicle cell
    // (3, 2) = 2801 + 5 * 253: its diagonal to (2, 1) would cut the corner of the lethal (3, 1).
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);
    CHECK(node.map_cost().size() == 24 && node.map_potential().size() == 24);
    if (node.map_cost().size() != 24 || node.map_potential().size() != 24) { std::printf("  %s\n", node.error().c_str()); return; }
    const uint8_t cost1[24] = {255, 92, 152, 254, 152, 254, 255, 255, 152, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255};
    for (size_t k = 0; k < 24; ++k) CHECK(node.map_cost()[k] == cost1[k]);
    const std::vector<uint32_t>& pot = node.map_potential();
    const uint32_t X = CM_PLAN_UNREACHABLE;
    CHECK(pot[0] == 0u && pot[1] == 465u && pot[2] == 1230u && pot[3] == X && pot[5] == X && pot[9] == X);
    CHECK(pot[6] == 1265u && pot[7] == 1730u && pot[8] == 1536u && pot[12] == 2530u && pot[13] == 2995u && pot[14] == 2801u && pot[15] == 4066u);
    const cm_path_info pi = node.map_path_info();
    CHECK(pi.start[0] == 3u && pi.start[1] == 2u && pi.goal[0] == 0u && pi.goal[1] == 0u && pi.n_cells == 5u && pi.status == CM_PATH_FOUND && pi.pot_start == 4066u);
    const uint32_t path1[5] = {15, 14, 8, 1, 0};
    CHECK(node.map_path().size() == 5);
    for (size_t k = 0; k < 5 && k < node.map_path().size(); ++k) CHECK(node.map_path()[k] == path1[k]);
    CHECK(node.map_plan_info().goal[0] == 0u && node.map_plan_info().goal[1] == 0u && node.map_plan_info().n_sweeps >= 1u);
    // what the library returns for the same frame on a context of its own: the same words
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 6, 4, c.map_z_band[0], c.map_z_band[1], 85, 40, -200, 350, -40, 85, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_plan_params pp{1, 256, CM_PLAN_ALLOW_UNKNOWN, 24};
        const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_map_plan_configure(ctx, &pp) == CM_BAD_ARG);                                // no cost layer yet
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK);
        CHECK(cm_map_plan_configure(ctx, &pp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        cm_result r2{};
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
        CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_OK);
        CHECK(cm_map_plan_update(ctx, -1.25f, -0.75f, nullptr, nullptr) == CM_BAD_ARG);      // the cost layer is stale
        CHECK(cm_map_cost_update(ctx, nullptr) == CM_OK);
        std::vector<uint32_t> got(24), cells(24, 7u);
        CHECK(cm_map_plan_copy(ctx, got.data(), 24, nullptr, nullptr) == CM_BAD_ARG);        // stale until the update
        cm_plan_info info{};
        CHECK(cm_map_plan_update(ctx, -1.25f, -0.75f, &info, nullptr) == CM_OK && info.goal[0] == 0u && info.goal[1] == 0u);
        CHECK(cm_map_plan_copy(ctx, got.data(), 24, nullptr, nullptr) == CM_OK);
        CHECK(std::memcmp(got.data(), pot.data(), 24 * sizeof(uint32_t)) == 0);
        cm_path_info pj{};
        CHECK(cm_map_plan_path(ctx, 0.0f, 0.0f, cells.data(), 4, &pj) == CM_CAPACITY && cells[0] == 7u && pj.n_cells == 5u);
        CHECK(cm_map_plan_path(ctx, 0.0f, 0.0f, cells.data(), 24, &pj) == CM_OK && std::memcmp(&pj, &pi, sizeof pj) == 0);
        CHECK(std::memcmp(cells.data(), path1, sizeof path1) == 0 && cells[5] == 7u);
        CHECK(cm_map_plan_path(ctx, 0.25f, -0.25f, cells.data(), 24, &pj) == CM_OK && pj.status == CM_PATH_UNREACHABLE && pj.n_cells == 0u);   // the lethal (3, 1)
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing integrated, the tables stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.map_potential().size() == 24 && node.map_path().size() == 5);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
