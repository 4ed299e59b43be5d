// front_tests.cpp — the host shell's frontier layer behind the plan layer: NodeConfig keys (CPU) and, with "gpu", one node
// that integrates map_tests' first frame with the cost layer, the plan to the vehicle's own cell and the frontiers updated
// behind it, checked against a table worked out by hand and against what the library returns for the same frame.
//   front_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/front.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.map_frontier_min_cells == 0u && ref.map_frontier_max == 256u && ref.map_frontier_max_cost == 252u);   // off by default
    CHECK(ref.map_frontier_pot_scale == 1u && ref.map_frontier_gain_scale == 0u && !ref.map_goal_vehicle);
    CHECK(load_text(path, head + "map_cell 0.1\nmap_size 100 80\nmap_inflation 0.35 1.05 3\nmap_plan 50 205\nmap_frontier 4 1000\n"
                                 "map_frontier_max_cost 100\nmap_frontier_scales 3 20\nmap_goal_vehicle 1\n", &c, &err));
    CHECK(c.map_frontier_min_cells == 4u && c.map_frontier_max == 1000u && c.map_frontier_max_cost == 100u);
    CHECK(c.map_frontier_pot_scale == 3u && c.map_frontier_gain_scale == 20u && c.map_goal_vehicle && !c.map_has_goal);
    CHECK(load_text(path, head + "map_frontier 0 1   # min_cells 0 is off\nmap_goal_vehicle 0\n", &c, &err));
    CHECK(c.map_frontier_min_cells == 0u && c.map_frontier_max == 1u && !c.map_goal_vehicle);
    CHECK(load_text(path, head + "map_frontier 1 65536\nmap_frontier_max_cost 0\nmap_frontier_scales 0 4294967295\n", &c, &err));
    CHECK(c.map_frontier_max == CM_FRONTIER_MAX_TABLE && c.map_frontier_max_cost == 0u && c.map_frontier_gain_scale == 0xFFFFFFFFu);
    // rejected: a table beyond the library's range or empty, a cost byte above 252, missing values, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "map_frontier 1 65537\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "map_frontier 1 0\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier 1\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier 4 -1\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier_max_cost 253\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier_max_cost\n", &c, &err));
    CHECK(!load_text(path, head + "map_frontier_scales 1\n", &c, &err));
    CHECK(!load_text(path, head + "map_goal_vehicle 2\n", &c, &err));
    CHECK(!load_text(path, head + "map_goal_vehicle\n", &c, &err));
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static bool same_entry(const cm_frontier& a, const cm_frontier& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

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
    c.map_goal_vehicle = true;                         // no map_goal: the plan's goal is the pose's cell, (3, 2) under the identity
    c.map_frontier_min_cells = 1;
    c.map_frontier_max = 8;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    {
        // a layer the library refuses (a cost byte above 252 cannot come from a file, but can from code): the node does not start
        NodeConfig bad = c;
        bad.map_frontier_max_cost = 253;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_frontier_configure") != std::string::npos);
    }
    {
        // max_cost 0 admits no free cell of this frame (the lowest cost byte is 92): no frontier, no goal to explore, and the
        // frame stands; error() says why
        NodeConfig none = c;
        none.map_frontier_max_cost = 0;
        CloudMergerNode node(none);
        CHECK(node.ok());
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);
        float x = 7.0f, y = 7.0f;
        CHECK(node.map_potential().size() == 24 && node.frontiers().empty() && node.frontier_info().n_frontier_cells == 0u);
        CHECK(node.frontier_info().best == CM_FRONTIER_NONE && !node.explore_goal(&x, &y) && x == 7.0f && y == 7.0f);
        CHECK(node.error().find("explore") != std::string::npos);
    }
    {
        // the layer off: a plan to the vehicle's cell, no table
        NodeConfig off = c;
        off.map_frontier_min_cells = 0;
        CloudMergerNode node(off);
        CHECK(node.ok());
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);
        CHECK(node.map_potential().size() == 24 && node.map_potential()[15] == 0u && node.frontiers().empty() && !node.explore_goal(nullptr, nullptr));
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(node.frontiers().empty() && !node.explore_goal(nullptr, nullptr));
    // map_tests' first frame: the image, the cost table and the weights 1 + cost (unknown cells count as 252) are
    //   -1   0   0 100   0 100      255  92 152 254 152 254      253  93 153   X 153   X
    //   -1  -1   0 100  -1  -1      255 255 152 254 255 255      253 253 153   X 253 253
    //   -1 (the two rows above)     255 (the two rows above)     253 (the two rows above)
    // Frontier cells: (1, 0) has the unknown (0, 0) beside it, (2, 1) the unknown (1, 1), (4, 0) the unknown (4, 1) below it;
    // (2, 0) has free, occupied and free cells around it and the window's edge above: none. (1, 0) and (2, 1) touch at a corner:
    // one frontier, cells 1 and 8; (4, 0) stands alone between two occupied cells: cell 4.
    // The goal is the vehicle cell (3, 2). (2, 2) = 5 * 253 = 1265; (2, 1) = 1265 + 5 * 153 = 2030 (the diagonal from the goal
    // would cut the corner of the lethal (3, 1)); (1, 0) = 2030 + 7 * 93 = 2681 over the diagonal. (4, 2) = 1265, (4, 1) = 2530,
    // (4, 0) = 2530 + 5 * 153 = 3295. With pot_scale 1 and gain_scale 0 the first frontier is the best one, at 2030, and the
    // place to drive to is the centre of (2, 1): ((-3 + 2 + 0.5) * 0.5, (-2 + 1 + 0.5) * 0.5).
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);
    CHECK(node.map_potential().size() == 24 && node.frontiers().size() == 2);
    if (node.map_potential().size() != 24 || node.frontiers().size() != 2) { std::printf("  %s\n", node.error().c_str()); return; }
    const std::vector<uint32_t>& pot = node.map_potential();
    CHECK(pot[15] == 0u && pot[14] == 1265u && pot[8] == 2030u && pot[1] == 2681u && pot[10] == 2530u && pot[4] == 3295u);
    const cm_frontier want0{1u, 2u, 3u, 1u, 2030u, 8u, 1, 0, 2, 1}, want1{4u, 1u, 4u, 0u, 3295u, 4u, 4, 0, 4, 0};
    CHECK(same_entry(node.frontiers()[0], want0) && same_entry(node.frontiers()[1], want1));
    const cm_frontier_info fi = node.frontier_info();
    CHECK(fi.n_frontier_cells == 3u && fi.n_components == 2u && fi.n_frontiers == 2u && fi.n_written == 2u && fi.best == 0u && fi.best_score == 2030);
    float gx = 0.0f, gy = 0.0f;
    CHECK(node.explore_goal(&gx, &gy) && gx == -0.25f && gy == -0.25f);
    CHECK(node.map_path_info().status == CM_PATH_FOUND && node.map_path_info().n_cells == 1u);       // the vehicle stands on its goal
    // what the library returns for the same frame on a context of its own: the same bytes, and the labels
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 6, 4, c.map_z_band[0], c.map_z_band[1], 85, 40, -200, 350, -40, 85, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_plan_params pp{1, 256, CM_PLAN_ALLOW_UNKNOWN, 24};
        const cm_frontier_params fp{1, 8, 252, 1, 0};
        const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK && cm_map_cost_configure(ctx, &cp) == CM_OK);
        CHECK(cm_map_frontier_configure(ctx, &fp) == CM_BAD_ARG);                            // no plan layer yet
        CHECK(cm_map_plan_configure(ctx, &pp) == CM_OK && cm_map_frontier_configure(ctx, &fp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        cm_result r2{};
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
        CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_OK && cm_map_cost_update(ctx, nullptr) == CM_OK);
        CHECK(cm_map_frontier_update(ctx, nullptr, nullptr) == CM_BAD_ARG);                  // the plan layer is stale
        CHECK(cm_map_plan_update(ctx, 0.0f, 0.0f, nullptr, nullptr) == CM_OK);
        std::vector<cm_frontier> got(8);
        std::vector<uint32_t> labels(24, 7u);
        CHECK(cm_map_frontier_copy(ctx, got.data(), 8, nullptr) == CM_BAD_ARG);              // stale until the update
        cm_frontier_info info{}, info2{};
        CHECK(cm_map_frontier_update(ctx, &info, nullptr) == CM_OK && std::memcmp(&info, &fi, sizeof info) == 0);
        CHECK(cm_map_frontier_copy(ctx, got.data(), 1, &info2) == CM_CAPACITY && std::memcmp(&info2, &fi, sizeof fi) == 0);
        CHECK(cm_map_frontier_copy(ctx, got.data(), 8, nullptr) == CM_OK && same_entry(got[0], want0) && same_entry(got[1], want1));
        CHECK(cm_map_frontier_labels_copy(ctx, labels.data(), 23, nullptr) == CM_CAPACITY && labels[0] == 7u);
        CHECK(cm_map_frontier_labels_copy(ctx, labels.data(), 24, nullptr) == CM_OK);
        for (uint32_t k = 0; k < 24; ++k) CHECK(labels[k] == (k == 1u || k == 8u ? 0u : k == 4u ? 1u : CM_FRONTIER_NONE));
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing integrated, the tables stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.frontiers().size() == 2 && node.explore_goal(nullptr, nullptr));
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
