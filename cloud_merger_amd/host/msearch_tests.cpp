// msearch_tests.cpp — the host shell's search layer behind the cost layer (branch-and-bound scan matching over wide windows):
// NodeConfig keys (CPU) and, with "gpu", one node that integrates a first frame under a set pose, receives the same scene again
// with a set_pose that is 70 cells off — beyond what the exhaustive layer can search — and integrates it under the matched
// pose, checked against the shift worked out by hand and against what the library returns for the same calls.
//   msearch_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/msearch.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.match_search_enable && ref.match_search_wx == 128u && ref.match_search_wy == 128u && ref.match_search_depth == 5u);     // off by default
    CHECK(ref.match_search_max_nodes == (1u << 18) && ref.match_search_max_cells == (1u << 17));
    CHECK(load_text(path, head + "match_search 1\nmatch_search_window 300 200\nmatch_search_depth 6\nmatch_search_capacity 5000 700\nmatch_angles 30 4\n", &c, &err));
    CHECK(c.match_search_enable && !c.match_enable && c.match_search_wx == 300u && c.match_search_wy == 200u && c.match_search_depth == 6u);
    CHECK(c.match_search_max_nodes == 5000u && c.match_search_max_cells == 700u && c.match_n_a == 30u && c.match_a_stride == 4u);
    CHECK(load_text(path, head + "match_search 0   # off\n", &c, &err) && !c.match_search_enable);
    CHECK(load_text(path, head + "match_search_window 0 0\nmatch_search_depth 0\nmatch_search_capacity 1 1\n", &c, &err) && c.match_search_wx == 0u &&
          c.match_search_depth == 0u && c.match_search_max_cells == 1u);
    CHECK(load_text(path, head + "match_search_window 1024 1024\nmatch_search_depth 7\nmatch_search_capacity 4194304 4194304\n", &c, &err) &&
          c.match_search_wy == 1024u && c.match_search_depth == 7u && c.match_search_max_nodes == (1u << 22));
    CHECK(load_text(path, head + "match 1\nmatch_search 0\n", &c, &err) && c.match_enable && !c.match_search_enable);
    // rejected: both layers at once, counts beyond the library's, missing values, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "match 1\nmatch_search 1\n", &c, &err));
    CHECK(err.find("exclude") != std::string::npos);
    CHECK(!load_text(path, head + "match_search 1\nmatch 1\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_window 1025 1\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "match_search_window 1 1025\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_window 4\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_window -1 4\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_depth 8\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_depth\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_capacity 0 10\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_capacity 10 0\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_capacity 4194305 10\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_capacity 10 4194305\n", &c, &err));
    CHECK(!load_text(path, head + "match_search_capacity 10\n", &c, &err));
    CHECK(!load_text(path, head + "match_search 2\n", &c, &err));
    CHECK(!load_text(path, head + "match_search\n", &c, &err));
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // A window of 240 x 8 cells of 0.5 m around a vehicle at the world's origin (anchor (-120, -4)); the sensor at
    // (-0.75, -0.75). ray_scene's points stand in the middle of the absolute cells (2, -2), (0, -2), (0, -1) and (4, -2): window
    // cells (122, 2), (120, 2), (120, 3) and (124, 2), all within 2.4 m of the vehicle, so that a turn of 8 table entries
    // leaves every point in its cell and the three angle candidates tie: k = 0. The second set_pose is 35 m = 70 cells to the
    // left: under it the points fall into the window cells (52, 2) .. (54, 2), and only the shift (+70, 0) puts all four back
    // onto occupied cells (4 * 255). 161 x 7 shifts at depth 4: 11 root blocks per candidate, the last one partial.
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.map_cell = 0.5f;
    c.map_nx = 240;
    c.map_ny = 8;
    c.map_inscribed_radius = 0.0f;
    c.map_inflation_radius = 1.0f;
    c.map_cost_scaling = 1.0f;
    c.match_search_enable = true;
    c.match_n_a = 1;
    c.match_a_stride = 8;
    c.match_search_wx = 80;
    c.match_search_wy = 3;
    c.match_search_depth = 4;
    c.match_search_max_nodes = 1024;
    c.match_search_max_cells = 64;
    c.match_sigma = 0.25f;
    c.match_max_dist = 0.5f;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float wrong[12] = {1, 0, 0, -35.0f, 0, 1, 0, 0, 0, 0, 1, 0};
    {
        // a layer the library refuses (more roots than max_nodes): the node does not start
        NodeConfig bad = c;
        bad.match_search_max_nodes = 32;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_match_search_configure") != std::string::npos);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(!node.matched());
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);                               // the first frame: nothing to match against, integrated under the identity
    CHECK(!node.matched() && node.map_info().n_frames == 1u && node.map_info().anchor[0] == -120 && node.map_info().anchor[1] == -4);
    CHECK(node.match_search_info().n_roots == 0u);
    const std::vector<int8_t> image1 = node.map_image();
    CHECK(image1.size() == 1920 && image1[2 * 240 + 122] == 100 && image1[2 * 240 + 120] == 100 && image1[3 * 240 + 120] == 100 && image1[2 * 240 + 124] == 100);
    CHECK(node.set_pose(wrong) == CM_OK);
    feed(node, pts, &r);                               // the second: matched back by (+70, 0) cells onto the first
    const cm_match_result mr = node.match_result();
    const cm_match_search_info mi = node.match_search_info();
    CHECK(node.matched() && mr.k == 0 && mr.i == 70 && mr.j == 0 && mr.n_cells == 4u && mr.score == 1020u && mr.max_score == 1020u);
    CHECK(mr.best == (1u * 7u + 3u) * 161u + 150u && mr.yaw == 0.0f && mr.sub[0] == 0.0 && mr.sub[1] == 0.0);
    CHECK(std::memcmp(mr.pose, identity, sizeof identity) == 0 && std::memcmp(node.matched_pose(), identity, sizeof identity) == 0);
    CHECK(mi.depth == 4u && mi.n_roots == 33u && mi.scored[4] == 33u && mi.bound == 1020u && mi.overflow_level == -1 && mi.live[0] == 3u);
    CHECK(mi.live[4] >= 3u && mi.scored[0] < 161u * 7u * 3u / 4u);      // the three tied candidates survive; most of the range is never scored
    CHECK(node.map_info().n_frames == 2u && node.map_info().anchor[0] == -120 && node.map_info().anchor[1] == -4);   // integrated where the first was
    CHECK(node.map_image() == image1 && node.map_cells()[2 * 240 + 122].n_obs == 2u);
    // what the library returns for the same calls on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 240, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_match_search_params sp{0.25f, 0.5f, 1, 8, 80, 3, 4, 1024, 64, 0u};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_map_match_search_configure(ctx, &sp) == CM_BAD_ARG);                          // no cost layer yet
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK && cm_map_match_search_configure(ctx, &sp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        cm_result r2{};
        cm_match_result got{};
        cm_match_search_info gi{};
        for (int frame = 0; frame < 2; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
            if (frame == 0) {
                CHECK(cm_map_match_search(ctx, identity, &got, &gi) == CM_BAD_ARG);            // the map holds no frame
                CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_OK);
                CHECK(cm_map_match_search(ctx, identity, &got, &gi) == CM_BAD_ARG);            // dist2 is stale
                CHECK(cm_map_cost_update(ctx, nullptr) == CM_OK);
            }
        }
        CHECK(cm_map_match_search_result(ctx, &got, &gi) == CM_BAD_ARG);                       // stale until the evaluate
        CHECK(cm_map_match_search(ctx, wrong, &got, &gi) == CM_OK && std::memcmp(&got, &mr, sizeof got) == 0 && std::memcmp(&gi, &mi, sizeof gi) == 0);
        cm_match_result again{};
        CHECK(cm_map_match_search_result(ctx, &again, nullptr) == CM_OK && std::memcmp(&again, &mr, sizeof again) == 0);
        // a cell list one too short: CM_CAPACITY, the overflow named, the result stale again
        const cm_match_search_params tight{0.25f, 0.5f, 1, 8, 80, 3, 4, 1024, 3, 0u};
        CHECK(cm_map_match_search_configure(ctx, &tight) == CM_OK);
        CHECK(cm_map_match_search(ctx, wrong, &got, &gi) == CM_CAPACITY && gi.overflow_level == CM_MATCH_SEARCH_OVERFLOW_CELLS && gi.n_roots == 33u);
        CHECK(cm_map_match_search_result(ctx, &again, nullptr) == CM_BAD_ARG);
        CHECK(cm_map_integrate(ctx, mr.pose, nullptr) == CM_OK);
        std::vector<cm_map_cell> cells(1920);
        CHECK(cm_map_copy(ctx, cells.data(), 1920, nullptr) == CM_OK && std::memcmp(cells.data(), node.map_cells().data(), 1920 * sizeof(cm_map_cell)) == 0);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing matched, the result stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.matched() && node.match_result().score == 1020u && node.match_search_info().n_roots == 33u);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
