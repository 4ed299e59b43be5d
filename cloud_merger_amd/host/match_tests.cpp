// match_tests.cpp — the host shell's scan matching layer behind the cost layer: NodeConfig keys (CPU) and, with "gpu", one node
// that integrates a first frame under a set pose, receives the same scene again with a deliberately wrong set_pose and integrates
// it under the matched pose, checked against the shift worked out by hand and against what the library returns for the same
// calls.
//   match_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/match.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.match_enable && !ref.match_subcell && ref.match_n_a == 10u && ref.match_a_stride == 2u && ref.match_wx == 10u && ref.match_wy == 10u);   // off by default
    CHECK(ref.match_sigma == 0.1f && ref.match_max_dist == 0.5f);
    CHECK(load_text(path, head + "match 1\nmatch_angles 30 4\nmatch_window 20 12\nmatch_field 0.15 0.6\nmatch_subcell 1\n", &c, &err));
    CHECK(c.match_enable && c.match_subcell && c.match_n_a == 30u && c.match_a_stride == 4u && c.match_wx == 20u && c.match_wy == 12u);
    CHECK(c.match_sigma == 0.15f && c.match_max_dist == 0.6f);
    CHECK(load_text(path, head + "match 0   # off\nmatch_subcell 0\n", &c, &err) && !c.match_enable && !c.match_subcell);
    CHECK(load_text(path, head + "match_angles 0 1\nmatch_window 0 0\n", &c, &err) && c.match_n_a == 0u && c.match_wx == 0u);
    CHECK(load_text(path, head + "match_angles 127 8\nmatch_window 64 64\n", &c, &err) && c.match_n_a == 127u && c.match_wy == 64u);
    CHECK(load_text(path, head + "match_angles 1 1024\n", &c, &err) && c.match_a_stride == 1024u);
    // rejected: counts beyond the library's, a field that is none, missing values, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "match_angles 128 1\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "match_angles 3 0\n", &c, &err));
    CHECK(!load_text(path, head + "match_angles 127 9\n", &c, &err));
    CHECK(!load_text(path, head + "match_angles 2 513\n", &c, &err));
    CHECK(!load_text(path, head + "match_angles 3\n", &c, &err));
    CHECK(!load_text(path, head + "match_angles -1 2\n", &c, &err));
    CHECK(!load_text(path, head + "match_window 65 1\n", &c, &err));
    CHECK(!load_text(path, head + "match_window 1 65\n", &c, &err));
    CHECK(!load_text(path, head + "match_window 4\n", &c, &err));
    CHECK(!load_text(path, head + "match_field 0 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "match_field -0.1 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "match_field 0.1 0\n", &c, &err));
    CHECK(!load_text(path, head + "match_field nan 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "match_field 0.1 inf\n", &c, &err));
    CHECK(!load_text(path, head + "match_field 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "match 2\n", &c, &err));
    CHECK(!load_text(path, head + "match\n", &c, &err));
    CHECK(!load_text(path, head + "match_subcell 2\n", &c, &err));
    CHECK(!load_text(path, head + "match_subcell x\n", &c, &err));
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // A window of 12 x 8 cells of 0.5 m around a vehicle at the world's origin (anchor (-6, -4)); the sensor at (-0.75, -0.75).
    // ray_scene's points stand in the middle of the absolute cells (2, -2) (the pole), (0, -2), (0, -1) and (4, -2): window
    // cells (8, 2), (6, 2), (6, 3) and (10, 2), all within 2.4 m of the vehicle, so that a turn of 8 table entries (0.7
    // degrees) leaves every point in its cell and the three angle candidates tie: k = 0.
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.map_cell = 0.5f;
    c.map_nx = 12;
    c.map_ny = 8;
    c.map_inscribed_radius = 0.0f;
    c.map_inflation_radius = 1.0f;
    c.map_cost_scaling = 1.0f;
    c.match_enable = true;
    c.match_n_a = 1;
    c.match_a_stride = 8;
    c.match_wx = 3;
    c.match_wy = 3;
    c.match_sigma = 0.25f;
    c.match_max_dist = 0.5f;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    // two cells to the left, one up: under it every point still falls into the window (two cells to the right would push the
    // point in column 10 out of a window of 12, and a dropped point is not counted)
    const float wrong[12] = {1, 0, 0, -1.0f, 0, 1, 0, 0.5f, 0, 0, 1, 0};
    {
        // a layer the library refuses (such a field cannot come from a file, but can from code): the node does not start
        NodeConfig bad = c;
        bad.match_max_dist = 40.0f;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_match_configure") != std::string::npos);
    }
    {
        // the layer off: the wrong pose is taken as it is
        NodeConfig off = c;
        off.match_enable = false;
        CloudMergerNode node(off);
        CHECK(node.ok());
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);
        CHECK(node.set_pose(wrong) == CM_OK);
        feed(node, pts, &r);
        CHECK(!node.matched() && node.map_info().n_frames == 2u && node.map_info().anchor[0] == -8 && node.map_info().anchor[1] == -3);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(!node.matched());
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);                               // the first frame: nothing to match against, integrated under the identity
    CHECK(!node.matched() && node.map_info().n_frames == 1u && node.map_info().anchor[0] == -6 && node.map_info().anchor[1] == -4);
    CHECK(std::memcmp(node.matched_pose(), identity, sizeof identity) == 0);
    const std::vector<int8_t> image1 = node.map_image();
    CHECK(image1.size() == 96 && image1[2 * 12 + 8] == 100 && image1[2 * 12 + 6] == 100 && image1[3 * 12 + 6] == 100 && image1[2 * 12 + 10] == 100);
    CHECK(node.set_pose(wrong) == CM_OK);
    feed(node, pts, &r);                               // the second: matched back by (+2, -1) cells onto the first
    const cm_match_result mr = node.match_result();
    CHECK(node.matched() && mr.k == 0 && mr.i == 2 && mr.j == -1 && mr.n_cells == 4u && mr.score == 1020u && mr.max_score == 1020u);
    CHECK(mr.best == (1u * 7u + 2u) * 7u + 5u && mr.yaw == 0.0f && mr.sub[0] == 0.0 && mr.sub[1] == 0.0);
    CHECK(std::memcmp(mr.pose, identity, sizeof identity) == 0 && std::memcmp(node.matched_pose(), identity, sizeof identity) == 0);
    CHECK(node.map_info().n_frames == 2u && node.map_info().anchor[0] == -6 && node.map_info().anchor[1] == -4);   // integrated where the first was
    CHECK(node.map_image() == image1 && node.map_cells()[2 * 12 + 8].logodds == 170 && node.map_cells()[2 * 12 + 8].n_obs == 2u);
    // what the library returns for the same calls on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 12, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_match_params qp{0.25f, 0.5f, 1, 8, 3, 3, 0u};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_map_match_configure(ctx, &qp) == CM_BAD_ARG);                                 // no cost layer yet
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK && cm_map_match_configure(ctx, &qp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        cm_result r2{};
        cm_match_result got{};
        for (int frame = 0; frame < 2; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
            if (frame == 0) {
                CHECK(cm_map_match_evaluate(ctx, identity, &got) == CM_BAD_ARG);               // the map holds no frame
                CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_OK);
                CHECK(cm_map_match_evaluate(ctx, identity, &got) == CM_BAD_ARG);               // dist2 is stale
                CHECK(cm_map_cost_update(ctx, nullptr) == CM_OK);
            }
        }
        std::vector<uint32_t> vol(148, 7u);
        CHECK(cm_map_match_copy(ctx, vol.data(), 147, nullptr) == CM_BAD_ARG);                 // stale until the evaluate
        CHECK(cm_map_match_evaluate(ctx, wrong, &got) == CM_OK && std::memcmp(&got, &mr, sizeof got) == 0);
        CHECK(cm_map_match_copy(ctx, vol.data(), 146, nullptr) == CM_CAPACITY && vol[0] == 7u);
        CHECK(cm_map_match_copy(ctx, vol.data(), 147, nullptr) == CM_OK && vol[mr.best] == 1020u && vol[147] == 7u);
        uint32_t largest = 0;
        for (size_t e = 0; e < 147; ++e) largest = vol[e] > largest ? vol[e] : largest;
        CHECK(largest == 1020u);
        CHECK(cm_map_integrate(ctx, got.pose, nullptr) == CM_OK);
        std::vector<cm_map_cell> cells(96);
        CHECK(cm_map_copy(ctx, cells.data(), 96, nullptr) == CM_OK && std::memcmp(cells.data(), node.map_cells().data(), 96 * sizeof(cm_map_cell)) == 0);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing matched, the result stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.matched() && node.match_result().score == 1020u);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
