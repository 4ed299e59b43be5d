// map_tests.cpp — the host shell's occupancy map: NodeConfig keys (CPU) and, with "gpu", one node that integrates ray_tests' scene
// twice, the second time one cell further along x, checked against known cells and against what the library returns for the
// same two frames.
//   map_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/map.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.map_cell == 0.0f && ref.map_l_hit == 85 && ref.map_l_miss == 40 && ref.map_l_min == -200 && ref.map_l_max == 350);   // off by default
    CHECK(ref.map_l_free == -40 && ref.map_l_occ == 85 && ref.map_ray_range == 0 && ref.map_nx == 1 && ref.map_ny == 1);
    CHECK(load_text(path, head + "map_cell 0.1\nmap_size 1000 800\nmap_z_band -0.5 2.5\nmap_logodds 70 30 -150 300\nmap_thresholds -30 70\n"
                                 "map_ray_range 250\n", &c, &err));
    CHECK(c.map_cell == 0.1f && c.map_nx == 1000 && c.map_ny == 800 && c.map_z_band[0] == -0.5f && c.map_z_band[1] == 2.5f);
    CHECK(c.map_l_hit == 70 && c.map_l_miss == 30 && c.map_l_min == -150 && c.map_l_max == 300 && c.map_l_free == -30 && c.map_l_occ == 70);
    CHECK(c.map_ray_range == 250);
    CHECK(load_text(path, head + "map_size 8 8   # the size alone turns nothing on\n", &c, &err) && c.map_cell == 0.0f && c.map_nx == 8);
    CHECK(load_text(path, head + "map_cell 0\n", &c, &err) && c.map_cell == 0.0f);
    // rejected: a cell that is not a length, a window of no cells or of too many, a band upside down, steps below 1, clamps that
    // do not hold 0, thresholds in the wrong order, missing values
    CHECK(!load_text(path, head + "map_cell -0.5\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "map_cell nan\n", &c, &err));
    CHECK(!load_text(path, head + "map_cell\n", &c, &err));
    CHECK(!load_text(path, head + "map_size 0 8\n", &c, &err));
    CHECK(!load_text(path, head + "map_size 2049 2048\n", &c, &err));
    CHECK(!load_text(path, head + "map_size 8\n", &c, &err));
    CHECK(!load_text(path, head + "map_z_band 1 0\n", &c, &err));
    CHECK(!load_text(path, head + "map_logodds 0 40 -200 350\n", &c, &err));
    CHECK(!load_text(path, head + "map_logodds 85 0 -200 350\n", &c, &err));
    CHECK(!load_text(path, head + "map_logodds 85 40 1 350\n", &c, &err));
    CHECK(!load_text(path, head + "map_logodds 85 40 -200\n", &c, &err));
    CHECK(!load_text(path, head + "map_thresholds 85 85\n", &c, &err));
    CHECK(!load_text(path, head + "map_thresholds -40\n", &c, &err));
    CHECK(!load_text(path, head + "map_ray_range\n", &c, &err));
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
    {
        // a map the library refuses: the node does not start, and says why
        NodeConfig bad = c;
        bad.map_l_free = 90;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_configure") != std::string::npos);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(node.map_cells().empty() && node.map_image().empty() && node.map_info().n_frames == 0);
    // The identity pose: the vehicle in cell (0, 0), the window's anchor (-3, -2). The sensor at (-0.75, -0.75) is window cell
    // (1, 0); ray_scene()'s poles are window cells (5, 0) and (3, 0), its lone point (3, 1), its last point outside.
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    node.set_transform(0, q, t);
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    cm_result r{};
    feed(node, pts, &r);
    CHECK(node.map_cells().size() == 24 && node.map_image().size() == 24);
    if (node.map_cells().size() != 24 || node.map_image().size() != 24) return;
    CHECK(node.map_info().anchor[0] == -3 && node.map_info().anchor[1] == -2 && node.map_info().n_frames == 1 &&
          node.map_info().sensors_cast == 1u && node.map_info().nx == 6 && node.map_info().ny == 4);
    // three rays from (1, 0): to (5, 0) over (1,0) (2,0) (3,0) (4,0); to (3, 0) over (1,0) (2,0); to (3, 1) over (1,0) and (2,1).
    // A hit wins over the pass in (3, 0).
    const int32_t want1[24] = {0, -120, -80, 85, -40, 85, 0, 0, -40, 85, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int8_t image1[24] = {-1, 0, 0, 100, 0, 100, -1, -1, 0, 100, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (size_t k = 0; k < 24; ++k) {
        CHECK(node.map_cells()[k].logodds == want1[k] && node.map_cells()[k].n_obs == (want1[k] != 0 ? 1u : 0u));
        CHECK(node.map_image()[k] == image1[k]);
    }
    const std::vector<cm_map_cell> first = node.map_cells();
    // the vehicle one cell further along x: the window scrolls by one column, the evidence per window cell is the same
    const float moved[12] = {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, 0};
    const float bad_pose[12] = {1, 0, 0, NAN, 0, 1, 0, 0, 0, 0, 1, 0};
    CHECK(node.set_pose(bad_pose) == CM_BAD_ARG && node.set_pose(moved) == CM_OK);
    feed(node, pts, &r);
    CHECK(node.map_info().anchor[0] == -2 && node.map_info().anchor[1] == -2 && node.map_info().n_frames == 2);
    const int32_t want2[24] = {-120, -200, 5, 45, 45, 85, 0, -40, 45, 85, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t obs2[24] = {1, 2, 2, 2, 2, 1, 0, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int8_t image2[24] = {0, 0, -1, -1, -1, 100, -1, 0, -1, 100, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (size_t k = 0; k < 24; ++k) {
        CHECK(node.map_cells()[k].logodds == want2[k] && node.map_cells()[k].n_obs == obs2[k]);
        CHECK(node.map_image()[k] == image2[k]);
    }
    // what the library returns for the same two frames on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 6, 4, c.map_z_band[0], c.map_z_band[1], 85, 40, -200, 350, -40, 85, 0};
        const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        std::vector<cm_map_cell> want(24);
        std::vector<int8_t> image(24);
        cm_map_info info{};
        for (int frame = 0; frame < 2; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            cm_result r2{};
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
            CHECK(cm_map_integrate(ctx, frame ? moved : identity, &info) == CM_OK && info.n_frames == static_cast<uint64_t>(frame + 1));
            CHECK(cm_map_integrate(ctx, identity, nullptr) == CM_BAD_ARG);                 // each frame at most once
            CHECK(cm_map_copy(ctx, want.data(), 24, nullptr) == CM_OK);
            CHECK(cm_map_occupancy_copy(ctx, image.data(), 24, nullptr) == CM_OK);
            const std::vector<cm_map_cell>& got = frame ? node.map_cells() : first;
            CHECK(std::memcmp(want.data(), got.data(), 24 * sizeof(cm_map_cell)) == 0);
            if (frame) CHECK(std::memcmp(image.data(), node.map_image().data(), 24) == 0);
        }
        CHECK(std::memcmp(&info, &node.map_info(), sizeof info) == 0);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing integrated, the map stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.map_cells().size() == 24 && node.map_info().n_frames == 2);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
