// ray_tests.cpp — the host shell's free-space ray casting: NodeConfig keys (CPU) and, with "gpu", one node whose sensor sits in
// cell (0, 0) of a 6 x 4 grid and sees two poles and a lone point, checked against known cells and against what the library
// returns for the same frame.
//   ray_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/rays.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.grid_raycast && ref.grid_min_pass == 1 && ref.grid_ray_range == 0);          // off by default
    CHECK(load_text(path, head + "grid_cell 0.25\ngrid_size 160 84\ngrid_raycast 1\ngrid_min_pass 3\ngrid_ray_range 120\n", &c, &err));
    CHECK(c.grid_raycast && c.grid_min_pass == 3 && c.grid_ray_range == 120 && c.grid_cell == 0.25f);
    CHECK(load_text(path, head + "grid_raycast 1\ngrid_cell 0.5   # in either order\n", &c, &err) && c.grid_raycast && c.grid_min_pass == 1);
    CHECK(load_text(path, head + "grid_cell 0.5\ngrid_raycast 0\ngrid_min_pass 2\n", &c, &err) && !c.grid_raycast && c.grid_min_pass == 2);
    CHECK(load_text(path, head + "grid_min_pass 2\ngrid_ray_range 0\n", &c, &err) && !c.grid_raycast);   // the keys alone turn nothing on
    // rejected: casting without a grid, a flag that is no flag, min_pass 0, missing values
    CHECK(!load_text(path, head + "grid_raycast 1\n", &c, &err));
    CHECK(err.find("grid_cell") != std::string::npos);
    CHECK(!load_text(path, head + "grid_cell 0\ngrid_raycast 1\n", &c, &err));
    CHECK(!load_text(path, head + "grid_cell 0.5\ngrid_raycast 2\n", &c, &err));
    CHECK(err.find(":3:") != std::string::npos);
    CHECK(!load_text(path, head + "grid_raycast\n", &c, &err));
    CHECK(!load_text(path, head + "grid_min_pass 0\n", &c, &err));
    CHECK(!load_text(path, head + "grid_min_pass\n", &c, &err));
    CHECK(!load_text(path, head + "grid_ray_range\n", &c, &err));
    // a node configured in code the same way refuses to start
    NodeConfig bad = reference_config();
    bad.sensors = {{"a", "/a", "a_link", true}};
    bad.grid_raycast = true;
    CloudMergerNode node(bad);
    CHECK(!node.ok() && node.error().find("grid_cell") != std::string::npos);
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.grid_cell = 0.5f;
    c.grid_origin[0] = -1.0f;
    c.grid_origin[1] = -1.0f;
    c.grid_nx = 6;
    c.grid_ny = 4;
    c.grid_obstacle_height = 0.3f;
    c.grid_min_points = 1;
    c.grid_raycast = true;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    // the sensor at (-0.75, -0.75): cell (0, 0)
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    node.set_transform(0, q, t);
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    cm_result r{};
    CHECK(node.spin_once(&r) == CM_OK);
    const std::vector<cm_grid_ray_cell>& rays = node.grid_ray_cells();
    const std::vector<int8_t>& cleared = node.grid_cleared();
    const std::vector<int8_t>& occ = node.grid_occupancy();
    CHECK(rays.size() == 24 && cleared.size() == 24 && occ.size() == 24 && node.grid_cells().size() == 24);
    if (rays.size() != 24 || cleared.size() != 24 || occ.size() != 24) return;
    // three rays: to (4, 0) over (0,0) (1,0) (2,0) (3,0); to (2, 0) over (0,0) (1,0); to (2, 1) over (0,0) and — the tie of
    // dx = 2, dy = 1 away from zero — (1, 1)
    const uint32_t want_pass[24] = {3, 2, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t want_end[24] = {0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int8_t want_occ[24] = {-1, -1, 100, -1, 100, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    const int8_t want_clr[24] = {0, 0, 100, 0, 100, -1, -1, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (size_t k = 0; k < 24; ++k) {
        CHECK(rays[k].n_pass == want_pass[k] && rays[k].n_end == want_end[k]);
        CHECK(occ[k] == want_occ[k] && cleared[k] == want_clr[k]);
    }
    // what the library returns for the same frame on a context of its own: the same bytes; and min_pass 2, a range of 1
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        cm_result r2{};
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
        const cm_grid_params gp{{-1.0f, -1.0f}, 0.5f, 6, 4, c.grid_z_band[0], c.grid_z_band[1], 0.3f, 1};
        std::vector<cm_grid_ray_cell> want(24);
        std::vector<int8_t> image(24), base(24);
        uint64_t n_cells = 0;
        CHECK(cm_result_grid_rays(ctx, &gp, nullptr, want.data(), 24) == CM_OK);
        CHECK(cm_grid_ray_occupancy_copy(ctx, image.data(), 24, &n_cells) == CM_OK && n_cells == 24);
        CHECK(cm_grid_occupancy_copy(ctx, base.data(), 24, &n_cells) == CM_OK && n_cells == 24);
        CHECK(std::memcmp(want.data(), rays.data(), 24 * sizeof(cm_grid_ray_cell)) == 0);
        CHECK(std::memcmp(image.data(), cleared.data(), 24) == 0 && std::memcmp(base.data(), occ.data(), 24) == 0);
        const cm_ray_params two{2, 0}, near{1, 1};
        CHECK(cm_result_grid_rays(ctx, &gp, &two, want.data(), 24) == CM_OK);
        CHECK(cm_grid_ray_occupancy_copy(ctx, image.data(), 24, &n_cells) == CM_OK);
        CHECK(std::memcmp(want.data(), rays.data(), 24 * sizeof(cm_grid_ray_cell)) == 0);
        CHECK(image[0] == 0 && image[1] == 0 && image[3] == -1 && image[7] == -1 && image[2] == 100 && image[8] == 0);
        CHECK(cm_result_grid_rays(ctx, &gp, &near, want.data(), 24) == CM_OK);
        CHECK(want[0].n_pass == 3 && want[1].n_pass == 0 && want[7].n_pass == 0 && want[4].n_end == 1);
        cm_destroy(ctx);
    }
    // a frame without fresh clouds: nothing fused, the last frame's tables stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.grid_ray_cells().size() == 24 && node.grid_cleared().size() == 24);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
