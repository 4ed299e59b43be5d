// grid_tests.cpp — the host shell's 2-D grid map: NodeConfig keys (CPU) and, with "gpu", one node whose frame holds a flat
// patch, a pole and a lone point, checked against known cells and against what the library returns for the same frame.
//   grid_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/grid.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.grid_cell == 0.0f && ref.grid_nx == 1 && ref.grid_ny == 1 && ref.grid_obstacle_height == 0.3f && ref.grid_min_points == 1);   // off by default
    CHECK(std::isinf(ref.grid_z_band[0]) && ref.grid_z_band[0] < 0 && std::isinf(ref.grid_z_band[1]) && ref.grid_z_band[1] > 0);
    CHECK(load_text(path, head + "grid_cell 0.25\ngrid_origin -20 -10.5\ngrid_size 160 84\ngrid_z_band -0.5 2.5\n"
                                 "grid_obstacle_height 0.2\ngrid_min_points 3\n", &c, &err));
    CHECK(c.grid_cell == 0.25f && c.grid_origin[0] == -20.0f && c.grid_origin[1] == -10.5f && c.grid_nx == 160 && c.grid_ny == 84);
    CHECK(c.grid_z_band[0] == -0.5f && c.grid_z_band[1] == 2.5f && c.grid_obstacle_height == 0.2f && c.grid_min_points == 3);
    CHECK(load_text(path, head + "grid_cell 0.5   # the rest left alone\n", &c, &err));
    CHECK(c.grid_cell == 0.5f && c.grid_nx == 1 && c.grid_obstacle_height == 0.3f && std::isinf(c.grid_z_band[1]));
    CHECK(load_text(path, head + "grid_size 2048 2048\ngrid_cell 0\ngrid_obstacle_height 0\ngrid_z_band 1 1\n", &c, &err) && c.grid_cell == 0.0f);
    // rejected: a cell that is negative or whose inverse overflows, more cells than the library takes, an empty grid, a band
    // upside down, a negative height, min_points 0, missing values
    CHECK(!load_text(path, head + "grid_cell -0.5\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "grid_cell 1e-39\n", &c, &err));
    CHECK(!load_text(path, head + "grid_cell\n", &c, &err));
    CHECK(!load_text(path, head + "grid_origin 1\n", &c, &err));
    CHECK(!load_text(path, head + "grid_size 2049 2048\n", &c, &err));
    CHECK(!load_text(path, head + "grid_size 0 8\n", &c, &err));
    CHECK(!load_text(path, head + "grid_size 8\n", &c, &err));
    CHECK(!load_text(path, head + "grid_z_band 2 1\n", &c, &err));
    CHECK(!load_text(path, head + "grid_z_band 1\n", &c, &err));
    CHECK(!load_text(path, head + "grid_obstacle_height -0.1\n", &c, &err));
    CHECK(!load_text(path, head + "grid_min_points 0\n", &c, &err));
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.grid_cell = 0.5f;
    c.grid_origin[0] = -1.0f;
    c.grid_origin[1] = -1.0f;
    c.grid_nx = 6;
    c.grid_ny = 4;
    c.grid_obstacle_height = 0.3f;
    c.grid_min_points = 2;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    const std::vector<float> pts = grid_scene();
    const int n = static_cast<int>(pts.size() / 4);
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    cm_result r{};
    CHECK(node.spin_once(&r) == CM_OK);
    const std::vector<cm_grid_cell>& cells = node.grid_cells();
    const std::vector<int8_t>& occ = node.grid_occupancy();
    CHECK(cells.size() == 24 && occ.size() == 24);
    if (cells.size() != 24 || occ.size() != 24) return;
    const cm_grid_cell& flat = cells[0];
    CHECK(flat.n == 9 && flat.n_ground == 0 && flat.z_lo == 0.0f && flat.z_hi == 0.01f * 8.0f && flat.i_max == 8.0f && flat.state == CM_GRID_FREE);
    CHECK(std::isnan(flat.g_lo) && std::isnan(flat.g_hi) && occ[0] == 0);
    const cm_grid_cell& pole = cells[3 + 2 * 6];
    CHECK(pole.n == 5 && pole.z_lo == 0.0f && pole.z_hi == 1.0f && pole.i_max == 14.0f && pole.state == CM_GRID_OCCUPIED && occ[3 + 2 * 6] == 100);
    const cm_grid_cell& one = cells[5 + 3 * 6];
    CHECK(one.n == 1 && one.z_lo == 0.5f && one.z_hi == 0.5f && one.state == CM_GRID_UNKNOWN && occ[5 + 3 * 6] == -1);
    uint64_t counted = 0;
    for (const cm_grid_cell& g : cells) counted += g.n;
    CHECK(counted == 15);
    for (size_t k = 0; k < 24; ++k)
        if (k != 0 && k != 15 && k != 23) CHECK(cells[k].n == 0 && cells[k].state == CM_GRID_UNKNOWN && std::isnan(cells[k].z_lo) && occ[k] == -1);
    // what the library returns for the same frame on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        cm_result r2{};
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
        const cm_grid_params gp{{-1.0f, -1.0f}, 0.5f, 6, 4, c.grid_z_band[0], c.grid_z_band[1], 0.3f, 2};
        std::vector<cm_grid_cell> want(24);
        std::vector<int8_t> image(24);
        uint64_t n_cells = 0;
        CHECK(cm_result_grid_map(ctx, &gp, want.data(), 24) == CM_OK);
        CHECK(cm_grid_occupancy_copy(ctx, image.data(), 24, &n_cells) == CM_OK && n_cells == 24);
        CHECK(std::memcmp(want.data(), cells.data(), 24 * sizeof(cm_grid_cell)) == 0);
        CHECK(std::memcmp(image.data(), occ.data(), 24) == 0);
        cm_destroy(ctx);
    }
    // a frame without fresh clouds: nothing fused, the last frame's grid stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.grid_cells().size() == 24 && node.grid_occupancy().size() == 24);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
