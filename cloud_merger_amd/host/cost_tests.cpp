// cost_tests.cpp — the host shell's cost layer over the occupancy map: NodeConfig keys (CPU) and, with "gpu", one node that
// integrates map_tests' two frames with the layer updated behind each, checked against known cells and against what the library
// returns for the same two frames.
//   cost_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/cost.cfg";
    const std::string head = "sensor a /a a_link required\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.map_inscribed_radius == 0.0f && ref.map_inflation_radius == 0.0f && ref.map_cost_scaling == 0.0f && !ref.map_inflate_unknown);   // off by default
    CHECK(load_text(path, head + "map_cell 0.1\nmap_size 100 80\nmap_inflation 0.35 1.05 3\nmap_inflate_unknown 1\n", &c, &err));
    CHECK(c.map_inscribed_radius == 0.35f && c.map_inflation_radius == 1.05f && c.map_cost_scaling == 3.0f && c.map_inflate_unknown);
    CHECK(load_text(path, head + "map_inflation 0 0 0   # an inflation radius of 0 is off\nmap_inflate_unknown 0\n", &c, &err));
    CHECK(c.map_inflation_radius == 0.0f && !c.map_inflate_unknown);
    CHECK(load_text(path, head + "map_inflation 0.5 0 3\n", &c, &err) && c.map_inflation_radius == 0.0f);       // off, whatever the rest says
    CHECK(load_text(path, head + "map_inflation 0.5 0.5 0\n", &c, &err) && c.map_inflation_radius == 0.5f);
    // rejected: radii or a scaling that are not lengths, an inflation radius inside the inscribed one, missing values, a flag
    // that is not 0 or 1
    CHECK(!load_text(path, head + "map_inflation -0.1 1 3\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "map_inflation 0.35 nan 3\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflation 0.35 inf 3\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflation 0.35 1.05 -1\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflation 0.35 0.3 3\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflation 0.35 1.05\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflation\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflate_unknown 2\n", &c, &err));
    CHECK(!load_text(path, head + "map_inflate_unknown\n", &c, &err));
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
    c.map_inscribed_radius = 0.5f;
    c.map_inflation_radius = 1.0f;
    c.map_cost_scaling = 1.0f;
    {
        // a layer the library refuses (more than CM_COST_MAX_RADIUS_CELLS cells): the node does not start, and says why
        NodeConfig bad = c;
        bad.map_inflation_radius = 200.0f;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_cost_configure") != std::string::npos);
    }
    {
        // no inflation radius: the map alone, no tables of the layer
        NodeConfig off = c;
        off.map_inflation_radius = 0.0f;
        CloudMergerNode node(off);
        CHECK(node.ok());
        const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, ray_scene(), &r);
        CHECK(node.map_image().size() == 24 && node.map_cost().empty() && node.map_dist2().empty());
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    CHECK(node.map_cost().empty() && node.map_dist2().empty());
    // map_tests' first frame: the image is
    //   -1   0   0 100   0 100
    //   -1  -1   0 100  -1  -1
    //   -1 (the two rows above)
    // with the obstacles (3, 0), (5, 0), (3, 1). Cells of 0.5 m, radii 0.5 and 1.0, scaling 1: R = 2 and the table is 254, 253
    // (0.5 <= 0.5), 252 e^-0.2071 = 204.9, 252 e^-0.3660 = 174.8, 252 e^-0.5 = 152.8.
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    node.set_transform(0, q, t);
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    cm_result r{};
    feed(node, pts, &r);
    CHECK(node.map_cost().size() == 24 && node.map_dist2().size() == 24 && node.map_image().size() == 24);
    if (node.map_cost().size() != 24 || node.map_dist2().size() != 24) return;
    const uint32_t dist1[24] = {9, 4, 1, 0, 1, 0, 9, 4, 1, 0, 1, 1, 10, 5, 2, 1, 2, 4, 13, 8, 5, 4, 5, 8};
    // row 0: unknown beyond the radius, free at 1.0 m, free at 0.5 m, lethal, free at 0.5 m, lethal; row 1: the unknown cell at
    // 1.0 m stays NO_INFORMATION (152 < 253), the unknown cells at 0.5 m are inscribed; rows 2 and 3: all unknown, (3, 2) at 0.5 m
    const uint8_t cost1[24] = {255, 152, 253, 254, 253, 254, 255, 255, 253, 254, 253, 253, 255, 255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255};
    for (size_t k = 0; k < 24; ++k) {
        CHECK(node.map_dist2()[k] == dist1[k]);
        CHECK(node.map_cost()[k] == cost1[k]);
    }
    const std::vector<uint8_t> first_cost = node.map_cost();
    const std::vector<uint32_t> first_dist = node.map_dist2();
    const float moved[12] = {1, 0, 0, 0.5f, 0, 1, 0, 0, 0, 0, 1, 0};
    CHECK(node.set_pose(moved) == CM_OK);
    feed(node, pts, &r);
    // the second frame's image is 0 0 -1 -1 -1 100 / -1 0 -1 100 -1 -1 / -1 ...: the obstacles (5, 0) and (3, 1)
    CHECK(node.map_dist2()[0] == 10u && node.map_dist2()[5] == 0u && node.map_dist2()[9] == 0u && node.map_dist2()[23] == 8u);
    CHECK(node.map_cost()[5] == 254 && node.map_cost()[9] == 254 && node.map_cost()[0] == 0 && node.map_cost()[7] == 152 && node.map_cost()[4] == 253);
    // what the library returns for the same two frames on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 6, 4, c.map_z_band[0], c.map_z_band[1], 85, 40, -200, 350, -40, 85, 0};
        const cm_cost_params cp{0.5f, 1.0f, 1.0f, 0u};
        const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_BAD_ARG);                                // no map yet
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        uint8_t lut[5] = {0, 0, 0, 0, 0};
        uint64_t n_lut = 0;
        CHECK(cm_map_cost_table_copy(ctx, lut, 5, &n_lut) == CM_OK && n_lut == 5);
        CHECK(lut[0] == 254 && lut[1] == 253 && lut[2] == 204 && lut[3] == 174 && lut[4] == 152);
        std::vector<uint8_t> cost(24);
        std::vector<uint32_t> dist(24);
        cm_map_info info{};
        for (int frame = 0; frame < 2; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            cm_result r2{};
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
            CHECK(cm_map_integrate(ctx, frame ? moved : identity, nullptr) == CM_OK);
            CHECK(cm_map_cost_copy(ctx, cost.data(), 24, nullptr) == CM_BAD_ARG);            // stale until the update
            CHECK(cm_map_cost_update(ctx, &info) == CM_OK && info.n_frames == static_cast<uint64_t>(frame + 1));
            CHECK(cm_map_cost_copy(ctx, cost.data(), 24, nullptr) == CM_OK);
            CHECK(cm_map_dist_copy(ctx, dist.data(), 24, nullptr) == CM_OK);
            CHECK(std::memcmp(cost.data(), (frame ? node.map_cost() : first_cost).data(), 24) == 0);
            CHECK(std::memcmp(dist.data(), (frame ? node.map_dist2() : first_dist).data(), 24 * sizeof(uint32_t)) == 0);
        }
        CHECK(std::memcmp(&info, &node.map_info(), sizeof info) == 0);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing integrated, the tables stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.map_cost().size() == 24 && node.map_dist2().size() == 24);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
