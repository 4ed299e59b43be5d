// mcl_tests.cpp — the host shell's localisation layer behind the cost layer: NodeConfig keys and their refusals (CPU; a file
// with mcl 1 and no cost layer is refused) and, with "gpu", one node run through three frames with mcl_init pose — the first
// builds the map, the second initialises the particles, the third predicts and updates — whose mcl_info() and mcl_particles()
// must equal what the library returns for the same calls on a context of its own.
//   mcl_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/mcl.cfg";
    const std::string head = "sensor a /a a_link required\n";
    const std::string cost = head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.mcl_enable && !ref.mcl_init_uniform && !ref.mcl_resample_always && ref.mcl_particles == 2048u && ref.mcl_max_beams == 256u);   // off by default
    CHECK(ref.mcl_range_cells == 256u && ref.mcl_sigma == 0.1f && ref.mcl_max_dist == 0.5f && ref.mcl_tau == 8.0f && ref.mcl_resample_frac == 0.5f && ref.mcl_seed == 1u);
    CHECK(load_text(path, cost + "mcl 1\nmcl_particles 4096\nmcl_beams 512 300\nmcl_field 0.15 0.6\nmcl_tau 4.5\nmcl_resample 0.25 1\nmcl_seed 18446744073709551615\n"
                                 "mcl_init pose 0.3 0.4 0.1\nmcl_noise 0.03 0.02 0.01\n", &c, &err));
    CHECK(c.mcl_enable && c.mcl_particles == 4096u && c.mcl_max_beams == 512u && c.mcl_range_cells == 300u && c.mcl_sigma == 0.15f && c.mcl_max_dist == 0.6f);
    CHECK(c.mcl_tau == 4.5f && c.mcl_resample_frac == 0.25f && c.mcl_resample_always && c.mcl_seed == 18446744073709551615ull && !c.mcl_init_uniform);
    CHECK(c.mcl_init_sd[0] == 0.3f && c.mcl_init_sd[1] == 0.4f && c.mcl_init_sd[2] == 0.1f && c.mcl_noise[0] == 0.03f && c.mcl_noise[1] == 0.02f && c.mcl_noise[2] == 0.01f);
    CHECK(load_text(path, cost + "mcl 1\nmcl_init uniform\n", &c, &err) && c.mcl_enable && c.mcl_init_uniform);
    CHECK(load_text(path, cost + "mcl 0   # off\n", &c, &err) && !c.mcl_enable);
    CHECK(load_text(path, head + "mcl 0\nmcl_particles 1\nmcl_beams 1 1\n", &c, &err) && c.mcl_particles == 1u && c.mcl_range_cells == 1u);
    CHECK(load_text(path, head + "mcl_particles 65536\nmcl_beams 8192 1024\nmcl_resample 1 0\nmcl_init pose 0 0 1024\nmcl_noise 0 0 0\n", &c, &err) && c.mcl_max_beams == 8192u);
    // it needs the cost layer: without a map, or with a map and no inflation, the file is refused
    CHECK(!load_text(path, head + "mcl 1\n", &c, &err));
    CHECK(err.find("mcl needs the cost layer") != std::string::npos);
    CHECK(!load_text(path, head + "map_cell 0.5\nmap_size 12 8\nmcl 1\n", &c, &err) && err.find("mcl needs the cost layer") != std::string::npos);
    {
        NodeConfig bad = reference_config();           // ... and so is such a config made in code: the node does not start
        bad.mcl_enable = true;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("mcl needs the cost layer") != std::string::npos);
    }
    // rejected: counts beyond the library's, values that are none, missing values, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "mcl_particles 0\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "mcl_particles 65537\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_particles\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beams 0 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beams 8193 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beams 10 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beams 10 1025\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beams 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_field 0 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_field 0.1 -1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_field nan 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_field 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_tau 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_tau -2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_tau inf\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_resample 1.5 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_resample -0.1 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_resample 0.5 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_resample 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_seed x\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_init\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_init somewhere\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_init pose 0.1 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_init pose 0.1 -0.1 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_init pose 0.1 0.1 1025\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_noise 0.1 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_noise 0.1 nan 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_noise -1 0 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl\n", &c, &err));
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // match_tests' window: 12 x 8 cells of 0.5 m, the sensor at (-0.75, -0.75), ray_scene's points in four cells around the vehicle.
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.map_cell = 0.5f;
    c.map_nx = 12;
    c.map_ny = 8;
    c.map_inscribed_radius = 0.0f;
    c.map_inflation_radius = 1.0f;
    c.map_cost_scaling = 1.0f;
    c.mcl_enable = true;
    c.mcl_particles = 300;
    c.mcl_max_beams = 64;
    c.mcl_range_cells = 16;
    c.mcl_sigma = 0.25f;
    c.mcl_max_dist = 1.0f;
    c.mcl_tau = 2.0f;
    c.mcl_seed = 77;
    c.mcl_init_sd[0] = 0.4f;
    c.mcl_init_sd[1] = 0.3f;
    c.mcl_init_sd[2] = 0.1f;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    const float poses[3][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1, 0, 0, 0.25f, 0, 1, 0, -0.125f, 0, 0, 1, 0}, {1, 0, 0, 0.5f, 0, 1, 0, 0.125f, 0, 0, 1, 0}};
    {
        NodeConfig bad = c;                            // a layer the library refuses: the node does not start
        bad.mcl_max_dist = 40.0f;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_mcl_configure") != std::string::npos);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);                               // the first frame: the map holds nothing yet, no particles
    CHECK(!node.mcl_started() && node.mcl_particles().empty() && node.map_info().n_frames == 1u);
    CHECK(node.set_pose(poses[1]) == CM_OK);
    feed(node, pts, &r);                               // the second: the particles around the set pose
    CHECK(node.mcl_started() && node.mcl_particles().size() == 300u && node.mcl_info().n_particles == 0u && node.map_info().n_frames == 2u);
    const std::vector<cm_mcl_particle> first = node.mcl_particles();
    CHECK(node.set_pose(poses[2]) == CM_OK);
    feed(node, pts, &r);                               // the third: predict with the motion between the two set poses, update
    const cm_mcl_info info = node.mcl_info();
    CHECK(info.n_particles == 300u && info.gen == 2u && info.n_cells == 4u && info.n_beams == 4u && info.stride == 1u && info.sum_w >= 65536u);
    CHECK(node.map_info().n_frames == 3u && node.map_info().anchor[0] == -5 && node.map_info().anchor[1] == -4);    // integrated under the set pose
    // what the library returns for the same calls on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (ctx) {
        const cm_map_params mp{0.5f, 12, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_mcl_params lp{300, 64, 16, 0.25f, 1.0f, 2.0f, c.mcl_resample_frac, 0u, 77};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK);
        CHECK(cm_map_mcl_configure(ctx, &lp) == CM_BAD_ARG);                                   // no cost layer yet
        CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK && cm_map_mcl_configure(ctx, &lp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        cm_result r2{};
        cm_mcl_info got{};
        std::vector<cm_mcl_particle> parts(300);
        for (int frame = 0; frame < 3; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
            if (frame == 0) CHECK(cm_map_mcl_update(ctx, &got) == CM_BAD_ARG);                 // the map holds no frame
            if (frame == 1) {
                CHECK(cm_map_mcl_predict(ctx, 0.1f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f) == CM_BAD_ARG);   // no particles yet
                CHECK(cm_map_mcl_init_pose(ctx, 0.25f, -0.125f, 0.0f, 0.4f, 0.3f, 0.1f) == CM_OK);
                CHECK(cm_map_mcl_copy(ctx, parts.data(), 300) == CM_OK && std::memcmp(parts.data(), first.data(), 300 * sizeof(cm_mcl_particle)) == 0);
            }
            if (frame == 2) {
                const float dx = 0.5f - 0.25f, dy = 0.125f - -0.125f, cs = std::cos(0.0f), sn = std::sin(0.0f);
                CHECK(cm_map_mcl_predict(ctx, cs * dx + sn * dy, cs * dy - sn * dx, 0.0f, c.mcl_noise[0], c.mcl_noise[1], c.mcl_noise[2]) == CM_OK);
                CHECK(cm_map_mcl_update(ctx, &got) == CM_OK && std::memcmp(&got, &info, sizeof got) == 0);
                CHECK(cm_map_mcl_copy(ctx, parts.data(), 299) == CM_CAPACITY);
                CHECK(cm_map_mcl_copy(ctx, parts.data(), 300) == CM_OK);
                CHECK(std::memcmp(parts.data(), node.mcl_particles().data(), 300 * sizeof(cm_mcl_particle)) == 0);
            }
            CHECK(cm_map_integrate(ctx, poses[frame], nullptr) == CM_OK && cm_map_cost_update(ctx, nullptr) == CM_OK);
        }
        std::vector<cm_map_cell> cells(96);
        CHECK(cm_map_copy(ctx, cells.data(), 96, nullptr) == CM_OK && std::memcmp(cells.data(), node.map_cells().data(), 96 * sizeof(cm_map_cell)) == 0);
        cm_destroy(ctx);
    }
    // a tick without fresh clouds: nothing fused, nothing predicted, the belief stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.mcl_info().gen == 2u && std::memcmp(&info, &node.mcl_info(), sizeof info) == 0);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
