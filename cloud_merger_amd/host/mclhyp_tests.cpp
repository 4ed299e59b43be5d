// mclhyp_tests.cpp — the host shell's hypotheses and recovery of the localisation layer: NodeConfig keys and their refusals (CPU;
// a file with mcl_hyp 1 and no mcl 1 is refused), cm_mcl_kld_bound by hand and, with "gpu", one node run through three frames
// whose mcl_info(), mcl_hypotheses() and mcl_hyp_info() must equal what the library returns for the same calls on a context of
// its own.
//   mclhyp_tests <tmpdir> [gpu]
#include <cmath>
#include <cstdlib>

#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/mclhyp.cfg";
    const std::string head = "sensor a /a a_link required\n";
    const std::string mcl = head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\nmcl 1\nmcl_particles 300\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.mcl_hyp_enable && ref.mcl_hyp_bin_q == 512u && ref.mcl_hyp_heading_bits == 5u && ref.mcl_hyp_max == 8u && ref.mcl_inject_max == 0u);     // off by default
    CHECK(ref.mcl_recovery_alpha[0] == 0.05f && ref.mcl_recovery_alpha[1] == 0.5f && ref.mcl_kld_err == 0.05f && ref.mcl_kld_z == 2.326f);
    CHECK(load_text(path, mcl + "mcl_hyp 1\nmcl_hyp_bins 0.25 3\nmcl_hyp_max 64\nmcl_recovery 0.01 0.25 299\nmcl_kld 0.01 3.0\n", &c, &err));
    CHECK(c.mcl_hyp_enable && c.mcl_hyp_bin_q == 256u && c.mcl_hyp_heading_bits == 3u && c.mcl_hyp_max == 64u && c.mcl_inject_max == 299u);
    CHECK(c.mcl_recovery_alpha[0] == 0.01f && c.mcl_recovery_alpha[1] == 0.25f && c.mcl_kld_err == 0.01f && c.mcl_kld_z == 3.0f);
    CHECK(load_text(path, mcl + "mcl_hyp 0   # off\n", &c, &err) && !c.mcl_hyp_enable);
    CHECK(load_text(path, head + "mcl_hyp_bins 0.0625 0\nmcl_hyp_max 1\nmcl_recovery 0 0 0\nmcl_kld 1 0.001\n", &c, &err) && c.mcl_hyp_bin_q == 64u);
    CHECK(load_text(path, head + "mcl_hyp_bins 1024 8\nmcl_recovery 1 1 5\n", &c, &err) && c.mcl_hyp_bin_q == 1048576u && c.mcl_hyp_heading_bits == 8u);
    // the mode without the layer it is a mode of
    CHECK(!load_text(path, head + "mcl_hyp 1\n", &c, &err));
    CHECK(err.find("mcl_hyp needs the localisation layer") != std::string::npos);
    CHECK(!load_text(path, head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\nmcl 0\nmcl_hyp 1\n", &c, &err));
    CHECK(err.find("mcl_hyp needs the localisation layer") != std::string::npos);
    CHECK(!load_text(path, mcl + "mcl_hyp 1\nmcl_recovery 0.05 0.5 300\n", &c, &err));     // inject_max above mcl_particles - 1
    CHECK(err.find("inject_max") != std::string::npos);
    CHECK(load_text(path, mcl + "mcl_hyp 0\nmcl_recovery 0.05 0.5 300\n", &c, &err));      // (only the mode's own check)
    // values outside their ranges, missing values
    CHECK(!load_text(path, head + "mcl_hyp_bins 0.06 5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_bins 1025 5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_bins nan 5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_bins 0.5 9\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_bins 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_max 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp_max 65\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_recovery 0.5 0.25 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_recovery -0.1 0.25 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_recovery 0.1 1.5 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_recovery 0.1 inf 10\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_recovery 0.1 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_kld 0 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_kld 1.5 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_kld 0.05 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_kld 0.05 nan\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_kld 0.05\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_hyp\n", &c, &err));
}

static void test_cpu(const char* tmpdir) {
    test_config_keys(tmpdir);
    // the KLD bound by hand: k = 2, err = 0.5, z = 1: b = 7/9 + sqrt(2/9) = 1.2492, b^3 = 1.9493, times 1: 2
    uint32_t n = 7;
    CHECK(cm_mcl_kld_bound(2, 0.5f, 1.0f, &n) == CM_OK && n == 2u);
    CHECK(cm_mcl_kld_bound(0, 0.5f, 1.0f, &n) == CM_OK && n == 1u);
    CHECK(cm_mcl_kld_bound(1, 0.5f, 1.0f, &n) == CM_OK && n == 1u);
    CHECK(cm_mcl_kld_bound(65536, 1e-9f, 50.0f, &n) == CM_OK && n == 0xFFFFFFFFu);
    n = 7;
    CHECK(cm_mcl_kld_bound(2, 0.0f, 1.0f, &n) == CM_BAD_ARG && cm_mcl_kld_bound(2, 0.5f, 0.0f, &n) == CM_BAD_ARG && n == 7u);
    CHECK(cm_mcl_kld_bound(2, 0.5f, 1.0f, nullptr) == CM_BAD_ARG);
    const cm_mcl_hyp_params hp{512, 5, 8, 0, 0.05f, 0.5f, 0.05f, 2.326f, 0, 0};
    cm_mcl_hyp hyp{};
    hyp.label = 9;
    cm_mcl_hyp_info hi{};
    hi.gen = 7;
    CHECK(cm_map_mcl_hyp_configure(nullptr, &hp) == CM_BAD_ARG && cm_map_mcl_hyp_copy(nullptr, &hyp, 1, &hi) == CM_BAD_ARG && hyp.label == 9u && hi.gen == 7u);
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // mcl_tests' window and frames, with the hypotheses on.
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
    c.mcl_hyp_enable = true;
    c.mcl_hyp_bin_q = 256;
    c.mcl_hyp_heading_bits = 6;
    c.mcl_hyp_max = 4;
    c.mcl_inject_max = 75;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    const float poses[3][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1, 0, 0, 0.25f, 0, 1, 0, -0.125f, 0, 0, 1, 0}, {1, 0, 0, 0.5f, 0, 1, 0, 0.125f, 0, 0, 1, 0}};
    {
        NodeConfig bad = c;                            // a mode the library refuses: the node does not start
        bad.mcl_hyp_bin_q = 63;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_mcl_hyp_configure") != std::string::npos);
    }
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    node.set_transform(0, q, t);
    cm_result r{};
    feed(node, pts, &r);                               // the first frame: the map holds nothing yet, no particles
    CHECK(!node.mcl_started() && node.mcl_hypotheses().empty() && node.mcl_hyp_info().n_bins == 0u);
    CHECK(node.set_pose(poses[1]) == CM_OK);
    feed(node, pts, &r);                               // the second: the particles around the set pose
    CHECK(node.mcl_started() && node.mcl_hypotheses().empty());
    CHECK(node.set_pose(poses[2]) == CM_OK);
    feed(node, pts, &r);                               // the third: predict, update with the hypotheses
    const cm_mcl_info info = node.mcl_info();
    const cm_mcl_hyp_info hi = node.mcl_hyp_info();
    const std::vector<cm_mcl_hyp> hyps = node.mcl_hypotheses();
    CHECK(info.n_particles == 300u && info.gen == 2u && hi.gen == 2u && hi.n_bins >= 1u && hi.n_components >= 1u && hi.n_components <= hi.n_bins);
    CHECK(hyps.size() == hi.n_hyp && hi.n_hyp == std::min<uint32_t>(hi.n_components, 4u) && hi.n_free > 0u && hi.n_inject <= 75u);
    uint64_t in_hyps = 0;
    for (const cm_mcl_hyp& h : hyps) in_hyps += h.n;
    CHECK(in_hyps <= 300u && (hi.n_components > 4u || in_hyps == 300u));
    for (size_t k = 1; k < hyps.size(); ++k) CHECK(hyps[k - 1].sum_w > hyps[k].sum_w || (hyps[k - 1].sum_w == hyps[k].sum_w && hyps[k - 1].label < hyps[k].label));
    // what the library returns for the same calls on a context of its own: the same bytes
    cm_ctx* ctx = nullptr;
    const cm_limits lim{1, 0, 1000};
    CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
    if (!ctx) return;
    const cm_map_params mp{0.5f, 12, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
    const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
    const cm_mcl_params lp{300, 64, 16, 0.25f, 1.0f, 2.0f, c.mcl_resample_frac, 0u, 77};
    const cm_mcl_hyp_params hp{256, 6, 4, 75, c.mcl_recovery_alpha[0], c.mcl_recovery_alpha[1], c.mcl_kld_err, c.mcl_kld_z, 0u, 0u};
    CHECK(cm_map_configure(ctx, &mp) == CM_OK && cm_map_cost_configure(ctx, &cp) == CM_OK);
    CHECK(cm_map_mcl_hyp_configure(ctx, &hp) == CM_BAD_ARG);                                   // no localisation layer yet
    CHECK(cm_map_mcl_configure(ctx, &lp) == CM_OK && cm_map_mcl_hyp_configure(ctx, &hp) == CM_OK);
    CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
    cm_result r2{};
    cm_mcl_info got{};
    cm_mcl_hyp_info got_i{};
    std::vector<cm_mcl_hyp> got_h(CM_MCL_HYP_MAX);
    for (int frame = 0; frame < 3; ++frame) {
        CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
        CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK);
        if (frame == 1) CHECK(cm_map_mcl_init_pose(ctx, 0.25f, -0.125f, 0.0f, 0.4f, 0.3f, 0.1f) == CM_OK);
        if (frame == 2) {
            const float dx = 0.5f - 0.25f, dy = 0.125f - -0.125f, cs = std::cos(0.0f), sn = std::sin(0.0f);
            CHECK(cm_map_mcl_hyp_copy(ctx, got_h.data(), got_h.size(), &got_i) == CM_BAD_ARG);  // no update yet
            CHECK(cm_map_mcl_predict(ctx, cs * dx + sn * dy, cs * dy - sn * dx, 0.0f, c.mcl_noise[0], c.mcl_noise[1], c.mcl_noise[2]) == CM_OK);
            CHECK(cm_map_mcl_update(ctx, &got) == CM_OK && std::memcmp(&got, &info, sizeof got) == 0);
            CHECK(cm_map_mcl_hyp_copy(ctx, got_h.data(), got_h.size(), &got_i) == CM_OK && std::memcmp(&got_i, &hi, sizeof hi) == 0);
            CHECK(got_i.n_hyp == hyps.size() && std::memcmp(got_h.data(), hyps.data(), hyps.size() * sizeof(cm_mcl_hyp)) == 0);
        }
        CHECK(cm_map_integrate(ctx, poses[frame], nullptr) == CM_OK && cm_map_cost_update(ctx, nullptr) == CM_OK);
    }
    cm_destroy(ctx);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_cpu, test_node_on_gpu); }
