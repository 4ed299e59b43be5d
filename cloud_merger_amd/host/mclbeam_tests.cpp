// mclbeam_tests.cpp — the host shell's beam model of the localisation layer: NodeConfig keys and their refusals (CPU; a file with
// mcl_beam 1 and no mcl 1 is refused), the generalised arithmetic of csrc/cm_cast_math.hpp (the very code k_mcl_beam compiles:
// lines of |d| <= 1450 followed up to 64 steps past their end, both walks, one and three rays at a time) against a walk written
// with `/` on the CPU, the table of cm_mcl_beam_table by hand and, with "gpu", one node run through three frames whose
// mcl_info() and mcl_beam_info() must equal what the library returns for the same calls on a context of its own.
//   mclbeam_tests <tmpdir> [gpu]
#include <algorithm>
#include <cstdlib>

#include "../csrc/cm_cast_math.hpp"
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/mclbeam.cfg";
    const std::string head = "sensor a /a a_link required\n";
    const std::string mcl = head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\nmcl 1\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.mcl_beam_enable && !ref.mcl_beam_plain && ref.mcl_beam_sigma == 0.1f && ref.mcl_beam_over_cells == 8u);      // off by default
    CHECK(ref.mcl_beam_mix[0] == 0.75f && ref.mcl_beam_mix[1] == 0.125f && ref.mcl_beam_mix[2] == 0.125f);
    CHECK(load_text(path, mcl + "mcl_beam 1\nmcl_beam_model 0.2 12\nmcl_beam_mix 0.5 0.25 0.125\nmcl_beam_plain 1\n", &c, &err));
    CHECK(c.mcl_beam_enable && c.mcl_beam_sigma == 0.2f && c.mcl_beam_over_cells == 12u && c.mcl_beam_plain);
    CHECK(c.mcl_beam_mix[0] == 0.5f && c.mcl_beam_mix[1] == 0.25f && c.mcl_beam_mix[2] == 0.125f);
    CHECK(load_text(path, mcl + "mcl_beam 0   # off\n", &c, &err) && !c.mcl_beam_enable);
    CHECK(load_text(path, head + "mcl_beam_model 0.05 0\nmcl_beam_mix 1 0 0\nmcl_beam_plain 0\n", &c, &err) && c.mcl_beam_over_cells == 0u && c.mcl_beam_mix[0] == 1.0f);
    CHECK(load_text(path, head + "mcl_beam_model 3 64\nmcl_beam_mix 0.5 0.25 0.25\n", &c, &err) && c.mcl_beam_over_cells == 64u);
    // it needs the localisation layer
    CHECK(!load_text(path, head + "mcl_beam 1\n", &c, &err));
    CHECK(err.find("mcl_beam needs the localisation layer") != std::string::npos);
    CHECK(!load_text(path, head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\nmcl 0\nmcl_beam 1\n", &c, &err));
    CHECK(err.find("mcl_beam needs the localisation layer") != std::string::npos);
    // rejected: values beyond the library's, values that are none, missing values, a flag that is not 0 or 1
    CHECK(!load_text(path, head + "mcl_beam_model 0.1 65\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "mcl_beam_model 0 8\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_model -0.1 8\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_model nan 8\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_model 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0 0.5 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0.5 -0.1 0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0.5 0.1 -0.1\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0.8 0.1 0.1\n", &c, &err));             // as fp32 the three add up to more than 1
    CHECK(!load_text(path, head + "mcl_beam_mix 0.5 0.5 0.5\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0.5 inf 0\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_mix 0.5 0.25\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam_plain 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam 2\n", &c, &err));
    CHECK(!load_text(path, head + "mcl_beam\n", &c, &err));
}

// Steps 3 to 5 of the beam model with the C++ integer division: k | status << 16 as cm_cast_math.hpp's reach forms return it.
static int rdiv(int a, int L) { return a < 0 ? -((2 * -a + L) / (2 * L)) : (2 * a + L) / (2 * L); }

static uint32_t reach_by_division(int dx, int dy, int over, int ox, int oy, int nx, int ny, const int8_t* image) {
    const int L = std::max(std::abs(dx), std::abs(dy));
    for (int k = 0; k <= L + over; ++k) {
        const int cx = ox + rdiv(k * dx, L), cy = oy + rdiv(k * dy, L);
        if (cx < 0 || cx >= nx || cy < 0 || cy >= ny) return static_cast<uint32_t>(k - 1) | (2u << 16);
        if (image[cy * nx + cx] == 100) return static_cast<uint32_t>(k) | (1u << 16);
    }
    return static_cast<uint32_t>(L + over);
}

// The skip table of an image by brute force over its occupied cells, through cm_cast_step_of.
static std::vector<unsigned char> steps_of(const std::vector<int8_t>& image, int nx, int ny) {
    std::vector<unsigned char> steps(image.size());
    std::vector<std::pair<int, int>> occ;
    for (int v = 0; v < ny; ++v)
        for (int u = 0; u < nx; ++u)
            if (image[v * nx + u] == 100) occ.push_back({u, v});
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            uint32_t d2 = CM_MAP_DIST_NONE;
            for (const auto& o : occ) d2 = std::min(d2, static_cast<uint32_t>((o.first - x) * (o.first - x) + (o.second - y) * (o.second - y)));
            steps[y * nx + x] = static_cast<unsigned char>(cm_cast_step_of(d2, 255u));
        }
    return steps;
}

static void test_arithmetic(const char* tmpdir) {
    test_config_keys(tmpdir);
    static_assert(CM_CAST_MAX_D == CM_MCL_BEAM_MAX_D && CM_CAST_MAX_OVER == CM_MCL_BEAM_MAX_OVER, "the header's constants are the library's");
    // the line's cell at the beam model's bound: every k of a few lines next to 1450, against `/`
    int bad = 0;
    for (int L : {1, 2, 1025, 1447, 1450})
        for (int am : {0, 1, L / 2, L - 1, L})
            for (int sx : {-1, 1}) {
                const CmCastLine ln = cm_cast_line(sx * L, am);
                for (int k = 0; k <= L + 64; ++k) {
                    int32_t jx, jy;
                    cm_cast_cell(ln, static_cast<uint32_t>(k), &jx, &jy);
                    bad += jx != sx * k || jy != rdiv(k * am, L);
                }
            }
    CHECK(bad == 0);
    // both walks, one ray and three rays at a time, against the walk by division: random windows and densities, short lines in
    // small windows and lines up to the bound in long ones, over_cells 0, 1, 3, 8 and 64
    std::srand(11);
    const int overs[5] = {0, 1, 3, 8, 64};
    bad = 0;
    int rays = 0, hits = 0, offs = 0, beyonds = 0;
    for (int round = 0; round < 40; ++round) {
        const bool wide = round % 4 == 3;
        const int nx = round == 0 ? 1 : wide ? 1600 + std::rand() % 600 : 2 + std::rand() % 47, ny = round == 1 ? 1 : wide ? 2 + std::rand() % 6 : 2 + std::rand() % 47;
        const int pct = wide ? round % 3 == 0 : ((round / 5) % 5) * 5, reach = wide ? 1450 : 45;
        std::vector<int8_t> image(static_cast<size_t>(nx) * ny);
        for (auto& v : image) v = std::rand() % (wide ? 1000 : 100) < pct ? 100 : (std::rand() % 2 ? 0 : -1);
        const std::vector<unsigned char> steps = steps_of(image, nx, ny);
        const signed char* const img = reinterpret_cast<const signed char*>(image.data());
        for (int t = 0; t < 3000; t += 3) {
            const int over = overs[std::rand() % 5], ox = std::rand() % nx, oy = std::rand() % ny;
            CmCastLine ln[3];
            bool live[3];
            uint32_t want[3], skip[3] = {7u, 7u, 7u}, plain[3] = {7u, 7u, 7u};
            for (int i = 0; i < 3; ++i) {
                int dx = 0, dy = 0;
                while (dx == 0 && dy == 0) {
                    dx = std::rand() % (2 * reach + 1) - reach;
                    dy = wide && std::rand() % 2 ? std::rand() % 9 - 4 : std::rand() % (2 * reach + 1) - reach;
                }
                ln[i] = cm_cast_line(dx, dy);
                live[i] = std::rand() % 8 != 0;
                want[i] = live[i] ? reach_by_division(dx, dy, over, ox, oy, nx, ny, image.data()) : 7u;
                if (live[i]) {
                    bad += cm_cast_reach_skip(ln[i], over, ox, oy, nx, ny, steps.data()) != want[i];
                    bad += cm_cast_reach_plain(ln[i], over, ox, oy, nx, ny, img) != want[i];
                    ++rays;
                    hits += (want[i] >> 16) == 1u;
                    offs += (want[i] >> 16) == 2u;
                    beyonds += (want[i] >> 16) == 0u;
                }
            }
            cm_cast_reach_skip_n<3>(ln, live, over, ox, oy, nx, ny, steps.data(), skip);
            cm_cast_reach_plain_n<3>(ln, live, over, ox, oy, nx, ny, img, plain);
            for (int i = 0; i < 3; ++i) bad += skip[i] != want[i] || plain[i] != want[i];      // (a ray that is not live keeps its 7)
        }
    }
    CHECK(bad == 0);
    CHECK(rays > 90000 && hits > 10000 && offs > 10000 && beyonds > 2000);
    // the cast layer's walks are the reach forms with over = 0
    {
        const std::vector<int8_t> image = {0, 0, 0, 100, 0, 0, 0, 0};
        const std::vector<unsigned char> steps = steps_of(image, 8, 1);
        const CmCastWords w = cm_cast_walk_skip(5, 0, 0, 0, 8, 1, steps.data());
        CHECK(w.a == (3u | (1u << 16)) && w.b == 3u && cm_cast_reach_skip(cm_cast_line(2, 0), 1u, 0, 0, 8, 1, steps.data()) == (3u | (1u << 16)));
        CHECK(cm_cast_reach_skip(cm_cast_line(2, 0), 0u, 0, 0, 8, 1, steps.data()) == 2u && cm_cast_reach_skip(cm_cast_line(-2, 0), 3u, 1, 0, 8, 1, steps.data()) == (1u | (2u << 16)));
    }
    // the table by hand: sums of exactly 1, ties to even, a sigma so small that only e == 0 is above the floor
    uint8_t tab[8] = {7, 7, 7, 7, 7, 7, 7, 7};
    const cm_mcl_beam_params p1{1, 1e-3f, 0.5f, 0.25f, 0.25f, 0u};
    CHECK(cm_mcl_beam_table(&p1, 0.1f, tab, 4) == CM_CAPACITY && tab[0] == 7);
    CHECK(cm_mcl_beam_table(&p1, 0.1f, tab, 8) == CM_OK && tab[0] == 64 && tab[1] == 191 && tab[2] == 128 && tab[3] == 128 && tab[4] == 64 && tab[5] == 7);
    const cm_mcl_beam_params p2{65, 0.1f, 0.5f, 0.25f, 0.25f, 0u}, p3{1, 0.1f, 0.8f, 0.1f, 0.1f, 0u}, p4{1, 0.1f, 0.5f, 0.25f, 0.25f, 2u};
    CHECK(cm_mcl_beam_table(&p2, 0.1f, tab, 8) == CM_BAD_ARG && cm_mcl_beam_table(&p3, 0.1f, tab, 8) == CM_BAD_ARG && cm_mcl_beam_table(&p4, 0.1f, tab, 8) == CM_BAD_ARG);
    CHECK(cm_mcl_beam_table(nullptr, 0.1f, tab, 8) == CM_BAD_ARG && cm_mcl_beam_table(&p1, 0.1f, nullptr, 8) == CM_BAD_ARG && cm_mcl_beam_table(&p1, 0.0f, tab, 8) == CM_BAD_ARG);
    cm_mcl_beam_info bi{7, 7, 7, 7, 7, 7, 7};
    CHECK(cm_map_mcl_beam_configure(nullptr, &p1) == CM_BAD_ARG && cm_map_mcl_beam_info_copy(nullptr, &bi) == CM_BAD_ARG && bi.n_rays == 7u && bi.n_skipped == 7u);
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // mcl_tests' window and frames, with the beam model on.
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
    c.mcl_beam_enable = true;
    c.mcl_beam_sigma = 0.5f;
    c.mcl_beam_over_cells = 3;
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
    const std::vector<float> pts = ray_scene();
    const int n = static_cast<int>(pts.size() / 4);
    const float poses[3][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1, 0, 0, 0.25f, 0, 1, 0, -0.125f, 0, 0, 1, 0}, {1, 0, 0, 0.5f, 0, 1, 0, 0.125f, 0, 0, 1, 0}};
    {
        NodeConfig bad = c;                            // a mode the library refuses: the node does not start
        bad.mcl_beam_mix[0] = 0.9f;
        bad.mcl_beam_mix[1] = 0.2f;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cm_map_mcl_beam_configure") != std::string::npos);
    }
    for (int plain = 0; plain < 2; ++plain) {
        c.mcl_beam_plain = plain != 0;
        CloudMergerNode node(c);
        CHECK(node.ok());
        if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);                           // the first frame: the map holds nothing yet, no particles
        CHECK(!node.mcl_started() && node.mcl_beam_info().n_rays == 0u);
        CHECK(node.set_pose(poses[1]) == CM_OK);
        feed(node, pts, &r);                           // the second: the particles around the set pose
        CHECK(node.mcl_started() && node.mcl_beam_info().n_rays == 0u);
        CHECK(node.set_pose(poses[2]) == CM_OK);
        feed(node, pts, &r);                           // the third: predict, update under the beam model
        const cm_mcl_info info = node.mcl_info();
        const cm_mcl_beam_info bi = node.mcl_beam_info();
        CHECK(info.n_particles == 300u && info.gen == 2u && info.n_beams == 4u && bi.n_rays == 1200u);
        CHECK(bi.n_early + bi.n_at + bi.n_late + bi.n_beyond + bi.n_off + bi.n_skipped == bi.n_rays);
        // what the library returns for the same calls on a context of its own: the same bytes
        cm_ctx* ctx = nullptr;
        const cm_limits lim{1, 0, 1000};
        CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
        if (!ctx) return;
        const cm_map_params mp{0.5f, 12, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
        const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
        const cm_mcl_params lp{300, 64, 16, 0.25f, 1.0f, 2.0f, c.mcl_resample_frac, 0u, 77};
        const cm_mcl_beam_params bp{3, 0.5f, c.mcl_beam_mix[0], c.mcl_beam_mix[1], c.mcl_beam_mix[2], plain ? CM_MCL_BEAM_PLAIN : 0u};
        CHECK(cm_map_configure(ctx, &mp) == CM_OK && cm_map_cost_configure(ctx, &cp) == CM_OK);
        CHECK(cm_map_mcl_beam_configure(ctx, &bp) == CM_BAD_ARG);                              // no localisation layer yet
        CHECK(cm_map_mcl_configure(ctx, &lp) == CM_OK && cm_map_mcl_beam_configure(ctx, &bp) == CM_OK);
        CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
        cm_result r2{};
        cm_mcl_info got{};
        cm_mcl_beam_info got_b{};
        for (int frame = 0; frame < 3; ++frame) {
            CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
            CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK);
            if (frame == 1) CHECK(cm_map_mcl_init_pose(ctx, 0.25f, -0.125f, 0.0f, 0.4f, 0.3f, 0.1f) == CM_OK);
            if (frame == 2) {
                const float dx = 0.5f - 0.25f, dy = 0.125f - -0.125f, cs = std::cos(0.0f), sn = std::sin(0.0f);
                CHECK(cm_map_mcl_beam_info_copy(ctx, &got_b) == CM_BAD_ARG);                   // no update yet
                CHECK(cm_map_mcl_predict(ctx, cs * dx + sn * dy, cs * dy - sn * dx, 0.0f, c.mcl_noise[0], c.mcl_noise[1], c.mcl_noise[2]) == CM_OK);
                CHECK(cm_map_mcl_update(ctx, &got) == CM_OK && std::memcmp(&got, &info, sizeof got) == 0);
                CHECK(cm_map_mcl_beam_info_copy(ctx, &got_b) == CM_OK && std::memcmp(&got_b, &bi, sizeof bi) == 0);
            }
            CHECK(cm_map_integrate(ctx, poses[frame], nullptr) == CM_OK && cm_map_cost_update(ctx, nullptr) == CM_OK);
        }
        cm_destroy(ctx);
    }
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_arithmetic, test_node_on_gpu); }
