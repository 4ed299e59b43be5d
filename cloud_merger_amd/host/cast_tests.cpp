// cast_tests.cpp — the host shell's cast layer behind the cost layer: NodeConfig keys and their refusals (a file with cast 1 and
// no cost layer is refused) and the layer's arithmetic (csrc/cm_cast_math.hpp, the very code the kernel compiles) against a walk
// written with `/` over random windows, all on the CPU; and, with "gpu", one node run through two frames with cast 1 whose
// cast_rays() and cast_info() must equal what the library returns for the same calls on a context of its own, in both modes,
// and the walk written with `/` over the node's own image.
//   cast_tests <tmpdir> [gpu]
#include <cstdlib>

#include "../csrc/cm_cast_math.hpp"
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/cast.cfg";
    const std::string head = "sensor a /a a_link required\n";
    const std::string cost = head + "map_cell 0.5\nmap_size 12 8\nmap_inflation 0.0 1.0 1.0\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.cast_enable && !ref.cast_plain && ref.cast_bearings == 360u && ref.cast_range_cells == 256u);      // off by default
    CHECK(load_text(path, cost + "cast 1\ncast_bearings 720\ncast_range 300\ncast_plain 1\n", &c, &err));
    CHECK(c.cast_enable && c.cast_bearings == 720u && c.cast_range_cells == 300u && c.cast_plain);
    CHECK(load_text(path, cost + "cast 0   # off\n", &c, &err) && !c.cast_enable);
    CHECK(load_text(path, head + "cast 0\ncast_bearings 1\ncast_range 1\n", &c, &err) && c.cast_bearings == 1u && c.cast_range_cells == 1u);
    CHECK(load_text(path, head + "cast_bearings 4096\ncast_range 1024\ncast_plain 0\n", &c, &err) && c.cast_bearings == 4096u && !c.cast_plain);
    // it needs the cost layer: without a map, or with a map and no inflation, the file is refused
    CHECK(!load_text(path, head + "cast 1\n", &c, &err));
    CHECK(err.find("cast needs the cost layer") != std::string::npos);
    CHECK(!load_text(path, head + "map_cell 0.5\nmap_size 12 8\ncast 1\n", &c, &err) && err.find("cast needs the cost layer") != std::string::npos);
    {
        NodeConfig bad = reference_config();           // ... and so is such a config made in code: the node does not start
        bad.cast_enable = true;
        CloudMergerNode node(bad);
        CHECK(!node.ok() && node.error().find("cast needs the cost layer") != std::string::npos);
    }
    CHECK(!load_text(path, head + "cast_bearings 0\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "cast_bearings 4097\n", &c, &err));
    CHECK(!load_text(path, head + "cast_bearings\n", &c, &err));
    CHECK(!load_text(path, head + "cast_range 0\n", &c, &err));
    CHECK(!load_text(path, head + "cast_range 1025\n", &c, &err));
    CHECK(!load_text(path, head + "cast_range x\n", &c, &err));
    CHECK(!load_text(path, head + "cast_plain 2\n", &c, &err));
    CHECK(!load_text(path, head + "cast 2\n", &c, &err));
    CHECK(!load_text(path, head + "cast\n", &c, &err));
}

// Steps 4 and 5 of the semantics with the C++ integer division: what both walks of cm_cast_math.hpp must return.
static int rdiv(int a, int L) { return a < 0 ? -((2 * -a + L) / (2 * L)) : (2 * a + L) / (2 * L); }

static cm_cast_ray walk_by_division(int dx, int dy, int ox, int oy, int nx, int ny, const int8_t* image) {
    const int L = std::max(std::abs(dx), std::abs(dy));
    for (int k = 0; k <= L; ++k) {
        const int cx = ox + rdiv(k * dx, L), cy = oy + rdiv(k * dy, L);
        if (cx < 0 || cx >= nx || cy < 0 || cy >= ny)
            return cm_cast_ray{static_cast<uint16_t>(k - 1), CM_CAST_OFF_MAP, 0, static_cast<int16_t>(rdiv((k - 1) * dx, L)), static_cast<int16_t>(rdiv((k - 1) * dy, L))};
        if (image[cy * nx + cx] == 100) return cm_cast_ray{static_cast<uint16_t>(k), CM_CAST_HIT, 0, static_cast<int16_t>(cx - ox), static_cast<int16_t>(cy - oy)};
    }
    return cm_cast_ray{static_cast<uint16_t>(L), CM_CAST_MAX, 0, static_cast<int16_t>(dx), static_cast<int16_t>(dy)};
}

static bool same_ray(const CmCastWords& w, const cm_cast_ray& r) {
    cm_cast_ray g;
    std::memcpy(&g, &w, sizeof g);
    return std::memcmp(&g, &r, sizeof g) == 0;
}

// The skip table of an image by brute force over its occupied cells, through cm_cast_step_of.
static std::vector<unsigned char> steps_of(const std::vector<int8_t>& image, int nx, int ny) {
    std::vector<unsigned char> steps(image.size());
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            uint32_t d2 = CM_MAP_DIST_NONE;
            for (int v = 0; v < ny; ++v)
                for (int u = 0; u < nx; ++u)
                    if (image[v * nx + u] == 100) d2 = std::min(d2, static_cast<uint32_t>((u - x) * (u - x) + (v - y) * (v - y)));
            steps[y * nx + x] = static_cast<unsigned char>(cm_cast_step_of(d2, 255u));
        }
    return steps;
}

static void test_arithmetic(const char* tmpdir) {
    test_config_keys(tmpdir);
    // the quotient: every n on a stride and the neighbourhood of every multiple, for every divisor of a line and of a ray index
    int bad = 0;
    for (uint32_t d = 1; d <= 4096u; ++d) {
        const float rd = 1.0f / static_cast<float>(d);
        const uint32_t top = d < 2u ? (1u << 21) - 1u : (1u << 22) - 1u;          // (n / d < 2^21)
        for (uint32_t n = 0; n <= top; n += 997u) bad += cm_cast_quot(n, d, rd) != n / d;
        for (uint32_t m = 1; m * d <= top && m < 4096u; m += 7u)
            for (int o = -1; o <= 1; ++o) bad += cm_cast_quot(m * d + o, d, rd) != (m * d + o) / d;
        bad += cm_cast_quot(top, d, rd) != top / d;
        for (uint32_t m : {4097u, 40000u, 65535u})                      // a ray index: n < 2^24, n / d < 2^16
            for (int o = -1; o <= 1; ++o) {
                const uint32_t n = std::min(m * d + o, (1u << 24) - 1u);
                bad += cm_cast_quot(n, d, rd) != n / d;
            }
    }
    CHECK(bad == 0);
    // the skip count: j* by its definition
    bad = 0;
    for (uint32_t d2 = 0; d2 <= 140000u; ++d2) {
        uint32_t j = 1;
        while (2u * j * j < d2) ++j;
        bad += cm_cast_step_of(d2, 255u) != (d2 == 0u ? 0u : std::min(j, 255u));
    }
    CHECK(bad == 0 && cm_cast_step_of(CM_MAP_DIST_NONE, 255u) == 255u && cm_cast_step_of(2u * 2047u * 2047u, 255u) == 255u);
    // both walks against the walk by division: random windows and densities, every direction table of a few ranges
    std::srand(7);
    std::vector<int16_t> dirs(2 * 4096);
    const uint32_t ranges[5] = {1, 7, 40, 300, 1024};
    bad = 0;
    int rays = 0, hits = 0, offs = 0;
    for (int round = 0; round < 40; ++round) {
        const int nx = round == 0 ? 1 : 2 + std::rand() % 47, ny = round == 1 ? 1 : 2 + std::rand() % 47, pct = ((round / 5) % 5) * 5;
        std::vector<int8_t> image(static_cast<size_t>(nx) * ny);
        for (auto& v : image) v = std::rand() % 100 < pct ? 100 : (std::rand() % 2 ? 0 : -1);
        const std::vector<unsigned char> steps = steps_of(image, nx, ny);
        CHECK(cm_cast_directions(ranges[round % 5], dirs.data(), 4096) == CM_OK);
        for (int t = 0; t < 3000; ++t) {
            const int e = std::rand() % 4096, ox = std::rand() % nx, oy = std::rand() % ny;
            const int dx = dirs[2 * e], dy = dirs[2 * e + 1];
            const cm_cast_ray want = walk_by_division(dx, dy, ox, oy, nx, ny, image.data());
            const bool ok = same_ray(cm_cast_walk_skip(dx, dy, ox, oy, nx, ny, steps.data()), want) &&
                            same_ray(cm_cast_walk_plain(dx, dy, ox, oy, nx, ny, reinterpret_cast<const signed char*>(image.data())), want);
            bad += !ok;
            ++rays;
            hits += want.status == CM_CAST_HIT;
            offs += want.status == CM_CAST_OFF_MAP;
        }
    }
    CHECK(bad == 0 && rays == 120000 && hits > 10000 && offs > 10000);
    int16_t small[8];
    CHECK(cm_cast_directions(1, small, 4095) == CM_CAPACITY && cm_cast_directions(0, dirs.data(), 4096) == CM_BAD_ARG);
    CHECK(cm_cast_directions(1025, dirs.data(), 4096) == CM_BAD_ARG && cm_cast_directions(5, nullptr, 4096) == CM_BAD_ARG);
}

static void feed(CloudMergerNode& node, const std::vector<float>& pts, cm_result* r) {
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    CHECK(node.spin_once(r) == CM_OK);
}

static void test_node_on_gpu() {
    // mcl_tests' window: 12 x 8 cells of 0.5 m, the sensor at (-0.75, -0.75), ray_scene's points in four cells around the vehicle.
    for (int plain = 0; plain < 2; ++plain) {
        NodeConfig c = single_sensor_config(0.125f, 1000);
        c.map_cell = 0.5f;
        c.map_nx = 12;
        c.map_ny = 8;
        c.map_inscribed_radius = 0.0f;
        c.map_inflation_radius = 1.0f;
        c.map_cost_scaling = 1.0f;
        c.cast_enable = true;
        c.cast_bearings = 90;
        c.cast_range_cells = 9;
        c.cast_plain = plain != 0;
        const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};
        const std::vector<float> pts = ray_scene();
        const int n = static_cast<int>(pts.size() / 4);
        const float cy = std::cos(0.3f), sy = std::sin(0.3f);
        const float poses[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {cy, -sy, 0, 0.25f, sy, cy, 0, -0.125f, 0, 0, 1, 0}};
        CloudMergerNode node(c);
        CHECK(node.ok());
        if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
        node.set_transform(0, q, t);
        cm_result r{};
        feed(node, pts, &r);
        CHECK(node.cast_rays().size() == 90u && node.cast_info().n_poses == 1u && node.cast_info().n_bearings == 90u);
        CHECK(node.set_pose(poses[1]) == CM_OK);
        feed(node, pts, &r);
        const cm_cast_info info = node.cast_info();
        CHECK(node.cast_rays().size() == 90u && info.n_max + info.n_hit + info.n_off_map + info.n_no_origin == 90u && info.n_hit > 0u && info.n_no_origin == 0u);
        // the walk by division over the node's own image
        std::vector<int16_t> dirs(2 * 4096);
        CHECK(cm_cast_directions(9, dirs.data(), 4096) == CM_OK);
        const cm_map_info mi = node.map_info();
        const int ox = static_cast<int>(std::floor(0.25f * (1.0f / 0.5f))) - mi.anchor[0], oy = static_cast<int>(std::floor(-0.125f * (1.0f / 0.5f))) - mi.anchor[1];
        const uint32_t h = static_cast<uint32_t>(static_cast<int64_t>(std::rint(std::atan2(static_cast<double>(sy), static_cast<double>(cy)) * (4294967296.0 / 6.283185307179586))));
        int bad = 0;
        for (uint32_t a = 0; a < 90u && node.cast_rays().size() == 90u; ++a) {
            const uint32_t H = h + static_cast<uint32_t>((static_cast<uint64_t>(a) << 32) / 90u), e = ((H + 0x80000u) >> 20) & 4095u;
            const cm_cast_ray want = walk_by_division(dirs[2 * e], dirs[2 * e + 1], ox, oy, 12, 8, node.map_image().data());
            bad += std::memcmp(&want, &node.cast_rays()[a], sizeof want) != 0;
        }
        CHECK(bad == 0);
        // what the library returns for the same calls on a context of its own: the same bytes
        cm_ctx* ctx = nullptr;
        const cm_limits lim{1, 0, 1000};
        CHECK(cm_create(&ctx, c.device, &lim) == CM_OK);
        if (ctx) {
            const cm_map_params mp{0.5f, 12, 8, c.map_z_band[0], c.map_z_band[1], c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max, c.map_l_free, c.map_l_occ, 0};
            const cm_cost_params cp{0.0f, 1.0f, 1.0f, 0u};
            const cm_cast_params kp{1u, 90u, 9u, plain ? CM_CAST_PLAIN : 0u};
            CHECK(cm_map_configure(ctx, &mp) == CM_OK);
            CHECK(cm_map_cast_configure(ctx, &kp, nullptr) == CM_BAD_ARG);                         // no cost layer yet
            CHECK(cm_map_cost_configure(ctx, &cp) == CM_OK && cm_map_cast_configure(ctx, &kp, nullptr) == CM_OK);
            CHECK(cm_set_sensor_transform(ctx, 0, q, t) == CM_OK);
            cm_result r2{};
            cm_cast_info got{};
            std::vector<cm_cast_ray> rays(90);
            const cm_cast_pose pose{0.25f, -0.125f, h};
            for (int frame = 0; frame < 2; ++frame) {
                CHECK(cm_submit_cloud(ctx, 0, pts.data(), static_cast<uint32_t>(n), 16, 0, 4, 8, 12) == CM_OK);
                CHECK(cm_merge_voxelize(ctx, &c.params, &r2) == CM_OK && r2.status == CM_OK && r2.n_out == r.n_out);
                CHECK(cm_map_integrate(ctx, poses[frame], nullptr) == CM_OK);
                CHECK(cm_map_cast_evaluate(ctx, &pose, 1u, &got) == CM_BAD_ARG);                   // dist2 is stale
                CHECK(cm_map_cost_update(ctx, nullptr) == CM_OK);
                CHECK(cm_map_cast_copy(ctx, rays.data(), 90, nullptr) == CM_BAD_ARG);              // and so are the rays
            }
            CHECK(cm_map_cast_evaluate(ctx, &pose, 1u, &got) == CM_OK && std::memcmp(&got, &info, sizeof got) == 0);
            CHECK(cm_map_cast_copy(ctx, rays.data(), 89, nullptr) == CM_CAPACITY);
            CHECK(cm_map_cast_copy(ctx, rays.data(), 90, nullptr) == CM_OK);
            CHECK(node.cast_rays().size() == 90u && std::memcmp(rays.data(), node.cast_rays().data(), 90 * sizeof(cm_cast_ray)) == 0);
            cm_destroy(ctx);
        }
    }
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_arithmetic, test_node_on_gpu); }
