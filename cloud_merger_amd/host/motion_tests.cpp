// motion_tests.cpp — the host shell's ego-motion compensation: NodeConfig keys (CPU) and, with "gpu", one node that fuses
// two moving sensors — one with a per-point time field — checked against the compensation restated here in fp32.
//   motion_tests <tmpdir> [gpu]
#include <algorithm>
#include <array>

#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/motion.cfg";
    NodeConfig c;
    std::string err;
    CHECK(!reference_config().motion_compensation);
    CHECK(load_text(path, "sensor a /a a_link required\nsensor b /b b_link optional\n"
                          "motion_compensation 1\ntime_field b 18 f32\ntime_field a 16 u32ns   # ouster t\n", &c, &err));
    CHECK(c.motion_compensation);
    CHECK(c.time_field[0].offset == 16 && c.time_field[0].type == CM_TIME_U32_NS);
    CHECK(c.time_field[1].offset == 18 && c.time_field[1].type == CM_TIME_F32_S);
    CHECK(c.time_field[2].type == CM_TIME_NONE);
    CHECK(load_text(path, "sensor a /a a_link required\nmotion_compensation 0\n", &c, &err) && !c.motion_compensation);
    CHECK(c.time_field[0].type == CM_TIME_NONE);
    // rejected: unknown sensor, unknown type, missing offset, a flag other than 0/1
    CHECK(!load_text(path, "sensor a /a a_link required\ntime_field z 16 f32\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, "sensor a /a a_link required\ntime_field a 16 f64\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\ntime_field a f32\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\nmotion_compensation 2\n", &c, &err));
}

// The compensation of include/cloudmerge.h (cm_set_ego_motion) in fp32, this file being built with -ffp-contract=off.
static std::array<float, 3> compensate(const float p[3], float dt, const float v[3], const float w[3]) {
    auto cross = [](const float a[3], const float b[3], float o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    float k[3], c[3], e[3];
    cross(w, v, k); cross(w, p, c); cross(w, c, e);
    const float h = 0.5f * (dt * dt);
    std::array<float, 3> o;
    for (int a = 0; a < 3; ++a) o[a] = p[a] + ((dt * (c[a] + v[a])) + (h * (e[a] + k[a])));
    return o;
}

static void test_node_on_gpu() {
    NodeConfig c = reference_config();
    c.sensors = {{"a", "/a", "a_link", true}, {"b", "/b", "b_link", true}};
    c.params.crop_enable = 0;
    c.params.min_points_per_voxel = 0;
    c.params.leaf[0] = c.params.leaf[1] = c.params.leaf[2] = 0.01f;
    c.publish_pcl_layout = false;
    c.motion_compensation = true;
    c.time_field[0] = NodeConfig::TimeField{16, CM_TIME_F32_S};
    c.max_points_total = 1000;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    node.set_transform(1, q, t);
    const uint64_t T = 1700000000000000000ull;
    node.set_clock([T] { return T; });
    const float v[3] = {12.0f, 0.5f, 0.0f}, w[3] = {0.0f, 0.01f, 0.4f};
    CHECK(node.set_ego_twist(v, w) == CM_OK);
    const float bad[3] = {NAN, 0, 0};
    CHECK(node.set_ego_twist(bad, w) == CM_BAD_ARG);
    // sensor a: x,y,z,intensity + time f32 @16 (step 20), 30 ms before the clock; sensor b: x,y,z,intensity, 60 ms before
    const int n = 40;
    PointCloud2 ma;
    ma.height = 1; ma.width = n; ma.point_step = 20; ma.row_step = 20 * n;
    ma.fields = {{"x", 0, PointField::FLOAT32, 1}, {"y", 4, PointField::FLOAT32, 1}, {"z", 8, PointField::FLOAT32, 1},
                 {"intensity", 12, PointField::FLOAT32, 1}, {"time", 16, PointField::FLOAT32, 1}};
    ma.data.resize(20 * n);
    ma.header.stamp_ns = T - 30000000ull;
    PointCloud2 mb = make_xyzi16_message(n);
    mb.header.stamp_ns = T - 60000000ull;
    std::vector<std::array<float, 4>> want;
    for (int i = 0; i < n; ++i) {
        const float pa[4] = {1.0f + 0.7f * i, -3.0f + 0.31f * i, 0.05f * i, 1.0f * i}, tau = 0.0025f * i;
        std::memcpy(ma.data.data() + 20 * i, pa, 16);
        std::memcpy(ma.data.data() + 20 * i + 16, &tau, 4);
        const float pb[4] = {-2.0f - 0.9f * i, 4.0f - 0.17f * i, 1.0f - 0.03f * i, 100.0f + i};
        std::memcpy(mb.data.data() + 16 * i, pb, 16);
        const float dta = static_cast<float>(-30000000.0 * 1e-9) + tau, dtb = static_cast<float>(-60000000.0 * 1e-9);
        const auto oa = compensate(pa, dta, v, w), ob = compensate(pb, dtb, v, w);
        want.push_back({oa[0], oa[1], oa[2], pa[3]});
        want.push_back({ob[0], ob[1], ob[2], pb[3]});
    }
    std::vector<std::array<float, 4>> got;
    uint64_t stamp = 0;
    node.set_publisher([&](const std::string&, const PointCloud2& out) {
        stamp = out.header.stamp_ns;
        got.resize(out.num_points());
        for (size_t i = 0; i < got.size(); ++i) std::memcpy(got[i].data(), out.data.data() + 16 * i, 16);
    });
    CHECK(node.on_cloud(0, ma) == CM_OK && node.on_cloud(1, mb) == CM_OK);
    cm_result r{};
    CHECK(node.spin_once(&r) == CM_OK);
    CHECK(r.path_flags & CM_PATH_MOTION);
    CHECK(stamp == T);                                   // the published stamp is the instant the cloud is expressed at
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    CHECK(got.size() == want.size() && std::memcmp(got.data(), want.data(), want.size() * 16) == 0);   // one point per voxel
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
