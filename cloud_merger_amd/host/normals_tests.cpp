// normals_tests.cpp — the host shell's normal estimation: NodeConfig keys (CPU) and, with "gpu", one node whose voxel cloud
// is a tilted plane beside a short line, checked against the plane's known normal.
//   normals_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/normals.cfg";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.normals_k == 0 && ref.normals_viewpoint[0] == 0.0f && ref.normals_viewpoint[1] == 0.0f &&
          ref.normals_viewpoint[2] == 0.0f);                                                            // off by default
    CHECK(load_text(path, "sensor a /a a_link required\nnormals_k 12\nnormals_viewpoint 1.5 -2 0.25\n", &c, &err));
    CHECK(c.normals_k == 12 && c.normals_viewpoint[0] == 1.5f && c.normals_viewpoint[1] == -2.0f && c.normals_viewpoint[2] == 0.25f);
    CHECK(load_text(path, "sensor a /a a_link required\nnormals_k 3   # viewpoint left alone\n", &c, &err));
    CHECK(c.normals_k == 3 && c.normals_viewpoint[0] == 0.0f);
    CHECK(load_text(path, "sensor a /a a_link required\nnormals_k 64\n", &c, &err) && c.normals_k == CM_NORMAL_MAX_K);
    CHECK(load_text(path, "sensor a /a a_link required\nnormals_k 0\n", &c, &err) && c.normals_k == 0);
    // rejected: k of 1, 2 or above the maximum, a missing k, a viewpoint of two numbers or one that is not finite
    CHECK(!load_text(path, "sensor a /a a_link required\nnormals_k 2\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, "sensor a /a a_link required\nnormals_k 65\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\nnormals_k\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\nnormals_viewpoint 1 2\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\nnormals_viewpoint 1 2 inf\n", &c, &err));
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.normals_k = 9;
    c.normals_viewpoint[0] = 0.0f; c.normals_viewpoint[1] = 0.0f; c.normals_viewpoint[2] = 50.0f;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    // the plane z = x / 2 (exact in fp32 on this lattice), 20 x 20 points 0.5 apart, each its own voxel; and, 100 m away, a
    // line of 12 points along y
    std::vector<float> pts;
    for (int i = 0; i < 20; ++i)
        for (int j = 0; j < 20; ++j) { const float p[4] = {0.5f * i, 0.5f * j, 0.25f * i, 1.0f}; pts.insert(pts.end(), p, p + 4); }
    for (int j = 0; j < 12; ++j) { const float p[4] = {100.0f, 0.5f * j, 0.0f, 1.0f}; pts.insert(pts.end(), p, p + 4); }
    const int n = static_cast<int>(pts.size() / 4);
    PointCloud2 m = xyzi_message(pts);
    std::vector<float> out;
    node.set_publisher([&](const std::string&, const PointCloud2& o) {
        out.resize(o.num_points() * 4);
        std::memcpy(out.data(), o.data.data(), out.size() * 4);
    });
    CHECK(node.on_cloud(0, m) == CM_OK);
    cm_result r{};
    CHECK(node.spin_once(&r) == CM_OK);
    CHECK(r.n_out == static_cast<uint64_t>(n));
    const std::vector<cm_voxel_normal>& nr = node.normals();
    CHECK(nr.size() == out.size() / 4 && nr.size() == static_cast<size_t>(n));
    // the plane's normal towards z = +50: (-1, 0, 2) / sqrt(5)
    const double want[3] = {-1.0 / std::sqrt(5.0), 0.0, 2.0 / std::sqrt(5.0)};
    int on_plane = 0, on_line = 0;
    for (size_t i = 0; i < nr.size() && i * 4 + 3 < out.size(); ++i) {
        const cm_voxel_normal& e = nr[i];
        CHECK(e.n_neighbors == 9 && e.flags == CM_NORMAL_VALID && e.last < nr.size() && e.last != i);
        if (out[4 * i] < 50.0f) {
            ++on_plane;
            for (int a = 0; a < 3; ++a) CHECK(std::fabs(e.normal[a] - want[a]) < 1e-6);
            CHECK(e.curvature < 1e-9f);
        } else {
            // a line: the two smallest eigenvalues are both 0 and the normal is any direction across it
            ++on_line;
            CHECK(std::fabs(e.normal[1]) < 1e-6 && e.curvature < 1e-9f);
        }
    }
    CHECK(on_plane == 400 && on_line == 12);
    // a frame without fresh clouds: nothing fused, the last frame's table stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.normals().size() == static_cast<size_t>(n));
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
