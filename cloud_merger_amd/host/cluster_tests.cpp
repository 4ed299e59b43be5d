// cluster_tests.cpp — the host shell's cluster extraction: NodeConfig keys (CPU) and, with "gpu", one node whose voxel
// cloud holds three separated groups of points and a loose one, checked against the known partition.
//   cluster_tests <tmpdir> [gpu]
#include <map>

#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/cluster.cfg";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.cluster_tolerance == 0.0f && ref.cluster_min_size == 1 && ref.cluster_max_size == 0xFFFFFFFFu);   // off by default
    CHECK(load_text(path, "sensor a /a a_link required\ncluster_tolerance 0.35\ncluster_min_size 10\ncluster_max_size 25000\n", &c, &err));
    CHECK(c.cluster_tolerance == 0.35f && c.cluster_min_size == 10 && c.cluster_max_size == 25000);
    CHECK(load_text(path, "sensor a /a a_link required\ncluster_tolerance 0.5   # sizes left alone\n", &c, &err));
    CHECK(c.cluster_tolerance == 0.5f && c.cluster_min_size == 1 && c.cluster_max_size == 0xFFFFFFFFu);
    CHECK(load_text(path, "sensor a /a a_link required\ncluster_tolerance 0\n", &c, &err) && c.cluster_tolerance == 0.0f);
    // rejected: a negative or missing tolerance, a size of 0
    CHECK(!load_text(path, "sensor a /a a_link required\ncluster_tolerance -1\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, "sensor a /a a_link required\ncluster_tolerance\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\ncluster_min_size 0\n", &c, &err));
    CHECK(!load_text(path, "sensor a /a a_link required\ncluster_max_size 0\n", &c, &err));
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.cluster_tolerance = 0.6f;
    c.cluster_min_size = 2;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    // three rows of points 0.5 apart (10, 20 and 30 of them), 5 m from each other, and one loose point: each its own voxel
    std::vector<float> pts;
    const int rows[3] = {10, 20, 30};
    for (int g = 0; g < 3; ++g)
        for (int i = 0; i < rows[g]; ++i) { const float p[4] = {0.5f * i, 5.0f * g, 0.25f, 1.0f}; pts.insert(pts.end(), p, p + 4); }
    const float loose[4] = {40.0f, 40.0f, 0.25f, 1.0f};
    pts.insert(pts.end(), loose, loose + 4);
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
    CHECK(node.cluster_count() == 3);
    const std::vector<uint32_t>& lab = node.cluster_labels();
    CHECK(lab.size() == out.size() / 4 && lab.size() == static_cast<size_t>(n));
    // every voxel of a row carries the row's label, rows numbered in the order of the published cloud; the loose one none
    std::map<int, uint32_t> of_row;
    std::map<uint32_t, int> sizes;
    uint32_t next = 0;
    for (size_t i = 0; i < lab.size() && i * 4 + 1 < out.size(); ++i) {
        const float y = out[4 * i + 1];
        if (y > 20.0f) { CHECK(lab[i] == CM_CLUSTER_NONE); continue; }
        const int g = static_cast<int>(y / 5.0f + 0.5f);
        if (!of_row.count(g)) { CHECK(lab[i] == next); of_row[g] = lab[i]; ++next; }
        CHECK(lab[i] == of_row[g]);
        ++sizes[lab[i]];
    }
    CHECK(of_row.size() == 3);
    for (int g = 0; g < 3; ++g) CHECK(sizes[of_row[g]] == rows[g]);
    // a frame without fresh clouds: nothing fused, the last frame's clusters stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.cluster_count() == 3);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
