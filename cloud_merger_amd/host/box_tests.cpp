// box_tests.cpp — the host shell's oriented boxes: NodeConfig keys (CPU) and, with "gpu", one node whose voxel cloud holds
// three lattice rectangles at known headings and a loose point, checked against the known boxes.
//   box_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/box.cfg";
    const std::string head = "sensor a /a a_link required\ncluster_tolerance 0.5\n";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(ref.cluster_box_angles == 0 && ref.cluster_box_criterion == CM_BOX_CLOSENESS && ref.cluster_box_d_min == 0.01f);   // off by default
    CHECK(load_text(path, head + "cluster_box_angles 90\ncluster_box_criterion area\ncluster_box_d_min 0.05\n", &c, &err));
    CHECK(c.cluster_box_angles == 90 && c.cluster_box_criterion == CM_BOX_AREA && c.cluster_box_d_min == 0.05f);
    CHECK(load_text(path, head + "cluster_box_angles 180   # the rest left alone\n", &c, &err));
    CHECK(c.cluster_box_angles == 180 && c.cluster_box_criterion == CM_BOX_CLOSENESS && c.cluster_box_d_min == 0.01f);
    CHECK(load_text(path, head + "cluster_box_criterion closeness\ncluster_box_angles 0\n", &c, &err) && c.cluster_box_angles == 0);
    // rejected: more headings than the library takes, an unknown criterion, a d_min that is not > 0, missing values
    CHECK(!load_text(path, head + "cluster_box_angles 181\n", &c, &err));
    CHECK(err.find(":3:") != std::string::npos);
    CHECK(!load_text(path, head + "cluster_box_angles\n", &c, &err));
    CHECK(!load_text(path, head + "cluster_box_criterion perimeter\n", &c, &err));
    CHECK(!load_text(path, head + "cluster_box_criterion\n", &c, &err));
    CHECK(!load_text(path, head + "cluster_box_d_min 0\n", &c, &err));
    CHECK(!load_text(path, head + "cluster_box_d_min -0.01\n", &c, &err));
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.cluster_tolerance = 0.6f;
    c.cluster_min_size = 2;
    c.cluster_box_angles = 90;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    // three lattices of 9 x 4 points 0.5 apart, turned by 0, 30 and 60 degrees about their first point, 20 m from each other,
    // and one loose point: each point its own voxel (the smallest gap between two of a lattice is 0.5 m, four voxels)
    const int nx = 9, ny = 4;
    const double deg[3] = {0.0, 30.0, 60.0};
    std::vector<float> pts;
    for (int g = 0; g < 3; ++g) {
        const double th = deg[g] * 3.14159265358979323846 / 180.0, cs = std::cos(th), sn = std::sin(th);
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j) {
                const double x = 0.5 * i, y = 0.5 * j;
                const float p[4] = {static_cast<float>(5.0 + 20.0 * g + x * cs - y * sn), static_cast<float>(5.0 + x * sn + y * cs), 0.25f, 1.0f};
                pts.insert(pts.end(), p, p + 4);
            }
    }
    const float loose[4] = {40.0f, 40.0f, 0.25f, 1.0f};
    pts.insert(pts.end(), loose, loose + 4);
    const int n = static_cast<int>(pts.size() / 4);
    PointCloud2 m = xyzi_message(pts);
    CHECK(node.on_cloud(0, m) == CM_OK);
    cm_result r{};
    CHECK(node.spin_once(&r) == CM_OK);
    CHECK(r.n_out == static_cast<uint64_t>(n));
    CHECK(node.cluster_count() == 3);
    const std::vector<cm_cluster_box>& boxes = node.cluster_boxes();
    CHECK(boxes.size() == 3);
    // each lattice's box: 4 x 1.5 m at its heading (on a lattice every member of the rim is at distance 0 there), found
    // whichever number its cluster got
    bool seen[3] = {false, false, false};
    for (const cm_cluster_box& b : boxes) {
        CHECK(b.flags == CM_BOX_VALID);
        const int g = static_cast<int>(b.center[0] / 20.0f);
        CHECK(g >= 0 && g < 3);
        if (g < 0 || g > 2) continue;
        seen[g] = true;
        CHECK(b.angle == static_cast<uint32_t>(deg[g]));
        CHECK(std::fabs(b.yaw - static_cast<float>(deg[g] * 3.14159265358979323846 / 180.0)) < 1e-6f);
        CHECK(std::fabs(b.size[0] - 4.0f) < 1e-4f && std::fabs(b.size[1] - 1.5f) < 1e-4f && b.size[2] == 0.0f);
        const double th = deg[g] * 3.14159265358979323846 / 180.0;
        const double cx = 5.0 + 20.0 * g + 2.0 * std::cos(th) - 0.75 * std::sin(th), cy = 5.0 + 2.0 * std::sin(th) + 0.75 * std::cos(th);
        CHECK(std::fabs(b.center[0] - cx) < 1e-4 && std::fabs(b.center[1] - cy) < 1e-4 && b.center[2] == 0.25f);
        CHECK(b.score > 0.0);
    }
    CHECK(seen[0] && seen[1] && seen[2]);
    // a frame without fresh clouds: nothing fused, the last frame's boxes stay
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.cluster_boxes().size() == 3);
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
