// ndt_tests.cpp — the host shell's frame-to-frame registration by NDT (align_method ndt): the NodeConfig key and the
// start-up refusal (CPU) and, with "gpu", one node that sees a three-plane corner twice, the second time moved by a known
// rigid motion, and reports that motion.
//   ndt_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/ndt.cfg";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.align_prev && ref.align_method == "icp");                    // off, and ICP, by default
    const std::string head = "sensor a /a a_link required\n";
    CHECK(load_text(path, head + "align_prev 1\nalign_method ndt\nalign_max_iterations 40\n", &c, &err));
    CHECK(c.align_prev && c.align_method == "ndt" && c.align_max_iterations == 40);
    CHECK(load_text(path, head + "align_method icp   # the default, spelled out\n", &c, &err) && c.align_method == "icp" && !c.align_prev);
    CHECK(load_text(path, head + "align_method ndt\n", &c, &err) && c.align_method == "ndt" && !c.align_prev);
    // rejected: another name, no name
    CHECK(!load_text(path, head + "align_method gicp\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "align_method\n", &c, &err));
    CHECK(!load_text(path, head + "align_method NDT\n", &c, &err));
    // the node refuses ndt without the occupancy flag before it creates a context; with align_prev off the method is not used
    NodeConfig n = reference_config();
    n.sensors = {{"a", "/a", "a_link", true}};
    n.align_prev = true;
    n.align_method = "ndt";
    n.flags = 0;
    {
        CloudMergerNode node(n);
        CHECK(!node.ok() && node.error().find("CM_FLAG_OCCUPANCY") != std::string::npos);
    }
    n.align_method = "gicp";
    {
        CloudMergerNode node(n);
        CHECK(!node.ok() && node.error().find("align_method") != std::string::npos);
    }
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.5f, 40000);
    c.align_prev = true;
    c.align_method = "ndt";
    c.flags |= CM_FLAG_OCCUPANCY;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    node.set_publisher([](const std::string&, const PointCloud2&) {});
    const double rz = 0.03, sh[3] = {0.06, -0.04, 0.05};
    cm_result r{};
    for (int frame = 0; frame < 2; ++frame) {
        const std::vector<float> pts = frame == 0 ? corner(0.037, 0.011, 0.0, 0.0, 0.0, 0.0, 0.01) : corner(0.041, 0.017, rz, sh[0], sh[1], sh[2], 0.01);   // rippled by 1 cm
        PointCloud2 m = xyzi_message(pts);
        CHECK(node.on_cloud(0, m) == CM_OK);
        CHECK(node.spin_once(&r) == CM_OK);
        CHECK(r.n_out > 150 && r.n_out < 400);
        CHECK(node.has_alignment() == (frame == 1));
    }
    const cm_align_result& a = node.alignment();
    const cm_ndt_result& n = node.ndt_alignment();
    CHECK(n.flags == CM_NDT_CONVERGED && n.iterations >= 2 && n.iterations <= 30 && n.n_corr > 150 && n.score > 0);
    CHECK(n.gauss_d2 > 0 && n.gauss_d1 < 0);
    // alignment() carries the same outcome
    CHECK(a.flags == CM_ALIGN_CONVERGED && a.iterations == n.iterations && a.n_corr == n.n_corr && a.sse == 0 && a.rms == 0);
    CHECK(std::memcmp(a.pose, n.pose, sizeof a.pose) == 0 && std::memcmp(a.H, n.H, sizeof a.H) == 0 &&
          std::memcmp(a.pivot, n.pivot, sizeof a.pivot) == 0);
    // the pose maps the first cloud onto the second: the rotation about z through (2, 2, 2) and the shift
    const double cs = std::cos(rz), sn = std::sin(rz);
    const double want[12] = {cs, -sn, 0, 2.0 + sh[0] - (cs * 2.0 - sn * 2.0), sn, cs, 0, 2.0 + sh[1] - (sn * 2.0 + cs * 2.0), 0, 0, 1, sh[2]};
    // the source is the previous frame's few hundred centroids and the surfaces are rippled by 1 cm, which neither a centroid
    // nor a voxel's normal distribution models: twice that amplitude in translation, and that over the scene's 4 m in rotation
    for (int k = 0; k < 12; ++k) CHECK(std::fabs(a.pose[k] - want[k]) < ((k & 3) == 3 ? 0.02 : 0.005));
    // a frame without fresh clouds: nothing fused, the last outcome stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.has_alignment());
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
