// align_tests.cpp — the host shell's frame-to-frame registration: NodeConfig keys (CPU) and, with "gpu", one node that sees
// a three-plane corner twice, the second time moved by a known rigid motion, and reports that motion.
//   align_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

static void test_config_keys(const char* tmpdir) {
    const std::string path = std::string(tmpdir) + "/align.cfg";
    NodeConfig c;
    std::string err;
    const NodeConfig ref = reference_config();
    CHECK(!ref.align_prev && ref.align_max_corr == 0.5f && ref.align_normals_k == 10 && ref.align_max_iterations == 30);   // off by default
    const std::string head = "sensor a /a a_link required\n";
    CHECK(load_text(path, head + "align_prev 1\nalign_max_corr 0.25\nalign_normals_k 12\nalign_max_iterations 5\n", &c, &err));
    CHECK(c.align_prev && c.align_max_corr == 0.25f && c.align_normals_k == 12 && c.align_max_iterations == 5);
    CHECK(load_text(path, head + "align_prev 0   # the rest left alone\n", &c, &err) && !c.align_prev && c.align_normals_k == 10);
    CHECK(load_text(path, head + "align_max_iterations 0\nalign_normals_k 64\n", &c, &err));
    CHECK(c.align_max_iterations == 0 && c.align_normals_k == CM_NORMAL_MAX_K);
    CHECK(load_text(path, head + "align_max_iterations 64\nalign_normals_k 3\n", &c, &err) && c.align_max_iterations == CM_ALIGN_MAX_ITER);
    // rejected: a switch that is neither 0 nor 1, a radius that is not positive and finite, k or iterations out of range
    CHECK(!load_text(path, head + "align_prev 2\n", &c, &err));
    CHECK(err.find(":2:") != std::string::npos);
    CHECK(!load_text(path, head + "align_prev\n", &c, &err));
    CHECK(!load_text(path, head + "align_max_corr 0\n", &c, &err));
    CHECK(!load_text(path, head + "align_max_corr -1\n", &c, &err));
    CHECK(!load_text(path, head + "align_max_corr inf\n", &c, &err));
    CHECK(!load_text(path, head + "align_normals_k 2\n", &c, &err));
    CHECK(!load_text(path, head + "align_normals_k 65\n", &c, &err));
    CHECK(!load_text(path, head + "align_max_iterations 65\n", &c, &err));
}

static void test_node_on_gpu() {
    NodeConfig c = single_sensor_config(0.1f, 40000);
    c.align_prev = true;
    c.align_max_corr = 0.4f;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
    node.set_transform(0, q, t);
    node.set_publisher([](const std::string&, const PointCloud2&) {});
    const double rz = 0.03, sh[3] = {0.06, -0.04, 0.05};
    cm_result r{};
    for (int frame = 0; frame < 2; ++frame) {
        const std::vector<float> pts = frame == 0 ? corner(0.037, 0.011, 0.0, 0.0, 0.0, 0.0) : corner(0.041, 0.017, rz, sh[0], sh[1], sh[2]);
        PointCloud2 m = xyzi_message(pts);
        CHECK(node.on_cloud(0, m) == CM_OK);
        CHECK(node.spin_once(&r) == CM_OK);
        CHECK(r.n_out > 3000);
        CHECK(node.has_alignment() == (frame == 1));
    }
    const cm_align_result& a = node.alignment();
    CHECK(a.flags == CM_ALIGN_CONVERGED && a.iterations >= 2 && a.iterations <= 12 && a.n_corr > 3000 && a.rms < 0.02);
    // the pose maps the first cloud onto the second: the rotation about z through (2, 2, 2) and the shift
    const double cs = std::cos(rz), sn = std::sin(rz);
    const double want[12] = {cs, -sn, 0, 2.0 + sh[0] - (cs * 2.0 - sn * 2.0), sn, cs, 0, 2.0 + sh[1] - (sn * 2.0 + cs * 2.0), 0, 0, 1, sh[2]};
    for (int k = 0; k < 12; ++k) CHECK(std::fabs(a.pose[k] - want[k]) < ((k & 3) == 3 ? 0.01 : 0.003));
    // a frame without fresh clouds: nothing fused, the last outcome stays
    CHECK(node.spin_once(&r) == CM_NOT_READY);
    CHECK(node.has_alignment());
}

int main(int argc, char** argv) { return run_tests(argc, argv, test_config_keys, test_node_on_gpu); }
