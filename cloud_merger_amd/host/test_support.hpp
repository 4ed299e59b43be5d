// test_support.hpp — what the stand-alone test programs of the host shell share: the failure count and CHECK, a config
// text loaded through a file, the one-sensor node most of them run, its input message, and main()'s body.
//   <name>_tests <tmpdir> [gpu]
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "merger_node.hpp"

namespace cloudmerge {

inline int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++cloudmerge::failures; } } while (0)

inline bool load_text(const std::string& path, const std::string& text, NodeConfig* c, std::string* err) {
    std::ofstream(path) << text;
    return load_config(path, c, err);
}

// One required sensor "a", no crop, every voxel kept, 16-byte records out. Its transform is the test's to set.
inline NodeConfig single_sensor_config(float leaf, uint64_t max_points) {
    NodeConfig c = reference_config();
    c.sensors = {{"a", "/a", "a_link", true}};
    c.params.crop_enable = 0;
    c.params.min_points_per_voxel = 0;
    c.params.leaf[0] = c.params.leaf[1] = c.params.leaf[2] = leaf;
    c.publish_pcl_layout = false;
    c.max_points_total = max_points;
    return c;
}

// x, y, z, intensity per point, as an xyzi16 message.
inline PointCloud2 xyzi_message(const std::vector<float>& pts) {
    PointCloud2 m = make_xyzi16_message(static_cast<int>(pts.size() / 4));
    std::memcpy(m.data.data(), pts.data(), pts.size() * 4);
    return m;
}

// ray_tests' scene on the 6 x 4 grid (cell 0.5, origin (-1, -1)), in the frame of a sensor at (-0.75, -0.75), cell (0, 0): a pole
// of 5 points in cell (4, 0), one of 3 points in cell (2, 0) on the way to it, a lone point in cell (2, 1), one point outside.
inline std::vector<float> ray_scene() {
    std::vector<float> pts;
    for (int i = 0; i < 5; ++i) {
        const float p[4] = {2.0f, 0.0f, 0.25f * static_cast<float>(i), 1.0f};
        pts.insert(pts.end(), p, p + 4);
    }
    for (int i = 0; i < 3; ++i) {
        const float p[4] = {1.0f, 0.0f, 0.5f * static_cast<float>(i), 2.0f};
        pts.insert(pts.end(), p, p + 4);
    }
    const float lone[4] = {1.0f, 0.5f, 0.1f, 3.0f}, outside[4] = {3.0f, 0.0f, 0.5f, 4.0f};
    pts.insert(pts.end(), lone, lone + 4);
    pts.insert(pts.end(), outside, outside + 4);
    return pts;
}

// grid_tests' scene on the same grid, in the base frame. Cell (0, 0): a flat patch of 9 points 1 cm apart in height; cell (3, 2):
// a pole of 5 points 0.25 m apart; cell (5, 3): one point; one point outside the grid.
inline std::vector<float> grid_scene() {
    std::vector<float> pts;
    for (int i = 0; i < 9; ++i) {
        const float p[4] = {-0.9f + 0.04f * static_cast<float>(i), -0.8f, 0.01f * static_cast<float>(i), static_cast<float>(i)};
        pts.insert(pts.end(), p, p + 4);
    }
    for (int i = 0; i < 5; ++i) {
        const float p[4] = {0.75f, 0.25f, 0.25f * static_cast<float>(i), 10.0f + static_cast<float>(i)};
        pts.insert(pts.end(), p, p + 4);
    }
    const float lone[4] = {1.75f, 0.75f, 0.5f, 99.0f}, outside[4] = {2.0f, 0.0f, 0.5f, 1.0f};
    pts.insert(pts.end(), lone, lone + 4);
    pts.insert(pts.end(), outside, outside + 4);
    return pts;
}

// The corner x = 0, y = 0, z = 0 over [0, 4]^2 on a lattice of `step`, phase `ph`, moved by the rotation `rz` (radians about
// z through (2, 2, 2)) and the shift (sx, sy, sz). `ripple`: the amplitude by which each plane is rippled (a perfectly flat
// voxel has lambda_0 = 0 up to rounding, and the covariance table calls the ones that round below 0 invalid).
inline std::vector<float> corner(double step, double ph, double rz, double sx, double sy, double sz, double ripple = 0.0) {
    std::vector<float> pts;
    const double c = std::cos(rz), s = std::sin(rz);
    for (int axis = 0; axis < 3; ++axis)
        for (double u = ph; u < 4.0; u += step)
            for (double v = ph; v < 4.0; v += step) {
                double p[3];
                p[axis] = ripple * std::sin(13.7 * u + 7.1 * v + axis); p[(axis + 1) % 3] = u; p[(axis + 2) % 3] = v;
                const double x = p[0] - 2.0, y = p[1] - 2.0;
                const float q[4] = {static_cast<float>(c * x - s * y + 2.0 + sx), static_cast<float>(s * x + c * y + 2.0 + sy),
                                    static_cast<float>(p[2] + sz), 1.0f};
                pts.insert(pts.end(), q, q + 4);
            }
    return pts;
}

inline bool gpu_mode(int argc, char** argv) { return argc > 2 && std::strcmp(argv[2], "gpu") == 0; }

// main(): cpu_fn(tmpdir) always, gpu_fn() with "gpu"; the last line printed and the exit code are what the wrappers read.
template <class CpuFn, class GpuFn>
int run_tests(int argc, char** argv, CpuFn cpu_fn, GpuFn gpu_fn) {
    cpu_fn(argc > 1 ? argv[1] : "/tmp");
    if (gpu_mode(argc, argv)) gpu_fn();
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}

}  // namespace cloudmerge
