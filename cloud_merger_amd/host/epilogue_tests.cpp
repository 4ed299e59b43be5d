// epilogue_tests.cpp — the node's three publish modes (blocking, pipelined_publish, pipelined_publish + deferred_wait) with
// every by-product switched on: with "gpu", the same stream of clouds through each mode must publish the same messages and
// leave the same by-product tables behind every frame, byte for byte. There is nothing to check without a GPU.
//   epilogue_tests <tmpdir> [gpu]
#include "test_support.hpp"

using namespace cloudmerge;

// The node's tables after the call that waited for a frame.
struct Tables {
    uint64_t n_clusters = 0;
    std::vector<uint32_t> labels;
    std::vector<cm_cluster_box> boxes;
    std::vector<cm_grid_cell> cells;
    std::vector<int8_t> occupancy;
    std::vector<cm_grid_ray_cell> ray_cells;
    std::vector<int8_t> cleared;
    std::vector<cm_voxel_normal> normals;
    bool has_alignment = false;
    cm_align_result alignment{};

    explicit Tables(const CloudMergerNode& n)
        : n_clusters(n.cluster_count()), labels(n.cluster_labels()), boxes(n.cluster_boxes()), cells(n.grid_cells()),
          occupancy(n.grid_occupancy()), ray_cells(n.grid_ray_cells()), cleared(n.grid_cleared()), normals(n.normals()),
          has_alignment(n.has_alignment()) {
        if (has_alignment) alignment = n.alignment();
    }
};

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Run {
    std::vector<PointCloud2> messages;
    std::vector<Tables> tables;         // one per frame, in frame order
    uint64_t frames_published = 0;
};

// The stream: calls 1 to 5 are spin_once, call 6 is flush(). Frames are fused in calls 1, 3, 4 and 5; `waited_in` names the
// call that waits for each of them (deferred_wait: the next fusing call, or flush()).
static Run run_mode(bool pipelined, bool deferred, const int waited_in[4]) {
    Run run;
    NodeConfig c = single_sensor_config(0.125f, 1000);
    c.pipelined_publish = pipelined;
    c.deferred_wait = deferred;
    c.stamp_from_inputs = true;
    c.cluster_tolerance = 0.3f;
    c.cluster_box_angles = 8;
    c.grid_cell = 0.5f;                                     // the 6 x 4 grid of grid_tests, with rays
    c.grid_origin[0] = c.grid_origin[1] = -1.0f;
    c.grid_nx = 6;
    c.grid_ny = 4;
    c.grid_min_points = 2;
    c.grid_raycast = true;
    c.normals_k = 3;
    c.align_prev = true;
    CloudMergerNode node(c);
    CHECK(node.ok());
    if (!node.ok()) { std::printf("  %s\n", node.error().c_str()); return run; }
    const double q[4] = {0, 0, 0, 1}, t[3] = {-0.75, -0.75, 0};   // ray_tests' sensor, in cell (0, 0)
    node.set_transform(0, q, t);
    node.set_clock([] { return uint64_t{77}; });
    node.set_publisher([&](const std::string&, const PointCloud2& m) { run.messages.push_back(m); });

    // (grid_tests' scene is seen by the same sensor here, so it lies 0.75 lower on x and y than in grid_tests)
    const std::vector<float> rays = ray_scene(), grid = grid_scene(), nans(16, NAN);
    const std::vector<float>* cloud_of_call[5] = {&rays, nullptr, &grid, &nans, &rays};
    const uint64_t stamp_of_call[5] = {1000, 0, 2000, 3000, 4000};
    for (int call = 1; call <= 6; ++call) {
        if (call <= 5) {
            const std::vector<float>* pts = cloud_of_call[call - 1];
            if (pts) {
                PointCloud2 m = xyzi_message(*pts);
                m.header.stamp_ns = stamp_of_call[call - 1];
                CHECK(node.on_cloud(0, m) == CM_OK);
            }
            const int st = node.spin_once();
            CHECK(pts ? (st == CM_OK || st == CM_EMPTY_INPUT) : st == CM_NOT_READY);
        } else {
            node.flush();
        }
        for (int f = 0; f < 4; ++f)
            if (waited_in[f] == call) run.tables.emplace_back(node);
    }
    run.frames_published = node.frames_published();
    return run;
}

static void check_one_mode(const Run& r) {
    CHECK(r.frames_published == 4 && r.messages.size() == 4 && r.tables.size() == 4);
    if (r.messages.size() != 4 || r.tables.size() != 4) return;
    const uint64_t stamps[4] = {1000, 2000, 3000, 4000};
    for (uint32_t f = 0; f < 4; ++f) {
        const PointCloud2& m = r.messages[f];
        const Tables& t = r.tables[f];
        CHECK(m.header.seq == f && m.header.stamp_ns == stamps[f] && m.header.frame_id == "base_footprint" && m.point_step == 16);
        if (f == 2) {                                           // the frame of NaN points: no voxel grid, no by-products
            CHECK(m.width == 0 && m.height == 0 && m.row_step == 0 && m.data.empty());
            CHECK(t.n_clusters == 0 && t.labels.empty() && t.boxes.empty() && t.cells.empty() && t.occupancy.empty());
            CHECK(t.ray_cells.empty() && t.cleared.empty() && t.normals.empty());
            continue;
        }
        // (ray_tests' points are two voxels or more apart; grid_tests' flat patch shares voxels)
        CHECK(m.height == 1 && (f == 1 ? m.width >= 3 && m.width <= 16 : m.width == 10) && m.row_step == 16 * m.width && m.data.size() == m.row_step);
        CHECK(t.n_clusters >= 1 && t.labels.size() == m.width && t.boxes.size() == t.n_clusters);
        CHECK(t.cells.size() == 24 && t.occupancy.size() == 24 && t.ray_cells.size() == 24 && t.cleared.size() == 24);
        CHECK(t.normals.size() == m.width);
        for (const cm_voxel_normal& e : t.normals) CHECK(e.n_neighbors == 3);
    }
    // registered against the frame before: not the first frame, not a frame without a voxel grid, not the one after it
    CHECK(!r.tables[0].has_alignment && r.tables[1].has_alignment && !r.tables[2].has_alignment && !r.tables[3].has_alignment);
    uint64_t rays_crossing = 0;
    for (const cm_grid_ray_cell& g : r.tables[0].ray_cells) rays_crossing += g.n_pass;
    CHECK(rays_crossing == 8);                                  // ray_tests' three rays
}

static void check_modes_agree(const Run& a, const Run& b) {
    if (a.messages.size() != 4 || a.tables.size() != 4 || b.messages.size() != 4 || b.tables.size() != 4) return;
    for (int f = 0; f < 4; ++f) {
        const PointCloud2 &m = a.messages[f], &n = b.messages[f];
        CHECK(m.header.seq == n.header.seq && m.header.stamp_ns == n.header.stamp_ns && m.header.frame_id == n.header.frame_id);
        CHECK(m.point_step == n.point_step && m.width == n.width && m.height == n.height && m.row_step == n.row_step);
        CHECK(same_bytes(m.data, n.data));
        const Tables &s = a.tables[f], &t = b.tables[f];
        CHECK(s.n_clusters == t.n_clusters && same_bytes(s.labels, t.labels) && same_bytes(s.boxes, t.boxes));
        CHECK(same_bytes(s.cells, t.cells) && same_bytes(s.occupancy, t.occupancy));
        CHECK(same_bytes(s.ray_cells, t.ray_cells) && same_bytes(s.cleared, t.cleared));
        CHECK(same_bytes(s.normals, t.normals));
        CHECK(s.has_alignment == t.has_alignment && std::memcmp(&s.alignment, &t.alignment, sizeof s.alignment) == 0);
    }
}

static void test_modes_on_gpu() {
    const int same_call[4] = {1, 3, 4, 5}, next_fusing_call[4] = {2, 4, 5, 6};
    const Run blocking = run_mode(false, false, same_call);
    const Run pipelined = run_mode(true, false, same_call);
    const Run deferred = run_mode(true, true, next_fusing_call);
    check_one_mode(blocking);
    check_one_mode(pipelined);
    check_one_mode(deferred);
    check_modes_agree(blocking, pipelined);
    check_modes_agree(blocking, deferred);
}

int main(int argc, char** argv) { return run_tests(argc, argv, [](const char*) {}, test_modes_on_gpu); }
