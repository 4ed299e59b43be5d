// merger_node.cpp — see merger_node.hpp.
#include "merger_node.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <fstream>
#include <sstream>
#include <thread>

namespace cloudmerge {

bool traj_footprint_lattice(float x_back, float x_front, float half_width, float cell, std::vector<float>* xy) {
    const double h = 0.5 * static_cast<double>(cell), len = static_cast<double>(x_front) - x_back, wid = 2.0 * static_cast<double>(half_width);
    uint64_t n_x = static_cast<uint64_t>(std::ceil(len / h)) + 1u, n_y = static_cast<uint64_t>(std::ceil(wid / h)) + 1u;
    const bool coarsened = n_x * n_y > CM_TRAJ_MAX_FOOT;
    if (coarsened) {
        const double scale = std::sqrt(static_cast<double>(CM_TRAJ_MAX_FOOT) / (static_cast<double>(n_x) * static_cast<double>(n_y)));
        n_x = std::max<uint64_t>(1u, static_cast<uint64_t>(static_cast<double>(n_x) * scale));
        n_y = std::max<uint64_t>(1u, static_cast<uint64_t>(static_cast<double>(n_y) * scale));
        n_x = std::min<uint64_t>(n_x, CM_TRAJ_MAX_FOOT);               // (one of the two was raised to 1: a strip)
        n_y = std::min<uint64_t>(n_y, CM_TRAJ_MAX_FOOT / n_x);
    }
    xy->clear();
    for (uint64_t i = 0; i < n_x; ++i)
        for (uint64_t j = 0; j < n_y; ++j) {
            xy->push_back(static_cast<float>(n_x == 1u ? x_back + 0.5 * len : x_back + len * static_cast<double>(i) / static_cast<double>(n_x - 1u)));
            xy->push_back(static_cast<float>(n_y == 1u ? 0.0 : -static_cast<double>(half_width) + wid * static_cast<double>(j) / static_cast<double>(n_y - 1u)));
        }
    return coarsened;
}

NodeConfig reference_config() {
    NodeConfig c;
    // Topics :520-525, TF frames :556-561, fuse order :137-142, gate :134-136.
    c.sensors = {
        {"front_right", "/velodyne/front_right/velodyne_points", "/velodyne_front_right", true},
        {"front_left", "/velodyne/front_left/velodyne_points", "/velodyne_front_left", true},
        {"rear_right", "/velodyne/rear_right/velodyne_points", "/velodyne_rear_right", true},
        {"rear_left", "/velodyne/rear_left/velodyne_points", "/velodyne_rear_left", true},
        {"top_middle", "/velodyne/top_middle/velodyne_points", "/velodyne_top_middle", false},
        {"front_middle", "/livoxfront/livox/lidar", "/livox_front", true},
    };
    cm_params& p = c.params;
    p.leaf[0] = p.leaf[1] = p.leaf[2] = 0.1f;       // voxel_size, Parameter.h:28
    p.min_points_per_voxel = 2;                     // points_per_voxel, Parameter.h:27
    p.downsample_all_data = 1;                      // :174
    p.crop_enable = 1;                              // getROI, :20-40
    const float roi_width = 10.0f, roi_length = 75.0f, roi_mid = 15.0f;   // Parameter.h:31-33
    p.crop_min[0] = -roi_mid;        p.crop_max[0] = roi_length - roi_mid;
    p.crop_min[1] = -roi_width / 2;  p.crop_max[1] = roi_width / 2;
    p.crop_min[2] = -0.5f;           p.crop_max[2] = 3.0f;                 // Parameter.h:34-35
    // Radius outlier removal is off here: the live node applies it per ground-removal zone
    // (:119, out of scope). fusion_config() below is the class-based node's chain, which runs it
    // on the fused cloud.
    return c;
}

NodeConfig live_node_config() {
    NodeConfig c = reference_config();
    c.ground_enable = true;
    cm_ground_params& g = c.ground;
    g.max_iterations = 1000;                       // Parameter.h:38
    g.distance_threshold = 0.3f;                   // :40
    g.probability = 0.99f;                         // :41
    g.optimize_coefficients = 1;                   // :95
    g.z_keep_max = 3.0f;                           // roi_z_max, :35
    g.outlier_radius = 0.15f;                      // removeGround's outlierRemoval(no_ground_cloud_ptr), :119 — radius_search, Parameter.h:23
    g.outlier_min_neighbors = 1;                   // min_neighbor, Parameter.h:24
    g.seed = 12345;
    const float roi_mid = 15.0f;
    // proceedFront (:228-269), in its processing order: front, mid2, mid, vehicle, rear (Parameter.h:45-55)
    const float vf_front = 30.0f, vf_mid = 15.0f, vf_mid2 = 11.0f, vf_veh = 8.0f, vf_rear = 11.0f;
    const cm_zone front[5] = {
        {-roi_mid + vf_rear + vf_veh + vf_mid + vf_mid2, vf_front, 2.5f},
        {-roi_mid + vf_rear + vf_veh + vf_mid, vf_mid2, 2.0f},
        {-roi_mid + vf_rear + vf_veh, vf_mid, 1.5f},
        {-roi_mid + vf_rear, vf_veh, 0.3f},
        {-roi_mid, vf_rear, 0.5f}};
    for (int s = 0; s < 4; ++s) {                  // all four corner Velodynes go through proceedFront (:326,:352,:378,:404)
        g.n_zones[s] = 5;
        for (int z = 0; z < 5; ++z) g.zones[s][z] = front[z];
    }
    // top middle (:436-444): one slab with a plane, the part behind it kept whole (Parameter.h:66-68)
    g.n_zones[4] = 2;
    g.zones[4][0] = {20.0f, 40.0f, 1.0f};
    g.zones[4][1] = {-roi_mid, roi_mid + 20.0f, -1.0f};
    // Livox (:475-497): front, mid2, mid, rear (Parameter.h:71-80)
    const float l_front = 26.0f, l_mid = 10.0f, l_mid2 = 10.0f, l_rear = 10.0f, l_dev = 4.0f;
    g.n_zones[5] = 4;
    g.zones[5][0] = {l_dev + l_rear + l_mid + l_mid2, l_front, 1.5f};
    g.zones[5][1] = {l_dev + l_rear + l_mid, l_mid2, 1.2f};
    g.zones[5][2] = {l_dev + l_rear, l_mid, 0.8f};
    g.zones[5][3] = {l_dev, l_rear, 0.5f};
    return c;
}

NodeConfig fusion_config() {
    // my_cloud_fusion/src/cloud_fusion_node.cpp:72-75: remove_outliers, then voxelgrid, on the
    // fused cloud; constants from my_cloud_fusion/src/Parameter.h:15-16,109-110.
    NodeConfig c = reference_config();
    c.voxel_topic = "/cloud_fusion_node/points_voxel";
    c.params.outlier_enable = 1;
    c.params.outlier_radius = 0.1f;
    c.params.outlier_min_neighbors = 1;
    return c;
}

namespace {

// load_config's line helpers. read: whether every value was extracted (what follows them on the line is ignored).
template <class... T>
bool read(std::istream& is, T&... v) { return static_cast<bool>((is >> ... >> v)); }

bool read_flag(std::istream& is, bool* flag) {                          // the strict 0|1 keys
    int v = 0;
    if (!read(is, v) || (v != 0 && v != 1)) return false;
    *flag = v == 1;
    return true;
}

// the sensor of that name (the last one, should several carry it); c.sensors.size(): none
size_t sensor_index(const NodeConfig& c, const std::string& name) {
    size_t idx = c.sensors.size();
    for (size_t q = 0; q < c.sensors.size(); ++q) if (c.sensors[q].name == name) idx = q;
    return idx;
}

// CM_NODE_TRACE (a debugging aid): which of two calls of a slow tick took the time, written when the timer goes out of scope.
struct SlowTick {
    const char *first, *second;
    double ms[2] = {0, 0};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(int k) { const auto t1 = std::chrono::steady_clock::now(); ms[k] = std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1; }
    ~SlowTick() {
        static const bool trace = std::getenv("CM_NODE_TRACE") != nullptr;
        if (trace && (ms[0] > 3 || ms[1] > 3)) std::fprintf(stderr, "[node] slow tick: %s %.2f %s %.2f ms\n", first, ms[0], second, ms[1]);
    }
};

}  // namespace

bool load_config(const std::string& path, NodeConfig* cfg, std::string* err) {
    std::ifstream f(path);
    if (!f) { if (err) *err = "cannot open " + path; return false; }
    NodeConfig c = reference_config();
    cm_params& p = c.params;
    bool own_sensors = false, ground_z_from_crop = false;
    int lineno = 0;
    for (std::string line; std::getline(f, line);) {
        ++lineno;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        std::istringstream is(line);
        std::string key;
        if (!(is >> key)) continue;
        bool ok = true;
        if (key == "sensor") {
            SensorSpec s;
            std::string req;
            ok = read(is, s.name, s.topic, s.frame, req) && (req == "required" || req == "optional");
            s.required = req == "required";
            if (ok) { if (!own_sensors) { c.sensors.clear(); own_sensors = true; } c.sensors.push_back(s); }
        } else if (key == "base_frame") ok = read(is, c.base_frame);
        else if (key == "voxel_topic") ok = read(is, c.voxel_topic);
        else if (key == "rate_hz") ok = read(is, c.rate_hz) && c.rate_hz > 0;
        else if (key == "leaf") { float v = 0; ok = read(is, v) && v > 0; if (ok) p.leaf[0] = p.leaf[1] = p.leaf[2] = v; }
        else if (key == "min_points_per_voxel") ok = read(is, p.min_points_per_voxel);
        else if (key == "crop") {
            ok = read(is, p.crop_min[0], p.crop_min[1], p.crop_min[2], p.crop_max[0], p.crop_max[1], p.crop_max[2]);
            p.crop_enable = 1;
        } else if (key == "no_crop") p.crop_enable = 0;
        else if (key == "outlier") { ok = read(is, p.outlier_radius, p.outlier_min_neighbors); p.outlier_enable = 1; }
        else if (key == "stamp_from_inputs") { int v = 0; ok = read(is, v); c.stamp_from_inputs = v != 0; }   // (any integer: not read_flag)
        else if (key == "max_stamp_spread_ms") { double v = 0; ok = read(is, v) && v >= 0; if (ok) c.max_stamp_spread_ns = static_cast<uint64_t>(v * 1e6); }
        else if (key == "ground") {
            ok = read(is, c.ground.max_iterations, c.ground.distance_threshold, c.ground.probability);
            c.ground.optimize_coefficients = 1; c.ground.seed = 12345;
            ground_z_from_crop = true;                 // roi_z_max: taken from the crop box once the whole file is read
            c.ground_enable = true;
        } else if (key == "ground_outlier") ok = read(is, c.ground.outlier_radius, c.ground.outlier_min_neighbors) && c.ground.outlier_radius >= 0.0f;
        else if (key == "zone") {
            std::string name; cm_zone z{};
            ok = read(is, name, z.x_min, z.x_length, z.z_max_ground);
            const size_t sidx = sensor_index(c, name);
            ok = ok && sidx < c.sensors.size() && c.ground.n_zones[sidx] < CM_MAX_ZONES;
            if (ok) c.ground.zones[sidx][c.ground.n_zones[sidx]++] = z;
        } else if (key == "statistical_outlier") {
            cm_sor_params q{};
            ok = read(is, q.mean_k, q.std_mul) && q.mean_k >= 1 && q.mean_k <= CM_SOR_MAX_K;
            float cell = 0.0f;
            if (ok && read(is, cell)) q.search_cell = cell;                 // (optional: a third token that is no number is ignored)
            ok = ok && q.search_cell >= 0.0f;
            if (ok) { c.sor = q; c.sor_enable = true; }
        }
        else if (key == "cluster_tolerance") ok = read(is, c.cluster_tolerance) && c.cluster_tolerance >= 0.0f && std::isfinite(c.cluster_tolerance);
        else if (key == "cluster_min_size") ok = read(is, c.cluster_min_size) && c.cluster_min_size >= 1;
        else if (key == "cluster_max_size") ok = read(is, c.cluster_max_size) && c.cluster_max_size >= 1;
        else if (key == "cluster_box_angles") ok = read(is, c.cluster_box_angles) && c.cluster_box_angles <= CM_BOX_MAX_ANGLES;
        else if (key == "cluster_box_criterion") {
            std::string v;
            ok = read(is, v) && (v == "area" || v == "closeness");
            c.cluster_box_criterion = v == "area" ? CM_BOX_AREA : CM_BOX_CLOSENESS;
        }
        else if (key == "cluster_box_d_min") ok = read(is, c.cluster_box_d_min) && c.cluster_box_d_min > 0.0f && std::isfinite(c.cluster_box_d_min);
        else if (key == "grid_cell") ok = read(is, c.grid_cell) && std::isfinite(c.grid_cell) && c.grid_cell >= 0.0f &&
                                          (c.grid_cell == 0.0f || std::isfinite(1.0f / c.grid_cell));
        else if (key == "grid_origin") ok = read(is, c.grid_origin[0], c.grid_origin[1]) && std::isfinite(c.grid_origin[0]) && std::isfinite(c.grid_origin[1]);
        else if (key == "grid_size") ok = read(is, c.grid_nx, c.grid_ny) && c.grid_nx >= 1 && c.grid_ny >= 1 &&
                                          static_cast<uint64_t>(c.grid_nx) * c.grid_ny <= CM_GRID_MAX_CELLS;
        else if (key == "grid_z_band") ok = read(is, c.grid_z_band[0], c.grid_z_band[1]) && c.grid_z_band[0] <= c.grid_z_band[1];
        else if (key == "grid_obstacle_height") ok = read(is, c.grid_obstacle_height) && std::isfinite(c.grid_obstacle_height) && c.grid_obstacle_height >= 0.0f;
        else if (key == "grid_min_points") ok = read(is, c.grid_min_points) && c.grid_min_points >= 1;
        else if (key == "grid_raycast") ok = read_flag(is, &c.grid_raycast);
        else if (key == "grid_min_pass") ok = read(is, c.grid_min_pass) && c.grid_min_pass >= 1;
        else if (key == "grid_ray_range") ok = read(is, c.grid_ray_range);
        else if (key == "map_cell") ok = read(is, c.map_cell) && std::isfinite(c.map_cell) && c.map_cell >= 0.0f &&
                                         (c.map_cell == 0.0f || std::isfinite(1.0f / c.map_cell));
        else if (key == "map_size") ok = read(is, c.map_nx, c.map_ny) && c.map_nx >= 1 && c.map_ny >= 1 &&
                                         static_cast<uint64_t>(c.map_nx) * c.map_ny <= CM_GRID_MAX_CELLS;
        else if (key == "map_z_band") ok = read(is, c.map_z_band[0], c.map_z_band[1]) && c.map_z_band[0] <= c.map_z_band[1];
        else if (key == "map_logodds") ok = read(is, c.map_l_hit, c.map_l_miss, c.map_l_min, c.map_l_max) && c.map_l_hit >= 1 && c.map_l_miss >= 1 &&
                                            c.map_l_min <= 0 && c.map_l_max >= 0;
        else if (key == "map_thresholds") ok = read(is, c.map_l_free, c.map_l_occ) && c.map_l_free < c.map_l_occ;
        else if (key == "map_ray_range") ok = read(is, c.map_ray_range);
        else if (key == "map_inflation") ok = read(is, c.map_inscribed_radius, c.map_inflation_radius, c.map_cost_scaling) &&
                                              std::isfinite(c.map_inscribed_radius) && c.map_inscribed_radius >= 0.0f &&
                                              std::isfinite(c.map_inflation_radius) && std::isfinite(c.map_cost_scaling) && c.map_cost_scaling >= 0.0f &&
                                              (c.map_inflation_radius == 0.0f || c.map_inflation_radius >= c.map_inscribed_radius);
        else if (key == "map_inflate_unknown") ok = read_flag(is, &c.map_inflate_unknown);
        else if (key == "map_plan") ok = read(is, c.map_plan_neutral, c.map_plan_factor_q8) && c.map_plan_neutral <= 255u && c.map_plan_factor_q8 <= 256u;
        else if (key == "map_plan_allow_unknown") ok = read_flag(is, &c.map_plan_allow_unknown);
        else if (key == "map_frontier") ok = read(is, c.map_frontier_min_cells, c.map_frontier_max) && c.map_frontier_max >= 1u && c.map_frontier_max <= CM_FRONTIER_MAX_TABLE;
        else if (key == "map_frontier_max_cost") ok = read(is, c.map_frontier_max_cost) && c.map_frontier_max_cost <= 252u;
        else if (key == "map_frontier_scales") ok = read(is, c.map_frontier_pot_scale, c.map_frontier_gain_scale);
        else if (key == "map_goal_vehicle") ok = read_flag(is, &c.map_goal_vehicle);
        else if (key == "map_goal") { ok = read(is, c.map_goal[0], c.map_goal[1]) && std::isfinite(c.map_goal[0]) && std::isfinite(c.map_goal[1]); c.map_has_goal = ok; }
        else if (key == "traj") ok = read(is, c.traj_nv, c.traj_nw, c.traj_steps, c.traj_dt) &&
                                     (c.traj_nv == 0u || (c.traj_nw >= 1u && static_cast<uint64_t>(c.traj_nv) * c.traj_nw <= CM_TRAJ_MAX_SAMPLES &&
                                                          c.traj_steps >= 1u && c.traj_steps <= CM_TRAJ_MAX_STEPS && std::isfinite(c.traj_dt) && c.traj_dt > 0.0f));
        else if (key == "traj_limits") {
            float* l = c.traj_limits;
            ok = read(is, l[0], l[1], l[2], l[3]) && std::isfinite(l[0]) && std::isfinite(l[1]) && std::isfinite(l[2]) && std::isfinite(l[3]) &&
                 l[0] <= l[1] && l[2] <= l[3];
        }
        else if (key == "traj_footprint") {
            float* f = c.traj_footprint;
            ok = read(is, f[0], f[1], f[2]) && std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && f[0] <= f[1] && f[2] >= 0.0f;
        }
        else if (key == "traj_scales") ok = read(is, c.traj_occ_scale, c.traj_goal_scale);
        else if (key == "traj_allow_unknown") ok = read_flag(is, &c.traj_allow_unknown);
        else if (key == "match") ok = read_flag(is, &c.match_enable);
        else if (key == "match_angles") ok = read(is, c.match_n_a, c.match_a_stride) && c.match_n_a <= CM_MATCH_MAX_ANGLES && c.match_a_stride >= 1u &&
                                             static_cast<uint64_t>(c.match_n_a) * c.match_a_stride <= 1024u;
        else if (key == "match_window") ok = read(is, c.match_wx, c.match_wy) && c.match_wx <= CM_MATCH_MAX_SHIFT && c.match_wy <= CM_MATCH_MAX_SHIFT;
        else if (key == "match_field") ok = read(is, c.match_sigma, c.match_max_dist) && std::isfinite(c.match_sigma) && c.match_sigma > 0.0f &&
                                            std::isfinite(c.match_max_dist) && c.match_max_dist > 0.0f;
        else if (key == "match_subcell") ok = read_flag(is, &c.match_subcell);
        else if (key == "match_search") ok = read_flag(is, &c.match_search_enable);
        else if (key == "match_search_window") ok = read(is, c.match_search_wx, c.match_search_wy) && c.match_search_wx <= CM_MATCH_SEARCH_MAX_SHIFT &&
                                                    c.match_search_wy <= CM_MATCH_SEARCH_MAX_SHIFT;
        else if (key == "match_search_depth") ok = read(is, c.match_search_depth) && c.match_search_depth <= CM_MATCH_SEARCH_MAX_DEPTH;
        else if (key == "match_search_capacity") ok = read(is, c.match_search_max_nodes, c.match_search_max_cells) && c.match_search_max_nodes >= 1u &&
                                                      c.match_search_max_nodes <= CM_MATCH_SEARCH_MAX_NODES && c.match_search_max_cells >= 1u &&
                                                      c.match_search_max_cells <= CM_MATCH_SEARCH_MAX_NODES;
        else if (key == "mcl") ok = read_flag(is, &c.mcl_enable);
        else if (key == "mcl_particles") ok = read(is, c.mcl_particles) && c.mcl_particles >= 1u && c.mcl_particles <= CM_MCL_MAX_PARTICLES;
        else if (key == "mcl_beams") ok = read(is, c.mcl_max_beams, c.mcl_range_cells) && c.mcl_max_beams >= 1u && c.mcl_max_beams <= CM_MCL_MAX_BEAMS &&
                                          c.mcl_range_cells >= 1u && c.mcl_range_cells <= CM_MCL_MAX_RANGE_CELLS;
        else if (key == "mcl_field") ok = read(is, c.mcl_sigma, c.mcl_max_dist) && std::isfinite(c.mcl_sigma) && c.mcl_sigma > 0.0f &&
                                          std::isfinite(c.mcl_max_dist) && c.mcl_max_dist > 0.0f;
        else if (key == "mcl_tau") ok = read(is, c.mcl_tau) && std::isfinite(c.mcl_tau) && c.mcl_tau > 0.0f;
        else if (key == "mcl_resample") ok = read(is, c.mcl_resample_frac) && read_flag(is, &c.mcl_resample_always) && std::isfinite(c.mcl_resample_frac) &&
                                             c.mcl_resample_frac >= 0.0f && c.mcl_resample_frac <= 1.0f;
        else if (key == "mcl_seed") ok = read(is, c.mcl_seed);
        else if (key == "mcl_init") {
            std::string how;
            ok = read(is, how) && (how == "pose" || how == "uniform");
            if (ok && how == "pose") {
                float* sd = c.mcl_init_sd;
                ok = read(is, sd[0], sd[1], sd[2]);
                for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(sd[k]) && sd[k] >= 0.0f && sd[k] <= 1024.0f;
            }
            if (ok) c.mcl_init_uniform = how == "uniform";
        }
        else if (key == "mcl_noise") {
            float* sd = c.mcl_noise;
            ok = read(is, sd[0], sd[1], sd[2]);
            for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(sd[k]) && sd[k] >= 0.0f && sd[k] <= 1024.0f;
        }
        else if (key == "mcl_beam") ok = read_flag(is, &c.mcl_beam_enable);
        else if (key == "mcl_beam_model") ok = read(is, c.mcl_beam_sigma, c.mcl_beam_over_cells) && std::isfinite(c.mcl_beam_sigma) && c.mcl_beam_sigma > 0.0f &&
                                               c.mcl_beam_over_cells <= CM_MCL_BEAM_MAX_OVER;
        else if (key == "mcl_beam_mix") {
            float* z = c.mcl_beam_mix;
            ok = read(is, z[0], z[1], z[2]) && std::isfinite(z[0]) && std::isfinite(z[1]) && std::isfinite(z[2]) && z[0] > 0.0f && z[1] >= 0.0f && z[2] >= 0.0f &&
                 (static_cast<double>(z[0]) + static_cast<double>(z[1])) + static_cast<double>(z[2]) <= 1.0;
        }
        else if (key == "mcl_beam_plain") ok = read_flag(is, &c.mcl_beam_plain);
        else if (key == "mcl_hyp") ok = read_flag(is, &c.mcl_hyp_enable);
        else if (key == "mcl_hyp_bins") {
            float bin_m = 0.0f;
            ok = read(is, bin_m, c.mcl_hyp_heading_bits) && std::isfinite(bin_m) && bin_m >= 0.0625f && bin_m <= 1024.0f && c.mcl_hyp_heading_bits <= 8u;
            if (ok) c.mcl_hyp_bin_q = static_cast<uint32_t>(std::lrint(static_cast<double>(bin_m) * 1024.0));
        }
        else if (key == "mcl_hyp_max") ok = read(is, c.mcl_hyp_max) && c.mcl_hyp_max >= 1u && c.mcl_hyp_max <= CM_MCL_HYP_MAX;
        else if (key == "mcl_recovery") {
            float* al = c.mcl_recovery_alpha;
            ok = read(is, al[0], al[1], c.mcl_inject_max) && std::isfinite(al[0]) && std::isfinite(al[1]) && 0.0f <= al[0] && al[0] <= al[1] && al[1] <= 1.0f;
        }
        else if (key == "mcl_kld") ok = read(is, c.mcl_kld_err, c.mcl_kld_z) && std::isfinite(c.mcl_kld_err) && c.mcl_kld_err > 0.0f && c.mcl_kld_err <= 1.0f &&
                                        std::isfinite(c.mcl_kld_z) && c.mcl_kld_z > 0.0f;
        else if (key == "cast") ok = read_flag(is, &c.cast_enable);
        else if (key == "cast_bearings") ok = read(is, c.cast_bearings) && c.cast_bearings >= 1u && c.cast_bearings <= CM_CAST_MAX_BEARINGS;
        else if (key == "cast_range") ok = read(is, c.cast_range_cells) && c.cast_range_cells >= 1u && c.cast_range_cells <= CM_CAST_MAX_RANGE_CELLS;
        else if (key == "cast_plain") ok = read_flag(is, &c.cast_plain);
        else if (key == "normals_k") ok = read(is, c.normals_k) && (c.normals_k == 0 || (c.normals_k >= 3 && c.normals_k <= CM_NORMAL_MAX_K));
        else if (key == "normals_viewpoint") {
            float* v = c.normals_viewpoint;
            ok = read(is, v[0], v[1], v[2]) && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
        }
        else if (key == "align_prev") ok = read_flag(is, &c.align_prev);
        else if (key == "align_max_corr") ok = read(is, c.align_max_corr) && c.align_max_corr > 0.0f && std::isfinite(c.align_max_corr);
        else if (key == "align_normals_k") ok = read(is, c.align_normals_k) && c.align_normals_k >= 3 && c.align_normals_k <= CM_NORMAL_MAX_K;
        else if (key == "align_max_iterations") ok = read(is, c.align_max_iterations) && c.align_max_iterations <= CM_ALIGN_MAX_ITER;
        else if (key == "align_method") ok = read(is, c.align_method) && (c.align_method == "icp" || c.align_method == "ndt");
        else if (key == "motion_compensation") ok = read_flag(is, &c.motion_compensation);
        else if (key == "time_field") {
            std::string name, type;
            uint32_t off = 0;
            ok = read(is, name, off, type) && (type == "f32" || type == "u32ns");
            const size_t sidx = sensor_index(c, name);
            ok = ok && sidx < c.sensors.size();
            if (ok) c.time_field[sidx] = NodeConfig::TimeField{off, type == "f32" ? CM_TIME_F32_S : CM_TIME_U32_NS};
        }
        else if (key == "max_points_total") ok = read(is, c.max_points_total);
        else if (key == "device") ok = read(is, c.device);
        else ok = false;
        if (!ok) { if (err) *err = path + ":" + std::to_string(lineno) + ": bad line"; return false; }
    }
    if (c.sensors.empty() || c.sensors.size() > CM_MAX_SENSORS) { if (err) *err = "sensor count must be 1..16"; return false; }
    if (c.grid_raycast && !(c.grid_cell > 0.0f)) { if (err) *err = "grid_raycast needs grid_cell > 0"; return false; }
    if (c.match_enable && c.match_search_enable) { if (err) *err = "match and match_search exclude each other"; return false; }
    if (c.mcl_enable && !(c.map_cell > 0.0f && c.map_inflation_radius > 0.0f)) { if (err) *err = "mcl needs the cost layer (map and map_inflation)"; return false; }
    if (c.mcl_beam_enable && !c.mcl_enable) { if (err) *err = "mcl_beam needs the localisation layer (mcl 1)"; return false; }
    if (c.mcl_hyp_enable && !c.mcl_enable) { if (err) *err = "mcl_hyp needs the localisation layer (mcl 1)"; return false; }
    if (c.mcl_hyp_enable && c.mcl_inject_max > c.mcl_particles - 1u) { if (err) *err = "mcl_recovery: inject_max is above mcl_particles - 1"; return false; }
    if (c.cast_enable && !(c.map_cell > 0.0f && c.map_inflation_radius > 0.0f)) { if (err) *err = "cast needs the cost layer (map and map_inflation)"; return false; }
    if (ground_z_from_crop) c.ground.z_keep_max = c.params.crop_max[2];     // (whichever of `crop` and `ground` came first)
    *cfg = c;
    return true;
}

CloudMergerNode::CloudMergerNode(const NodeConfig& cfg)
    : cfg_(cfg), have_tf_(cfg.sensors.size()), stamp_ns_(cfg.sensors.size()), submitted_(cfg.sensors.size()),
      consumed_(cfg.sensors.size()), slot_mu_(cfg.sensors.size()) {
    for (auto& f : have_tf_) f.store(false);
    for (auto& t : stamp_ns_) t.store(0);
    for (auto& f : submitted_) f.store(0);
    for (auto& f : consumed_) f.store(0);
    goal_[0] = cfg_.map_goal[0];
    goal_[1] = cfg_.map_goal[1];
    has_goal_ = cfg_.map_has_goal;
    if (cfg_.sensors.empty() || cfg_.sensors.size() > CM_MAX_SENSORS) {
        error_ = "sensor count must be 1..CM_MAX_SENSORS";
        return;
    }
    if (cfg_.align_method != "icp" && cfg_.align_method != "ndt") {
        error_ = "align_method must be icp or ndt";
        return;
    }
    if (cfg_.align_prev && cfg_.align_method == "ndt" && !(cfg_.flags & CM_FLAG_OCCUPANCY)) {
        error_ = "align_method ndt needs CM_FLAG_OCCUPANCY (the voxel covariance table)";
        return;
    }
    if (cfg_.grid_raycast && (!(cfg_.grid_cell > 0.0f) || cfg_.grid_min_pass == 0)) {
        error_ = "grid_raycast needs grid_cell > 0 and grid_min_pass >= 1";
        return;
    }
    if (cfg_.mcl_enable && !(cfg_.map_cell > 0.0f && cfg_.map_inflation_radius > 0.0f)) {
        error_ = "mcl needs the cost layer (map and map_inflation)";
        return;
    }
    if (cfg_.cast_enable && !(cfg_.map_cell > 0.0f && cfg_.map_inflation_radius > 0.0f)) {
        error_ = "cast needs the cost layer (map and map_inflation)";
        return;
    }
    uint32_t mask = 0;
    for (size_t s = 0; s < cfg_.sensors.size(); ++s)
        if (cfg_.sensors[s].required) mask |= 1u << s;
    cfg_.params.required_sensor_mask = mask;
    cm_limits lim{};
    lim.max_sensors = static_cast<uint32_t>(cfg_.sensors.size());
    lim.flags = cfg_.flags;
    lim.max_points_total = cfg_.max_points_total;
    auto refuse = [this](const char* what) {                            // a set-up call failed: its reason, and no context
        error_ = std::string(what) + ": " + cm_last_error(ctx_);
        cm_destroy(ctx_);
        ctx_ = nullptr;
    };
    const int st = cm_create(&ctx_, cfg_.device, &lim);
    if (st != CM_OK) {
        ctx_ = nullptr;
        error_ = std::string("cm_create: ") + cm_status_string(st);
    } else if (cfg_.ground_enable && cm_set_ground_removal(ctx_, &cfg_.ground) != CM_OK) refuse("cm_set_ground_removal");
    if (ctx_ && cfg_.sor_enable && cm_set_statistical_outlier(ctx_, &cfg_.sor) != CM_OK) refuse("cm_set_statistical_outlier");
    if (ctx_ && cfg_.map_cell > 0.0f) {
        const cm_map_params mp{cfg_.map_cell, cfg_.map_nx, cfg_.map_ny, cfg_.map_z_band[0], cfg_.map_z_band[1], cfg_.map_l_hit, cfg_.map_l_miss,
                               cfg_.map_l_min, cfg_.map_l_max, cfg_.map_l_free, cfg_.map_l_occ, cfg_.map_ray_range};
        if (cm_map_configure(ctx_, &mp) != CM_OK) refuse("cm_map_configure");
        if (ctx_ && cfg_.map_inflation_radius > 0.0f) {         // the cost layer behind the map
            const cm_cost_params cp{cfg_.map_inscribed_radius, cfg_.map_inflation_radius, cfg_.map_cost_scaling,
                                    cfg_.map_inflate_unknown ? CM_COST_INFLATE_UNKNOWN : 0u};
            if (cm_map_cost_configure(ctx_, &cp) != CM_OK) refuse("cm_map_cost_configure");
            if (ctx_ && cfg_.match_enable) {                       // the matching layer behind the cost layer
                const cm_match_params qp{cfg_.match_sigma, cfg_.match_max_dist, cfg_.match_n_a, cfg_.match_a_stride, cfg_.match_wx, cfg_.match_wy,
                                         cfg_.match_subcell ? CM_MATCH_SUBCELL : 0u};
                if (cm_map_match_configure(ctx_, &qp) != CM_OK) refuse("cm_map_match_configure");
            }
            if (ctx_ && cfg_.match_search_enable) {                // the search layer behind the cost layer, in the matching layer's place
                const cm_match_search_params sp{cfg_.match_sigma, cfg_.match_max_dist, cfg_.match_n_a, cfg_.match_a_stride, cfg_.match_search_wx,
                                                cfg_.match_search_wy, cfg_.match_search_depth, cfg_.match_search_max_nodes, cfg_.match_search_max_cells,
                                                cfg_.match_subcell ? CM_MATCH_SUBCELL : 0u};
                if (cm_map_match_search_configure(ctx_, &sp) != CM_OK) refuse("cm_map_match_search_configure");
            }
            if (ctx_ && cfg_.mcl_enable) {                         // the localisation layer behind the cost layer
                const cm_mcl_params lp{cfg_.mcl_particles, cfg_.mcl_max_beams, cfg_.mcl_range_cells, cfg_.mcl_sigma, cfg_.mcl_max_dist, cfg_.mcl_tau,
                                       cfg_.mcl_resample_frac, cfg_.mcl_resample_always ? CM_MCL_RESAMPLE_ALWAYS : 0u, cfg_.mcl_seed};
                if (cm_map_mcl_configure(ctx_, &lp) != CM_OK) refuse("cm_map_mcl_configure");
                if (ctx_ && cfg_.mcl_beam_enable) {                // its beam model: rays cast per beam in the field score's place
                    const cm_mcl_beam_params bp{cfg_.mcl_beam_over_cells, cfg_.mcl_beam_sigma, cfg_.mcl_beam_mix[0], cfg_.mcl_beam_mix[1], cfg_.mcl_beam_mix[2],
                                                cfg_.mcl_beam_plain ? CM_MCL_BEAM_PLAIN : 0u};
                    if (cm_map_mcl_beam_configure(ctx_, &bp) != CM_OK) refuse("cm_map_mcl_beam_configure");
                }
                if (ctx_ && cfg_.mcl_hyp_enable) {                 // its hypotheses and recovery
                    const cm_mcl_hyp_params hp{cfg_.mcl_hyp_bin_q, cfg_.mcl_hyp_heading_bits, cfg_.mcl_hyp_max, cfg_.mcl_inject_max, cfg_.mcl_recovery_alpha[0],
                                               cfg_.mcl_recovery_alpha[1], cfg_.mcl_kld_err, cfg_.mcl_kld_z, 0u, 0u};
                    if (cm_map_mcl_hyp_configure(ctx_, &hp) != CM_OK) refuse("cm_map_mcl_hyp_configure");
                }
            }
            if (ctx_ && cfg_.cast_enable) {                        // the cast layer behind the cost layer: one pose, evenly spaced bearings
                const cm_cast_params kp{1u, cfg_.cast_bearings, cfg_.cast_range_cells, cfg_.cast_plain ? CM_CAST_PLAIN : 0u};
                if (cm_map_cast_configure(ctx_, &kp, nullptr) != CM_OK) refuse("cm_map_cast_configure");
            }
            if (ctx_ && cfg_.map_plan_neutral > 0u) {              // the plan layer behind the cost layer
                const cm_plan_params pp{cfg_.map_plan_neutral, cfg_.map_plan_factor_q8, cfg_.map_plan_allow_unknown ? CM_PLAN_ALLOW_UNKNOWN : 0u,
                                        cfg_.map_nx * cfg_.map_ny};
                if (cm_map_plan_configure(ctx_, &pp) != CM_OK) refuse("cm_map_plan_configure");
                if (ctx_ && cfg_.map_frontier_min_cells > 0u) {    // the frontier layer behind the plan layer
                    const cm_frontier_params fp{cfg_.map_frontier_min_cells, cfg_.map_frontier_max, cfg_.map_frontier_max_cost,
                                                cfg_.map_frontier_pot_scale, cfg_.map_frontier_gain_scale};
                    if (cm_map_frontier_configure(ctx_, &fp) != CM_OK) refuse("cm_map_frontier_configure");
                }
                if (ctx_ && cfg_.traj_nv > 0u) {                   // the rollout layer behind the plan layer
                    std::vector<float> foot;
                    if (traj_footprint_lattice(cfg_.traj_footprint[0], cfg_.traj_footprint[1], cfg_.traj_footprint[2], cfg_.map_cell, &foot))
                        set_error("traj_footprint: the lattice was coarsened to CM_TRAJ_MAX_FOOT points");
                    const cm_traj_params tp{cfg_.traj_nv, cfg_.traj_nw, cfg_.traj_steps, cfg_.traj_occ_scale, cfg_.traj_goal_scale,
                                            cfg_.traj_allow_unknown ? CM_TRAJ_ALLOW_UNKNOWN : 0u};
                    if (cm_map_traj_configure(ctx_, &tp, foot.data(), static_cast<uint32_t>(foot.size() / 2)) != CM_OK) refuse("cm_map_traj_configure");
                }
            }
        }
    }
    for (size_t s = 0; ctx_ && s < cfg_.sensors.size(); ++s)
        if (cm_set_sensor_time_field(ctx_, static_cast<uint32_t>(s), cfg_.time_field[s].offset, cfg_.time_field[s].type) != CM_OK)
            refuse("cm_set_sensor_time_field");
    clock_ = [] {
        return static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(
            std::chrono::system_clock::now().time_since_epoch()).count());
    };
}

CloudMergerNode::~CloudMergerNode() {
    if (ctx_) (void)cm_sync(ctx_);
    for (void* p : pipe_registered_) if (p) (void)cm_host_unregister(p);
    if (ctx_) cm_destroy(ctx_);
}

int CloudMergerNode::set_ego_twist(const float v[3], const float w[3]) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(v[a]) || !std::isfinite(w[a])) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(twist_mu_);
    for (int a = 0; a < 3; ++a) { twist_v_[a] = v[a]; twist_w_[a] = w[a]; }
    return CM_OK;
}

// Enqueues the tick's frame (wait: and waits for it, into *r). With motion_compensation the stamps of the clouds the frame
// will read, the reference stamp and the twist go to the context first — under every slot's lock, so that no callback
// replaces a cloud between the stamps being read and the frame taking the clouds over.
int CloudMergerNode::enqueue_frame(bool wait, cm_result* r) {
    if (!cfg_.motion_compensation)
        return wait ? cm_merge_voxelize(ctx_, &cfg_.params, r) : cm_merge_voxelize_async(ctx_, &cfg_.params);
    int eq;
    {
        std::vector<std::unique_lock<std::mutex>> locks;
        for (auto& m : slot_mu_) locks.emplace_back(m);
        cm_motion mo{};
        {
            std::lock_guard<std::mutex> lk(twist_mu_);
            for (int a = 0; a < 3; ++a) { mo.v[a] = twist_v_[a]; mo.w[a] = twist_w_[a]; }
        }
        const uint64_t newest = newest_stamp();
        const uint64_t t_ref = (cfg_.stamp_from_inputs && newest) ? newest : clock_();
        mo.t_ref_ns = static_cast<int64_t>(t_ref);
        for (size_t s = 0; s < stamp_ns_.size(); ++s) mo.stamp_ns[s] = static_cast<int64_t>(stamp_ns_[s].load());
        const int ms = cm_set_ego_motion(ctx_, &mo);
        if (ms != CM_OK) return ms;
        eq = cm_merge_voxelize_async(ctx_, &cfg_.params);
        if (eq == CM_OK) motion_t_ref_ = t_ref;
    }
    if (eq != CM_OK || !wait) {
        if (wait && r) { *r = cm_result{}; r->status = eq; }
        return eq;
    }
    return cm_wait(ctx_, r);
}

int CloudMergerNode::clusters_of_frame(const cm_result& r) {
    n_clusters_ = 0;
    cluster_labels_.clear();
    cluster_boxes_.clear();
    if (!(cfg_.cluster_tolerance > 0.0f) || r.status != CM_OK) return CM_OK;
    const cm_cluster_params q{cfg_.cluster_tolerance, cfg_.cluster_min_size, cfg_.cluster_max_size, 0};
    cluster_labels_.resize(r.n_out);
    uint64_t n_clusters = 0, n_clustered = 0;
    const int st = cm_result_clusters(ctx_, &q, cluster_labels_.data(), cluster_labels_.size(), nullptr, 0, nullptr, 0,
                                      &n_clusters, &n_clustered);
    if (st != CM_OK) { cluster_labels_.clear(); set_error(cm_last_error(ctx_)); return st; }
    n_clusters_ = n_clusters;
    if (cfg_.cluster_box_angles == 0) return CM_OK;
    const cm_box_params b{q, cfg_.cluster_box_angles, cfg_.cluster_box_criterion, cfg_.cluster_box_d_min, 0};
    cluster_boxes_.resize(n_clusters);
    uint64_t n_boxes = 0;
    const int sb = cm_result_cluster_boxes(ctx_, &b, cluster_boxes_.data(), cluster_boxes_.size(), &n_boxes);
    if (sb != CM_OK || n_boxes != n_clusters) {
        cluster_boxes_.clear();
        set_error(sb != CM_OK ? cm_last_error(ctx_) : "the box table does not match the cluster table");
        return sb != CM_OK ? sb : CM_INTERNAL;
    }
    return CM_OK;
}

int CloudMergerNode::grid_of_frame(const cm_result& r) {
    grid_cells_.clear();
    grid_occupancy_.clear();
    grid_ray_cells_.clear();
    grid_cleared_.clear();
    if (!(cfg_.grid_cell > 0.0f) || r.status != CM_OK) return CM_OK;
    const cm_grid_params q{{cfg_.grid_origin[0], cfg_.grid_origin[1]}, cfg_.grid_cell, cfg_.grid_nx, cfg_.grid_ny,
                           cfg_.grid_z_band[0], cfg_.grid_z_band[1], cfg_.grid_obstacle_height, cfg_.grid_min_points};
    const size_t n = static_cast<size_t>(q.nx) * q.ny;
    grid_cells_.resize(n);
    grid_occupancy_.resize(n);
    uint64_t n_cells = 0;
    int st = cm_result_grid_map(ctx_, &q, grid_cells_.data(), n);
    if (st == CM_OK) st = cm_grid_occupancy_copy(ctx_, grid_occupancy_.data(), n, &n_cells);
    if (st != CM_OK || n_cells != n) {
        grid_cells_.clear();
        grid_occupancy_.clear();
        set_error(st != CM_OK ? cm_last_error(ctx_) : "the occupancy image does not match the grid");
        return st != CM_OK ? st : CM_INTERNAL;
    }
    if (!cfg_.grid_raycast) return CM_OK;
    // (the ray call computes the same grid map again: the two copies above are those of its base map)
    const cm_ray_params rp{cfg_.grid_min_pass, cfg_.grid_ray_range};
    grid_ray_cells_.resize(n);
    grid_cleared_.resize(n);
    st = cm_result_grid_rays(ctx_, &q, &rp, grid_ray_cells_.data(), n);
    if (st == CM_OK) st = cm_grid_ray_occupancy_copy(ctx_, grid_cleared_.data(), n, &n_cells);
    if (st != CM_OK || n_cells != n) {
        grid_ray_cells_.clear();
        grid_cleared_.clear();
        set_error(st != CM_OK ? cm_last_error(ctx_) : "the cleared image does not match the grid");
        return st != CM_OK ? st : CM_INTERNAL;
    }
    return CM_OK;
}

int CloudMergerNode::set_pose(const float pose[12]) {
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose[k])) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(pose_mu_);
    std::memcpy(pose_, pose, sizeof pose_);
    return CM_OK;
}

int CloudMergerNode::set_goal(float x, float y) {
    if (!std::isfinite(x) || !std::isfinite(y)) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(pose_mu_);
    goal_[0] = x;
    goal_[1] = y;
    has_goal_ = true;
    return CM_OK;
}

bool CloudMergerNode::explore_goal(float* x, float* y) const {
    if (frontier_info_.best == CM_FRONTIER_NONE || frontier_info_.best >= frontiers_.size()) return false;
    const uint32_t c = frontiers_[frontier_info_.best].min_pot_cell;
    if (x) *x = (static_cast<float>(map_info_.anchor[0] + static_cast<int32_t>(c % map_info_.nx)) + 0.5f) * cfg_.map_cell;
    if (y) *y = (static_cast<float>(map_info_.anchor[1] + static_cast<int32_t>(c / map_info_.nx)) + 0.5f) * cfg_.map_cell;
    return true;
}

bool CloudMergerNode::best_command(float* v, float* w) const {
    if (traj_scores_.empty() || traj_info_.best == CM_TRAJ_NONE) return false;
    if (v) *v = traj_info_.best_v;
    if (w) *w = traj_info_.best_w;
    return true;
}

int CloudMergerNode::map_of_frame(const cm_result& r) {
    if (!(cfg_.map_cell > 0.0f) || r.status != CM_OK) return CM_OK;     // (a frame without a voxel grid leaves the map as it is)
    float pose[12];
    {
        std::lock_guard<std::mutex> lk(pose_mu_);
        std::memcpy(pose, pose_, sizeof pose);
    }
    // The match in front of the integration: once the map holds a frame, the frame against it with the given pose as the prior.
    // A match the library refuses (a stale distance field after a failed epilogue) leaves the prior in place and says so.
    // match_search 1: the search layer in the exhaustive layer's place; a capacity overflow is such a refusal too.
    if ((cfg_.match_enable || cfg_.match_search_enable) && cfg_.map_inflation_radius > 0.0f) {
        matched_ = false;
        match_result_ = cm_match_result{};
        match_search_info_ = cm_match_search_info{};
        if (map_info_.n_frames > 0) {
            const int ms = cfg_.match_search_enable ? cm_map_match_search(ctx_, pose, &match_result_, &match_search_info_)
                                                    : cm_map_match_evaluate(ctx_, pose, &match_result_);
            if (ms == CM_OK) {
                matched_ = true;
                std::memcpy(pose, match_result_.pose, sizeof pose);
            } else if (ms == CM_CAPACITY && cfg_.match_search_enable) {
                match_result_ = cm_match_result{};
                set_error(cm_last_error(ctx_));
            } else {
                match_result_ = cm_match_result{};
                set_error(cm_last_error(ctx_));
                if (ms != CM_BAD_ARG) return ms;
            }
        }
        std::memcpy(matched_pose_, pose, sizeof pose);
    }
    // The localisation in front of the integration, from the pose that was set (a match does not move it): once the map holds a
    // frame, the first frame initialises the particles, every later one predicts with the planar motion since and updates. A
    // call the library refuses leaves the belief as it is and says so.
    if (cfg_.mcl_enable && cfg_.map_inflation_radius > 0.0f && map_info_.n_frames > 0) {
        float set[12];
        {
            std::lock_guard<std::mutex> lk(pose_mu_);
            std::memcpy(set, pose_, sizeof set);
        }
        const float now[3] = {set[3], set[7], std::atan2(set[4], set[0])};
        int ls = CM_OK;
        if (!mcl_started_) {
            ls = cfg_.mcl_init_uniform ? cm_map_mcl_init_uniform(ctx_)
                                       : cm_map_mcl_init_pose(ctx_, now[0], now[1], now[2], cfg_.mcl_init_sd[0], cfg_.mcl_init_sd[1], cfg_.mcl_init_sd[2]);
            mcl_started_ = ls == CM_OK;
        } else {
            const float dx = now[0] - mcl_prev_[0], dy = now[1] - mcl_prev_[1];
            const float c = std::cos(mcl_prev_[2]), s = std::sin(mcl_prev_[2]);
            float dyaw = now[2] - mcl_prev_[2];
            if (dyaw > 3.14159265f) dyaw -= 6.28318531f;
            if (dyaw < -3.14159265f) dyaw += 6.28318531f;
            ls = cm_map_mcl_predict(ctx_, c * dx + s * dy, c * dy - s * dx, dyaw, cfg_.mcl_noise[0], cfg_.mcl_noise[1], cfg_.mcl_noise[2]);
            if (ls == CM_OK) ls = cm_map_mcl_update(ctx_, &mcl_info_);
            if (ls == CM_OK && cfg_.mcl_beam_enable) ls = cm_map_mcl_beam_info_copy(ctx_, &mcl_beam_info_);
            if (ls == CM_OK && cfg_.mcl_hyp_enable) {
                mcl_hyp_.resize(CM_MCL_HYP_MAX);
                ls = cm_map_mcl_hyp_copy(ctx_, mcl_hyp_.data(), mcl_hyp_.size(), &mcl_hyp_info_);
                mcl_hyp_.resize(ls == CM_OK ? mcl_hyp_info_.n_hyp : 0u);
            }
        }
        if (ls == CM_OK) {
            std::memcpy(mcl_prev_, now, sizeof now);
            mcl_particles_.resize(cfg_.mcl_particles);
            ls = cm_map_mcl_copy(ctx_, mcl_particles_.data(), mcl_particles_.size());
        }
        if (ls != CM_OK) {
            set_error(cm_last_error(ctx_));
            if (ls != CM_BAD_ARG) return ls;
        }
    }
    const size_t n = static_cast<size_t>(cfg_.map_nx) * cfg_.map_ny;
    map_cells_.resize(n);
    map_image_.resize(n);
    int st = cm_map_integrate(ctx_, pose, &map_info_);
    if (st == CM_OK) st = cm_map_copy(ctx_, map_cells_.data(), n, nullptr);
    if (st == CM_OK) st = cm_map_occupancy_copy(ctx_, map_image_.data(), n, nullptr);
    if (cfg_.map_inflation_radius > 0.0f) {
        map_cost_.resize(n);
        map_dist2_.resize(n);
        if (st == CM_OK) st = cm_map_cost_update(ctx_, nullptr);
        if (st == CM_OK) st = cm_map_cost_copy(ctx_, map_cost_.data(), n, nullptr);
        if (st == CM_OK) st = cm_map_dist_copy(ctx_, map_dist2_.data(), n, nullptr);
    }
    map_potential_.clear();
    map_path_.clear();
    map_path_info_ = cm_path_info{};
    traj_scores_.clear();
    traj_info_ = cm_traj_info{};
    frontiers_.clear();
    frontier_info_ = cm_frontier_info{};
    frontier_info_.best = CM_FRONTIER_NONE;
    if (st != CM_OK) {
        map_cells_.clear();
        map_image_.clear();
        map_cost_.clear();
        map_dist2_.clear();
        set_error(cm_last_error(ctx_));
        return st;
    }
    // The virtual scan of the map behind the cost update: one pose, the one that was set (a match does not move it). A call the
    // library refuses leaves the scan empty and says so.
    cast_rays_.clear();
    cast_info_ = cm_cast_info{};
    if (cfg_.cast_enable && cfg_.map_inflation_radius > 0.0f) {
        float set[12];
        {
            std::lock_guard<std::mutex> lk(pose_mu_);
            std::memcpy(set, pose_, sizeof set);
        }
        const double yaw = std::atan2(static_cast<double>(set[4]), static_cast<double>(set[0]));
        const cm_cast_pose cp{set[3], set[7], static_cast<uint32_t>(static_cast<int64_t>(std::rint(yaw * (4294967296.0 / 6.283185307179586))))};
        cast_rays_.resize(cfg_.cast_bearings);
        int cs = cm_map_cast_evaluate(ctx_, &cp, 1u, &cast_info_);
        if (cs == CM_OK) cs = cm_map_cast_copy(ctx_, cast_rays_.data(), cast_rays_.size(), nullptr);
        if (cs != CM_OK) {
            cast_rays_.clear();
            cast_info_ = cm_cast_info{};
            set_error(cm_last_error(ctx_));
            if (cs != CM_BAD_ARG) return cs;
        }
    }
    // The plan behind the cost update: the potential to the goal, then the path from the vehicle cell. A goal or a vehicle
    // outside the window is the caller's to mend (the window has scrolled away from it): the frame stands, the plan is empty.
    float goal[2];
    bool has_goal;
    {
        std::lock_guard<std::mutex> lk(pose_mu_);
        goal[0] = goal_[0];
        goal[1] = goal_[1];
        has_goal = has_goal_;
    }
    if (cfg_.map_goal_vehicle) {                       // exploration: the goal is where the vehicle is
        goal[0] = pose[3];
        goal[1] = pose[7];
        has_goal = true;
    }
    if (cfg_.map_inflation_radius > 0.0f && cfg_.map_plan_neutral > 0u && has_goal) {
        map_potential_.resize(n);
        map_path_.resize(n);
        int ps = cm_map_plan_update(ctx_, goal[0], goal[1], &map_plan_info_, nullptr);
        if (ps == CM_OK) ps = cm_map_plan_copy(ctx_, map_potential_.data(), n, nullptr, nullptr);
        if (ps == CM_OK) ps = cm_map_plan_path(ctx_, pose[3], pose[7], map_path_.data(), n, &map_path_info_);
        if (ps == CM_OK) map_path_.resize(map_path_info_.n_cells);
        else {
            map_potential_.clear();
            map_path_.clear();
            map_path_info_ = cm_path_info{};
            set_error(cm_last_error(ctx_));
            if (ps != CM_BAD_ARG) return ps;
        }
        // The frontiers behind the plan: the table, and the choice among its entries. No frontier with a reachable cell is an
        // answer, not a failure: explore_goal() is empty and error() says so.
        if (ps == CM_OK && cfg_.map_frontier_min_cells > 0u) {
            int fs = cm_map_frontier_update(ctx_, &frontier_info_, nullptr);
            if (fs == CM_OK) {
                frontiers_.resize(frontier_info_.n_written);
                fs = cm_map_frontier_copy(ctx_, frontiers_.data(), frontiers_.size(), nullptr);
            }
            if (fs != CM_OK) {
                frontiers_.clear();
                frontier_info_ = cm_frontier_info{};
                frontier_info_.best = CM_FRONTIER_NONE;
                set_error(cm_last_error(ctx_));
                if (fs != CM_BAD_ARG) return fs;
            } else if (frontier_info_.best == CM_FRONTIER_NONE) {
                set_error("no frontier with a reachable cell: nothing to explore");
            }
        }
        // The rollout behind the plan: every velocity sample from the pose. Without a plan there is nothing to score against;
        // a start the library refuses leaves the results empty like the path.
        if (ps == CM_OK && cfg_.traj_nv > 0u) {
            const cm_traj_window w{pose[3], pose[7], std::atan2(pose[4], pose[0]), cfg_.traj_limits[0], cfg_.traj_limits[1],
                                   cfg_.traj_limits[2], cfg_.traj_limits[3], cfg_.traj_dt};
            traj_scores_.resize(static_cast<size_t>(cfg_.traj_nv) * cfg_.traj_nw);
            int ts = cm_map_traj_evaluate(ctx_, &w, &traj_info_);
            if (ts == CM_OK) ts = cm_map_traj_copy(ctx_, traj_scores_.data(), traj_scores_.size(), nullptr);
            if (ts != CM_OK) {
                traj_scores_.clear();
                traj_info_ = cm_traj_info{};
                set_error(cm_last_error(ctx_));
                if (ts != CM_BAD_ARG) return ts;
            }
        }
    }
    return CM_OK;
}

int CloudMergerNode::normals_of_frame(const cm_result& r) {
    normals_.clear();
    if (cfg_.normals_k == 0 || r.status != CM_OK) return CM_OK;
    cm_normal_params q{};
    q.k = cfg_.normals_k;
    for (int a = 0; a < 3; ++a) q.viewpoint[a] = cfg_.normals_viewpoint[a];
    normals_.resize(r.n_out);
    const int st = cm_result_normals(ctx_, &q, normals_.data(), normals_.size());
    if (st != CM_OK) { normals_.clear(); set_error(cm_last_error(ctx_)); return st; }
    return CM_OK;
}

int CloudMergerNode::align_of_frame(const cm_result& r) {
    has_alignment_ = false;
    if (!cfg_.align_prev) return CM_OK;
    if (r.status != CM_OK) { prev_records_.clear(); return CM_OK; }
    auto common = [this](auto& q) {                                     // what both matchers take; the guess is the identity
        q.max_iterations = cfg_.align_max_iterations;
        q.min_correspondences = 6;
        q.trans_eps = q.rot_eps = 1e-6;
        q.guess[0] = q.guess[5] = q.guess[10] = 1.0;
    };
    if (!prev_records_.empty() && cfg_.align_method == "ndt") {
        cm_ndt_params q{};
        q.outlier_ratio = 0.55f;
        q.neighborhood = 7;
        common(q);
        const int st = cm_result_ndt_align(ctx_, &q, prev_records_.data(), prev_records_.size() / 4, &ndt_alignment_);
        if (st != CM_OK) { set_error(cm_last_error(ctx_)); return st; }
        const cm_ndt_result& n = ndt_alignment_;
        alignment_ = cm_align_result{};
        std::memcpy(alignment_.pose, n.pose, sizeof n.pose);
        std::memcpy(alignment_.H, n.H, sizeof n.H);
        std::memcpy(alignment_.g, n.g, sizeof n.g);
        std::memcpy(alignment_.pivot, n.pivot, sizeof n.pivot);
        alignment_.n_corr = n.n_corr;
        alignment_.iterations = n.iterations;
        alignment_.flags = n.flags;
        has_alignment_ = true;
    } else if (!prev_records_.empty()) {
        cm_align_params q{};
        q.max_corr_dist = cfg_.align_max_corr;
        q.normals_k = cfg_.align_normals_k;
        common(q);
        const int st = cm_result_align(ctx_, &q, prev_records_.data(), prev_records_.size() / 4, &alignment_);
        if (st != CM_OK) { set_error(cm_last_error(ctx_)); return st; }
        has_alignment_ = true;
    }
    // this frame's records, for the next frame (the 16-byte records of cm_result_copy, whatever layout is published)
    prev_records_.resize(static_cast<size_t>(r.n_out) * 4);
    const int st = r.n_out ? cm_result_copy(ctx_, prev_records_.data(), r.n_out, 16) : CM_OK;
    if (st != CM_OK) { prev_records_.clear(); set_error(cm_last_error(ctx_)); return st; }
    return CM_OK;
}

uint64_t CloudMergerNode::newest_stamp() const {
    uint64_t newest = 0;
    for (const auto& t : stamp_ns_) newest = std::max(newest, t.load());
    return newest;
}

void CloudMergerNode::flush_published() {
    if (!pipe_in_flight_ || !ctx_) return;
    (void)cm_publish_wait(ctx_);
    pipe_in_flight_ = false;
    if (publish_) publish_(cfg_.voxel_topic, pipe_msg_[pipe_cur_ ^ 1]);
    frames_.fetch_add(1);
}

// deferred_wait: the frame enqueued by the last spin_once, if any — the one before it goes out, this one is waited for.
int CloudMergerNode::collect_pending(cm_result* res) {
    if (!frame_pending_ || !ctx_) return CM_OK;
    flush_published();
    frame_pending_ = false;
    return collect_and_publish_async(res);
}

void CloudMergerNode::flush() {
    (void)collect_pending(nullptr);
    flush_published();
}

// After a successful wait, on either path: the path counters, the by-products (the first to fail ends the tick), the generations.
int CloudMergerNode::after_wait(const cm_result& r) {
    if (r.path_flags & CM_PATH_QUANTILE) n_quantile_.fetch_add(1);
    if (r.path_flags & CM_PATH_REDONE) n_redone_.fetch_add(1);
    int st = clusters_of_frame(r);
    if (st == CM_OK) st = grid_of_frame(r);
    if (st == CM_OK) st = map_of_frame(r);
    if (st == CM_OK) st = normals_of_frame(r);
    if (st == CM_OK) st = align_of_frame(r);
    if (st != CM_OK) return st;
    // flag reset, :151-157 — for exactly the clouds this fuse read: a callback may have delivered the next one since
    cm_frame_stats fs;
    if (cm_get_frame_stats(ctx_, &fs) == CM_OK)
        for (uint32_t k = 0; k < fs.n_sensors; ++k)
            if (fs.sensor[k] < consumed_.size()) consumed_[fs.sensor[k]].store(fs.generation[k]);
    return CM_OK;
}

// publishPointcloud, voxel leg (:215-219): the configured layout and the frame's shape; the payload is the caller's to fill.
void CloudMergerNode::shape_message(PointCloud2& msg, const cm_result& r, int st) {
    const bool pcl = cfg_.publish_pcl_layout;
    if (msg.fields.empty() || msg.point_step != (pcl ? 32u : 16u)) msg = pcl ? make_pcl_xyzi_message(0) : make_xyzi16_message(0);
    msg.height = 1; msg.width = static_cast<uint32_t>(r.n_out);
    msg.row_step = msg.point_step * msg.width;
    msg.data.resize(static_cast<size_t>(r.n_out) * msg.point_step);    // (capacity is kept: no zero-fill in steady state)
    if (st == CM_EMPTY_INPUT) { msg.width = 0; msg.height = 0; msg.row_step = 0; }   // A.4 step 1
}

// ... its header (:217-218). input_stamp: the newest stamp among the clouds the frame fused — each path reads it at its own moment.
void CloudMergerNode::stamp_message(PointCloud2& msg, uint64_t input_stamp) {
    msg.header.seq = seq_++;
    msg.header.stamp_ns = cfg_.motion_compensation ? motion_t_ref_ : (cfg_.stamp_from_inputs && input_stamp) ? input_stamp : clock_();
    msg.header.frame_id = cfg_.base_frame;
}

// spin_once with NodeConfig::pipelined_publish: enqueue frame n; while it computes, finish and publish frame n - 1; wait
// for frame n; start its copy-out (cm_result_publish_async: a stream of its own, double-buffered result) and return.
int CloudMergerNode::spin_once_pipelined(cm_result* res) {
    int eq;
    {
        SlowTick tick{"enqueue", "flush"};
        const uint64_t stamp_enq = newest_stamp();                      // (of the clouds this fuse reads: a callback may deliver the next ones before the wait)
        eq = enqueue_frame(false, nullptr);                             // fusePointclouds + voxelgrid, enqueued
        if (eq == CM_OK) enq_stamp_ = stamp_enq;
        tick.lap(0);
        flush_published();                                              // frame n - 1 goes out while frame n runs
        tick.lap(1);
    }
    if (res) *res = cm_result{};
    if (eq == CM_NOT_READY) return eq;                                  // :575 — nothing fused this tick
    if (eq < 0) { set_error(cm_last_error(ctx_)); return eq; }
    return collect_and_publish_async(res);
}

// spin_once with NodeConfig::deferred_wait (on top of pipelined_publish): the frame enqueued by the LAST call is waited for and
// its copy-out started, then this tick's frame is enqueued and the call returns without waiting for it — the kernels of frame
// n run while the subscriber callbacks of tick n + 1 copy their clouds to the device (a sensor's submit goes to the buffer
// the frame in flight does not read: cm_ctx.hpp Slot). The return value says whether THIS tick fused a frame (CM_OK /
// CM_NOT_READY, as always); `res` is the PREVIOUS frame's result (zero when there was none to wait for).
int CloudMergerNode::spin_once_deferred(cm_result* res) {
    if (res) *res = cm_result{};
    const int st_prev = collect_pending(res);                           // frame n - 2 goes out; frame n - 1: waited for, copy-out started
    if (st_prev < 0) return st_prev;
    const uint64_t stamp_enq = newest_stamp();
    const int eq = enqueue_frame(false, nullptr);                       // frame n: enqueued, not waited for
    if (eq == CM_OK) { frame_pending_ = true; enq_stamp_ = stamp_enq; }
    else if (eq != CM_NOT_READY) { set_error(cm_last_error(ctx_)); return eq; }
    return eq;                                                          // CM_OK: a frame was fused this tick; CM_NOT_READY: none (:575)
}

// The frame in flight on the context: cm_wait, the by-products, its message, the start of its copy-out.
int CloudMergerNode::collect_and_publish_async(cm_result* res) {
    SlowTick tick{"wait", "publish"};
    cm_result r{};
    const int st = cm_wait(ctx_, &r);
    tick.lap(0);
    if (res) *res = r;
    if (st < 0) { set_error(cm_last_error(ctx_)); return st; }
    { const int bs = after_wait(r); if (bs != CM_OK) return bs; }
    PointCloud2& msg = pipe_msg_[pipe_cur_];
    shape_message(msg, r, st);
    // The payload buffer is reserved once at the largest cloud the context can produce and made DMA-able: the copy-out
    // then is a true asynchronous transfer straight into the message that goes on the wire.
    const size_t cap_bytes = static_cast<size_t>(cfg_.max_points_total) * msg.point_step;
    if (msg.data.capacity() < cap_bytes || pipe_registered_[pipe_cur_] != msg.data.data()) {
        if (pipe_registered_[pipe_cur_]) { (void)cm_host_unregister(pipe_registered_[pipe_cur_]); pipe_registered_[pipe_cur_] = nullptr; }
        msg.data.resize(cap_bytes);                                     // (every page touched once before it is pinned)
        msg.data.resize(1);                                             // (capacity stays; data() of an empty vector need not be its buffer)
        if (cm_host_register(msg.data.data(), cap_bytes) == CM_OK) pipe_registered_[pipe_cur_] = msg.data.data();
        msg.data.resize(static_cast<size_t>(r.n_out) * msg.point_step); // (the frame's size again, within the reserved capacity: the buffer stays put)
    }
    if (r.n_out) {
        const int cs = cm_result_publish_async(ctx_, msg.data.data(), r.n_out, msg.point_step);
        if (cs != CM_OK) { set_error(cm_last_error(ctx_)); return cs; }
    }
    stamp_message(msg, enq_stamp_);                                     // (read at enqueue: a callback may have delivered since)
    pipe_in_flight_ = true;
    pipe_cur_ ^= 1;
    tick.lap(1);
    return st;
}

int CloudMergerNode::sensor_by_topic(const std::string& topic) const {
    for (size_t s = 0; s < cfg_.sensors.size(); ++s)
        if (cfg_.sensors[s].topic == topic) return static_cast<int>(s);
    return -1;
}

int CloudMergerNode::set_transform(size_t sensor, const double q[4], const double t[3]) {
    if (!ctx_ || sensor >= cfg_.sensors.size()) return CM_BAD_ARG;
    const int st = cm_set_sensor_transform(ctx_, static_cast<uint32_t>(sensor), q, t);
    if (st == CM_OK) have_tf_[sensor].store(true);
    return st;
}

bool CloudMergerNode::transforms_ready() const {
    for (const auto& f : have_tf_)
        if (!f.load()) return false;
    return true;
}

int CloudMergerNode::on_cloud(size_t sensor, const PointCloud2& msg, bool* accepted) {
    if (accepted) *accepted = false;
    if (!ctx_ || sensor >= cfg_.sensors.size()) return CM_BAD_ARG;
    if (!transforms_ready()) return CM_NOT_READY;
    const XyziLayout l = find_xyzi(msg);
    if (!l.ok) { set_error(l.error); return CM_BAD_ARG; }
    std::lock_guard<std::mutex> lk(slot_mu_[sensor]);
    const int st = (cfg_.async_submit ? cm_submit_cloud_async : cm_submit_cloud)(ctx_, static_cast<uint32_t>(sensor), msg.data.data(),
                                   static_cast<uint32_t>(msg.num_points()), msg.point_step, l.off_x, l.off_y, l.off_z, l.off_i);
    if (st == CM_OK) { stamp_ns_[sensor].store(msg.header.stamp_ns); submitted_[sensor].fetch_add(1); }   // CM_SKIPPED: the slot keeps its older cloud
    if (accepted) *accepted = st == CM_OK;
    return st == CM_SKIPPED ? CM_OK : st;
}

int CloudMergerNode::spin_once(cm_result* res) {
    if (!ctx_) return CM_NO_DEVICE;
    if (cfg_.max_stamp_spread_ns) {
        // The set the gate (:134) would fuse: every required sensor's unconsumed cloud. Too far apart in time:
        // drop the oldest and wait for that sensor's next cloud.
        bool complete = true;
        uint64_t lo = ~0ull, hi = 0;
        size_t oldest = 0;
        for (size_t s = 0; s < cfg_.sensors.size(); ++s) {
            if (!cfg_.sensors[s].required) continue;
            if (!fresh(s)) { complete = false; break; }
            const uint64_t t = stamp_ns_[s].load();
            if (t < lo) { lo = t; oldest = s; }
            hi = std::max(hi, t);
        }
        if (complete && hi - lo > cfg_.max_stamp_spread_ns) {
            std::lock_guard<std::mutex> lk(slot_mu_[oldest]);          // (no callback of that sensor between the clear and the reset)
            cm_clear_sensor(ctx_, static_cast<uint32_t>(oldest));
            consumed_[oldest].store(submitted_[oldest].load());
            stamp_ns_[oldest].store(0);
            dropped_.fetch_add(1);
            return CM_NOT_READY;
        }
    }
    if (cfg_.pipelined_publish && !cfg_.ground_enable) return (cfg_.deferred_wait && !cfg_.max_stamp_spread_ns) ? spin_once_deferred(res) : spin_once_pipelined(res);   // (the stamp gate above reads what the last frame consumed: known only once it was waited for)
    cm_result r{};
    const int st = enqueue_frame(true, &r);                         // fusePointclouds + voxelgrid
    if (res) *res = r;
    if (st == CM_NOT_READY) return st;                              // :575 — nothing fused this tick
    if (st < 0) { set_error(cm_last_error(ctx_)); return st; }
    { const int bs = after_wait(r); if (bs != CM_OK) return bs; }
    shape_message(out_msg_, r, st);
    if (r.n_out) {
        const int cs = cm_result_copy(ctx_, out_msg_.data.data(), r.n_out, out_msg_.point_step);
        if (cs != CM_OK) { set_error(cm_last_error(ctx_)); return cs; }
    }
    stamp_message(out_msg_, newest_stamp());                             // (read after the wait: stamp = now without stamp_from_inputs, :217)
    if (cfg_.ground_enable && publish_ && st != CM_EMPTY_INPUT) {
        // publishPointcloud's other two legs (:203-213): the fused no-ground and ground clouds
        for (int leg = 0; leg < 2; ++leg) {
            uint64_t n = 0;
            PointCloud2& m2 = side_msg_;
            if (m2.fields.empty()) m2 = make_xyzi16_message(0);
            m2.data.resize(static_cast<size_t>(r.n_in) * m2.point_step);
            const int cs = leg == 0 ? cm_merged_copy(ctx_, m2.data.data(), r.n_in, &n) : cm_ground_copy(ctx_, m2.data.data(), r.n_in, &n);
            if (cs != CM_OK) { set_error(cm_last_error(ctx_)); return cs; }
            m2.width = static_cast<uint32_t>(n); m2.height = n ? 1 : 0; m2.row_step = static_cast<uint32_t>(n) * m2.point_step;
            m2.data.resize(static_cast<size_t>(n) * m2.point_step);
            m2.header = out_msg_.header;
            publish_(leg == 0 ? cfg_.no_ground_topic : cfg_.ground_topic, m2);
        }
    }
    if (publish_) publish_(cfg_.voxel_topic, out_msg_);
    frames_.fetch_add(1);
    return st;
}

void CloudMergerNode::run(const std::atomic<bool>& stop) {
    const auto period = std::chrono::duration<double>(1.0 / cfg_.rate_hz);
    auto next = std::chrono::steady_clock::now();
    while (!stop.load()) {
        spin_once();
        next += std::chrono::duration_cast<std::chrono::steady_clock::duration>(period);
        std::this_thread::sleep_until(next);                        // loop_rate.sleep(), :583
    }
}

}  // namespace cloudmerge
