// merger_node.hpp — C++ host shell with the reference node's surface: subscribe N sensor clouds,
// publish one merged + voxel-filtered cloud. It re-creates the thin L3 layer of
// pcl_preprocessing/src/pc_preprocessing_main.cpp (main :509-587, callbacks :318-508) on top of
// the C-ABI in include/cloudmerge.h; every numeric step runs in libcloudmerge_hip.so.
//
// The SURVEY.md §8f "next" rows ride on the same surface: zone-wise RANSAC ground removal (:49-122, :228-312;
// live_node_config(), NodeConfig::ground*) and radius outlier removal on the fused cloud (cm_params.outlier_*).
#pragma once
#include <atomic>
#include <cstdint>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cloudmerge.h"
#include "pointcloud2.hpp"

namespace cloudmerge {

struct SensorSpec {
    std::string name;       // "front_right", ...
    std::string topic;      // input topic (:520-525)
    std::string frame;      // TF frame looked up against the base frame (:556-561)
    bool required = true;   // part of the fuse gate (:134); top_middle is not (:136)
};

struct NodeConfig {
    std::vector<SensorSpec> sensors;
    std::string base_frame = "base_footprint";     // frame_id of everything published (:206,:212,:218)
    std::string voxel_topic = "/points_voxel";      // :518
    double rate_hz = 10.0;                          // ros::Rate loop_rate(10) :527
    cm_params params{};                             // Parameter.h:27-35 by default
    uint64_t max_points_total = 4u << 20;
    int device = 0;
    uint32_t flags = 0;
    bool publish_pcl_layout = true;                 // 32-byte pcl::PointXYZI records like pcl::toROSMsg
    // Pipelined publish: spin_once() enqueues frame n, publishes frame n - 1 (whose copy-out has been running on a stream of
    // its own, into a DMA-able message buffer) while frame n computes, then starts frame n's copy-out and returns — the
    // voxel cloud reaches its subscribers one tick later, the loop no longer waits for PCIe (flush() publishes the last
    // one). Off by default: the reference publishes within the tick (:574-577). Not with ground_enable (three clouds per tick).
    bool pipelined_publish = false;
    // deferred_wait (needs pipelined_publish): spin_once enqueues this tick's frame and returns; the NEXT call waits for it. The
    // frame's kernels then run while the next tick's callbacks copy their clouds to the device — for replays and bulk
    // conversion, where frames per second count; a live 10 Hz node gains nothing and loses a tick of latency. spin_once's
    // return value still says whether THIS tick fused a frame; its cm_result is the previous frame's.
    bool deferred_wait = false;
    // async_submit: on_cloud returns behind the ENQUEUE of the host-to-device copy (cm_submit_cloud_async); the frame that
    // fuses the cloud waits for the copy on the device. The message's payload must then stay valid and unchanged until that
    // frame has been waited for — a transport that keeps its receive buffers (and registers them: cm_host_register) can say
    // so; a callback whose message dies when it returns cannot.
    bool async_submit = false;
    // Stamp of the published cloud. false: ros::Time::now() at publish like the reference (:217).
    // true: the newest stamp among the fused input clouds — what pcl::PointCloud::operator+= leaves in
    // the fused cloud's header and what §8f rank 4 proposes.
    bool stamp_from_inputs = false;
    // Approximate time synchronisation (the reference fuses whatever arrived first since
    // the last fuse, however far apart in time). 0: off. Otherwise a frame is fused only when the stamps of the
    // required sensors' clouds lie within this many nanoseconds of each other; if they do not, the oldest
    // cloud is dropped and the tick is skipped, so that sensor's next cloud can complete the set.
    uint64_t max_stamp_spread_ns = 0;
    // Zone-wise ground removal before the fuse (cm_set_ground_removal). Off in
    // reference_config() (the north-star path); live_node_config() switches it on with the reference's slabs.
    bool ground_enable = false;
    cm_ground_params ground{};
    std::string no_ground_topic = "/points_no_ground";   // :516
    std::string ground_topic = "/points_ground";          // :517
    // Ego-motion compensation (deskew) before the merge (cm_set_ego_motion; an extension, the reference has none). Off by
    // default. On: every frame moves each sensor's points from the instant they were measured — the cloud's header stamp
    // plus the point's own time field, when the sensor has one — into the vehicle frame at the stamp the frame is published
    // with, by the twist set_ego_twist() last gave. That stamp is then fixed when the frame is enqueued (the newest input
    // stamp with stamp_from_inputs, else the clock at that moment).
    bool motion_compensation = false;
    // Statistical outlier removal on the fused cloud before the voxel grid (cm_set_statistical_outlier;
    // pcl::StatisticalOutlierRemoval). Off by default; not combined with `outlier` or `ground`.
    bool sor_enable = false;
    cm_sor_params sor{};
    // Euclidean cluster extraction on every published voxel cloud (cm_result_clusters; pcl::EuclideanClusterExtraction). Off
    // by default (tolerance 0). On: after the frame has been waited for the node asks for the labels and keeps them, with
    // the cluster count, until the next frame (cluster_count(), cluster_labels()).
    float cluster_tolerance = 0.0f;
    uint32_t cluster_min_size = 1, cluster_max_size = 0xFFFFFFFFu;
    // Oriented boxes of those clusters (cm_result_cluster_boxes; search-based L-shape fitting). Off by default (angles 0) and
    // without cluster_tolerance. On: the node asks for the box table behind the labels and keeps it until the next frame
    // (cluster_boxes(): entry k belongs to cluster k). The call extracts the clusters a second time.
    uint32_t cluster_box_angles = 0;
    uint32_t cluster_box_criterion = CM_BOX_CLOSENESS;
    float cluster_box_d_min = 0.01f;
    // 2-D grid map of every frame (cm_result_grid_map: per-cell counts, lowest and highest return, occupancy; the image is
    // nav_msgs/OccupancyGrid::data). Off by default (grid_cell 0). On: after the frame has been waited for the node asks for
    // the table and the image and keeps them until the next frame (grid_cells(), grid_occupancy()). The origin is the corner of
    // cell (0, 0) in the base frame.
    float grid_cell = 0.0f;
    float grid_origin[2] = {0.0f, 0.0f};
    uint32_t grid_nx = 1, grid_ny = 1;
    float grid_z_band[2] = {-std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity()};
    float grid_obstacle_height = 0.3f;
    uint32_t grid_min_points = 1;
    // Free-space ray casting over that grid map (cm_result_grid_rays: per cell the rays that cross it and that end in it, and the
    // image in which an unknown cell crossed by grid_min_pass rays is free). Off by default (grid_raycast 0); on, it needs
    // grid_cell > 0. The node then asks for the ray table and the cleared image as well and keeps them until the next frame
    // (grid_ray_cells(), grid_cleared()). grid_ray_range: steps of a ray from its sensor that count, 0 = to the return.
    bool grid_raycast = false;
    uint32_t grid_min_pass = 1;
    uint32_t grid_ray_range = 0;
    // Rolling log-odds occupancy map accumulated over the frames (cm_map_configure, cm_map_integrate). Off by default
    // (map_cell 0). On: the node configures a window of map_nx x map_ny cells that scrolls with the vehicle, and after every
    // frame that has been waited for integrates it under the pose set_pose() last gave (the identity until then), then keeps
    // the state table, the image and the info until the next frame (map_cells(), map_image(), map_info()). The log-odds are
    // integers: the defaults are octomap's 0.85 / -0.4, clamps -2 and 3.5, thresholds -0.4 and 0.85, times 100.
    float map_cell = 0.0f;
    uint32_t map_nx = 1, map_ny = 1;
    float map_z_band[2] = {-std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity()};
    int32_t map_l_hit = 85, map_l_miss = 40, map_l_min = -200, map_l_max = 350;
    int32_t map_l_free = -40, map_l_occ = 85;
    uint32_t map_ray_range = 0;
    // Cost layer over that map (cm_map_cost_configure, cm_map_cost_update): costmap_2d's inflation layer and the exact distance
    // field under it. Off by default (an inflation radius of 0). On (it needs map_cell > 0): the node configures the layer
    // behind the map, updates it behind every integration and keeps the two tables until the next frame (map_cost(), map_dist2()).
    float map_inscribed_radius = 0.0f, map_inflation_radius = 0.0f, map_cost_scaling = 0.0f;
    bool map_inflate_unknown = false;
    // Plan layer behind that cost layer (cm_map_plan_configure, cm_map_plan_update, cm_map_plan_path): the shortest-path
    // potential to a goal and the path from the vehicle cell. Off by default (neutral 0). On (it needs an inflation radius
    // > 0): the node configures the layer behind the cost layer and, once a goal is known (map_goal, set_goal()), updates the
    // potential behind every cost update and walks the path from the pose's cell (map_potential(), map_path()).
    uint32_t map_plan_neutral = 0, map_plan_factor_q8 = 205;
    bool map_plan_allow_unknown = false;
    bool map_has_goal = false;
    float map_goal[2] = {0.0f, 0.0f};                // world frame, metres
    // Frontier layer behind that plan layer (cm_map_frontier_configure, cm_map_frontier_update): the connected frontiers of
    // the map's image and the one to explore next. Off by default (min_cells 0). On (it needs map_plan): the node configures
    // the layer behind the plan layer and updates it behind every plan update (frontiers(), frontier_info(), explore_goal()).
    // map_goal_vehicle makes the plan's goal of every frame the pose's cell instead of map_goal, which is what exploration
    // wants: pot is then the cost of the walk between a cell and the vehicle.
    uint32_t map_frontier_min_cells = 0, map_frontier_max = 256, map_frontier_max_cost = 252;
    uint32_t map_frontier_pot_scale = 1, map_frontier_gain_scale = 0;
    bool map_goal_vehicle = false;
    // Rollout layer behind that plan layer (cm_map_traj_configure, cm_map_traj_evaluate): sampled velocity commands rolled
    // forward from the pose and scored over the cost table and the potential. Off by default (traj_nv 0). On (it needs the plan
    // layer): the node lays a filled lattice over the footprint rectangle (traj_footprint_lattice), configures the layer behind
    // the plan layer and evaluates it behind every plan update, from the pose with yaw = atan2f(P[4], P[0]) (traj_scores(),
    // traj_info(), best_command()).
    uint32_t traj_nv = 0, traj_nw = 1, traj_steps = 1;
    float traj_dt = 0.1f;                            // seconds per step
    float traj_limits[4] = {0.0f, 1.0f, -1.0f, 1.0f};   // v_lo, v_hi (m/s), w_lo, w_hi (rad/s)
    float traj_footprint[3] = {0.0f, 0.0f, 0.0f};    // x_back, x_front, half_width (metres, body frame): the one point (0, 0) by default
    uint32_t traj_occ_scale = 1, traj_goal_scale = 1;
    bool traj_allow_unknown = false;
    // Scan matching of every frame against the map (cm_map_match_configure, cm_map_match_evaluate): a search over angle
    // candidates and shifts around the pose set_pose() gave. Off by default. On (it needs the cost layer): once the map holds a
    // frame and its distance field is fresh, the frame is matched with set_pose()'s pose as the prior and integrated under the
    // matched pose (matched(), match_result(), matched_pose()); the first frame, and a frame the library refuses to match, is
    // integrated under the prior.
    bool match_enable = false;
    uint32_t match_n_a = 10, match_a_stride = 2;     // angle candidates -n_a..n_a, a_stride entries of 2 pi / 4096 apart
    uint32_t match_wx = 10, match_wy = 10;           // shifts in cells
    float match_sigma = 0.1f, match_max_dist = 0.5f; // the likelihood field's standard deviation and cut (metres)
    bool match_subcell = false;
    // match_search 1: the same match by the search layer (cm_map_match_search_configure, cm_map_match_search): branch and
    // bound over shifts of up to CM_MATCH_SEARCH_MAX_SHIFT cells, with match_angles, match_field and match_subcell as above and
    // a window, a depth and capacities of its own. Off by default; `match` and `match_search` together is a config error.
    // matched() / match_result() / matched_pose() as above, and match_search_info(). A frame whose search overflows a
    // capacity is integrated under the prior, as a refused one is.
    bool match_search_enable = false;
    uint32_t match_search_wx = 128, match_search_wy = 128;
    uint32_t match_search_depth = 5;
    uint32_t match_search_max_nodes = 1u << 18, match_search_max_cells = 1u << 17;
    // The localisation layer (cm_map_mcl_configure, cm_map_mcl_update): a particle filter of the pose against the map. Off by
    // default. On (it needs the cost layer; without one load_config refuses the file and the node does not start): once the
    // map holds a frame and its distance field is fresh, the first frame initialises the particles, around set_pose()'s pose
    // (mcl_init pose) or over the map's free cells (mcl_init uniform); every later frame predicts with the planar motion between
    // the previous and the current set_pose() pose and the noise of mcl_noise, then updates (mcl_info(), mcl_particles()). The
    // pose a frame is integrated under does not change.
    bool mcl_enable = false;
    uint32_t mcl_particles = 2048;
    uint32_t mcl_max_beams = 256, mcl_range_cells = 256;
    float mcl_sigma = 0.1f, mcl_max_dist = 0.5f;     // the likelihood field, as match_field
    float mcl_tau = 8.0f;
    float mcl_resample_frac = 0.5f;
    bool mcl_resample_always = false;
    uint64_t mcl_seed = 1;
    bool mcl_init_uniform = false;                   // mcl_init uniform; otherwise around the pose with mcl_init_sd
    float mcl_init_sd[3] = {0.5f, 0.5f, 0.2f};       // sd_x, sd_y (metres), sd_yaw (radians)
    float mcl_noise[3] = {0.05f, 0.05f, 0.02f};      // sd_fwd, sd_left (metres), sd_yaw (radians) of every predict
    // Its beam model (cm_map_mcl_beam_configure): an update casts a ray per particle and beam instead of looking the beam's end
    // cell up in the field (mcl_beam_info()). Off by default; it needs mcl 1.
    bool mcl_beam_enable = false;
    float mcl_beam_sigma = 0.1f;                     // of the hit term (metres)
    uint32_t mcl_beam_over_cells = 8;                // how far past its measured end a ray is followed
    float mcl_beam_mix[3] = {0.75f, 0.125f, 0.125f}; // z_hit, z_short, z_rand
    bool mcl_beam_plain = false;                     // walk cell by cell instead of jumping
    // Its hypotheses and recovery (cm_map_mcl_hyp_configure): every update reports the clusters of the belief (mcl_hypotheses(),
    // mcl_hyp_info()) and may replace particles by random ones while the fast average of the score lies below the slow one.
    // Off by default; it needs mcl 1.
    bool mcl_hyp_enable = false;
    uint32_t mcl_hyp_bin_q = 512;                    // bin width in 1/1024 m (mcl_hyp_bins takes metres)
    uint32_t mcl_hyp_heading_bits = 5;
    uint32_t mcl_hyp_max = 8;
    float mcl_recovery_alpha[2] = {0.05f, 0.5f};     // alpha_slow, alpha_fast
    uint32_t mcl_inject_max = 0;                     // most particles one update may inject; 0: no injection
    float mcl_kld_err = 0.05f, mcl_kld_z = 2.326f;
    // The cast layer (cm_map_cast_configure, cm_map_cast_evaluate): the virtual scan of the map. Off by default. On (it needs
    // the cost layer; without one load_config refuses the file and the node does not start): after each frame's cost update
    // the node casts cast_bearings evenly spaced rays of at most cast_range_cells cells from set_pose()'s pose (cast_rays(),
    // cast_info()). cast_plain selects the cell-by-cell walk; the rays are the same.
    bool cast_enable = false;
    uint32_t cast_bearings = 360;
    uint32_t cast_range_cells = 256;
    bool cast_plain = false;
    // Normals and curvature of every published voxel cloud (cm_result_normals; pcl::NormalEstimation with setKSearch). Off by
    // default (normals_k 0). On: after the frame has been waited for the node asks for the table and keeps it until the next
    // frame (normals()). The viewpoint is in the base frame; PCL's default is the origin.
    uint32_t normals_k = 0;
    float normals_viewpoint[3] = {0.0f, 0.0f, 0.0f};
    // Frame-to-frame registration (cm_result_align; point-to-plane ICP). Off by default (align_prev 0). On: after the frame has
    // been waited for the node aligns the records it published for the previous frame to this frame's result, from the
    // identity, and keeps the outcome until the next frame (alignment()): the pose maps the previous cloud onto this one.
    bool align_prev = false;
    float align_max_corr = 0.5f;        // matching radius, metres
    uint32_t align_normals_k = 10;
    uint32_t align_max_iterations = 30;
    // The matcher of align_prev: "icp" (cm_result_align, the default) or "ndt" (cm_result_ndt_align against the frame's voxel
    // covariance table at the library's defaults; align_max_iterations applies, align_max_corr and align_normals_k do not).
    // "ndt" needs a context with CM_FLAG_OCCUPANCY: a node whose flags lack it refuses the combination at start-up.
    std::string align_method = "icp";
    struct TimeField { uint32_t offset = 0, type = CM_TIME_NONE; };
    TimeField time_field[CM_MAX_SENSORS];           // per sensor, in sensor order: cm_set_sensor_time_field
};

// Loads a node description from a text file (an N-sensor configuration instead
// of the reference's string literals). Lines, '#' comments allowed:
//   sensor <name> <topic> <tf_frame> <required|optional>
//   base_frame <id> | voxel_topic <topic> | rate_hz <v> | leaf <v> | min_points_per_voxel <n>
//   crop <x0> <y0> <z0> <x1> <y1> <z1> | no_crop | outlier <radius> <min_neighbors> | stamp_from_inputs <0|1>
//   max_points_total <n> | device <n> | max_stamp_spread_ms <v>
//   ground <max_iterations> <distance_threshold> <probability> | zone <sensor_name> <x_min> <x_length> <z_max_ground>
//   ground_outlier <radius> <min_neighbors>   (removeGround's outlierRemoval on every slab's band points, :119)
//   motion_compensation <0|1> | time_field <sensor_name> <byte_offset> <f32|u32ns>   (ego-motion compensation; f32: seconds,
//   u32ns: nanoseconds, relative to the cloud's header stamp)
//   statistical_outlier <mean_k> <std_mul> [search_cell]   (pcl::StatisticalOutlierRemoval before the voxel grid)
//   cluster_tolerance <metres> | cluster_min_size <n> | cluster_max_size <n>   (clusters of every voxel cloud; 0: off)
//   cluster_box_angles <n> | cluster_box_criterion <area|closeness> | cluster_box_d_min <metres>   (oriented boxes of those
//   clusters from n headings, 1..180; 0: off)
//   grid_cell <metres> | grid_origin <x> <y> | grid_size <nx> <ny> | grid_z_band <lo> <hi> | grid_obstacle_height <metres> |
//   grid_min_points <n>   (the 2-D grid map of every frame; grid_cell 0: off)
//   grid_raycast <0|1> | grid_min_pass <n> | grid_ray_range <cells>   (free-space ray casting over that grid map; it needs
//   grid_cell > 0; grid_ray_range 0: to the return)
//   map_cell <metres> | map_size <nx> <ny> | map_z_band <lo> <hi> | map_logodds <hit> <miss> <min> <max> |
//   map_thresholds <free> <occ> | map_ray_range <cells>   (the occupancy map accumulated over the frames; map_cell 0: off)
//   map_inflation <inscribed> <inflation> <scaling> | map_inflate_unknown <0|1>   (the cost layer over that map: radii in metres,
//   the decay per metre; an inflation radius of 0: off)
//   map_frontier <min_cells> <max_frontiers> | map_frontier_max_cost <0..252> | map_frontier_scales <pot> <gain> |
//   map_goal_vehicle <0|1>   (the frontier layer behind the plan layer: min_cells 0: off, at most 65536 table entries; with
//   map_goal_vehicle the plan's goal of every frame is the pose's cell)
//   map_plan <neutral> <factor_q8> | map_plan_allow_unknown <0|1> | map_goal <x> <y>   (the plan layer behind that cost layer:
//   neutral 1..255 and the cost's factor in 1/256, 0..256; neutral 0: off; the goal in the world frame, metres)
//   traj <nv> <nw> <n_steps> <dt> | traj_limits <v_lo> <v_hi> <w_lo> <w_hi> | traj_footprint <x_back> <x_front> <half_width> |
//   traj_scales <occ> <goal> | traj_allow_unknown <0|1>   (the rollout layer behind that plan layer: nv x nw velocity samples
//   between the limits, n_steps steps of dt seconds, the footprint rectangle in the body frame; nv 0: off)
//   match <0|1> | match_angles <n_a> <a_stride> | match_window <wx> <wy> | match_field <sigma> <max_dist> | match_subcell <0|1>
//   (scan matching of every frame against the map, behind the cost layer: 2 n_a + 1 angles a_stride table entries apart,
//   shifts of up to wx and wy cells, the field's standard deviation and cut in metres)
//   match_search <0|1> | match_search_window <wx> <wy> | match_search_depth <h> | match_search_capacity <max_nodes> <max_cells>
//   (the same match by branch and bound over shifts of up to 1024 cells, in the place of `match`: both on is an error)
//   mcl <0|1> | mcl_particles <n> | mcl_beams <max_beams> <range_cells> | mcl_field <sigma> <max_dist> | mcl_tau <tau> |
//   mcl_resample <frac> <always 0|1> | mcl_seed <seed> | mcl_init <pose sd_x sd_y sd_yaw | uniform> | mcl_noise <sd_fwd sd_left sd_yaw>
//   (the localisation layer behind the cost layer, which it needs: a file with mcl 1 and no map_inflation is refused)
//   mcl_beam <0|1> | mcl_beam_model <sigma> <over_cells> | mcl_beam_mix <z_hit> <z_short> <z_rand> | mcl_beam_plain <0|1>
//   (the localisation layer's beam model; a file with mcl_beam 1 and no mcl 1 is refused)
//   mcl_hyp <0|1> | mcl_hyp_bins <bin_m> <heading_bits> | mcl_hyp_max <n> | mcl_recovery <alpha_slow> <alpha_fast> <inject_max> |
//   mcl_kld <err> <z>   (its hypotheses and recovery; a file with mcl_hyp 1 and no mcl 1 is refused)
//   cast <0|1> | cast_bearings <n> | cast_range <cells> | cast_plain <0|1>
//   (the cast layer behind the cost layer, which it needs: the virtual scan of the map from the set pose after every frame)
//   normals_k <n> | normals_viewpoint <x> <y> <z>   (normals of every voxel cloud from n neighbours, 3..64; 0: off)
//   align_prev <0|1> | align_max_corr <metres> | align_normals_k <n> | align_max_iterations <n>   (the previous voxel cloud
//   aligned to every new one: 3..64 neighbours for the normals, 0..64 iterations)
//   align_method <icp|ndt>   (the matcher of align_prev; ndt needs the occupancy flag)
// Starts from reference_config() minus its sensors when the file names any. Returns false + *err.
bool load_config(const std::string& path, NodeConfig* cfg, std::string* err);

// The reference's literals: six sensors in fuse order fr, fl, rr, rl, tm, livox (:137-142), ROI
// crop (Parameter.h:31-35), leaf 0.1 m, min 2 points per voxel (Parameter.h:27-28).
// The rollout layer's footprint: a filled lattice over [x_back, x_front] x [-half_width, half_width] at a spacing of at most
// half a cell per axis, as (bx, by) pairs; a lattice of more than CM_TRAJ_MAX_FOOT points is laid again with both counts
// scaled down by the same factor. Returns whether that cap coarsened it.
bool traj_footprint_lattice(float x_back, float x_front, float half_width, float cell, std::vector<float>* xy);

NodeConfig reference_config();
// The live node as a whole (pcl_preprocessing): reference_config() plus the zone-wise ground removal of its
// callbacks — proceedFront for the four corner Velodynes (:228-269, called at :326,:352,:378,:404; proceedRear
// :277-312 is defined but never called), the top-middle slabs (:436-444), the Livox
// slabs (:475-497) — with Parameter.h:38-81's numbers. Publishes /points_no_ground and /points_ground as well.
NodeConfig live_node_config();
// The class-based variant (my_cloud_fusion): same sensors and ROI, plus radius outlier removal on the
// fused cloud before VoxelGrid (cloud_fusion_node.cpp:72-75).
NodeConfig fusion_config();

class CloudMergerNode {
public:
    using Publisher = std::function<void(const std::string& topic, const PointCloud2& msg)>;
    using Clock = std::function<uint64_t()>;        // nanoseconds; stands in for ros::Time::now()

    explicit CloudMergerNode(const NodeConfig& cfg);
    ~CloudMergerNode();
    CloudMergerNode(const CloudMergerNode&) = delete;
    CloudMergerNode& operator=(const CloudMergerNode&) = delete;

    bool ok() const { return ctx_ != nullptr; }
    std::string error() const { std::lock_guard<std::mutex> lk(err_mu_); return error_; }
    const NodeConfig& config() const { return cfg_; }
    int sensor_by_topic(const std::string& topic) const;

    // Result of listener.lookupTransform(base_frame, sensor.frame, Time(0)) (:556-561): the
    // quaternion/origin tf::Transform hands pcl_ros (:320).
    int set_transform(size_t sensor, const double q_xyzw[4], const double t_xyz[3]);
    bool transforms_ready() const;                  // flag_tf (:551,:562)

    // Subscriber callback body (:318-337 and siblings). Callable concurrently for different
    // sensors (AsyncSpinner(6), :513). Returns a cm_status; clouds are ignored until every
    // transform is known, like the reference, whose callbacks run on default transforms before
    // flag_tf but whose fuse gate only opens afterwards.
    // *accepted (optional): false when the slot still held an unconsumed cloud and this one was dropped (:330) — the
    // call still returns CM_OK like the reference's callback; a lossless replay waits and offers the cloud again.
    int on_cloud(size_t sensor, const PointCloud2& msg, bool* accepted = nullptr);

    // Ego twist for motion_compensation: linear (m/s) and angular (rad/s) velocity of the vehicle in the base frame, taken
    // as constant over a frame. Callable from any thread; the next fused frame uses it. Returns a cm_status (CM_BAD_ARG: not
    // finite).
    int set_ego_twist(const float v[3], const float w[3]);

    // The pose the next integrated frame enters the occupancy map with (map_cell > 0): a row-major 3 x 4 matrix from the base
    // frame at the frame's stamp into a fixed world frame, the identity until the first call. Callable from any thread.
    // Returns a cm_status (CM_BAD_ARG: not finite).
    int set_pose(const float pose[12]);

    void set_publisher(Publisher p) { publish_ = std::move(p); }
    void set_clock(Clock c) { clock_ = std::move(c); }

    // One pass of the main loop body (:570-580): fuse when the required sensors are fresh,
    // voxelise, publish. Returns CM_OK (published), CM_NOT_READY (tick skipped, :575) or an error.
    int spin_once(cm_result* res = nullptr);
    // while(ros::ok()) { spin_once(); loop_rate.sleep(); } (:549-584)
    void run(const std::atomic<bool>& stop);
    // pipelined_publish: publishes the frame whose copy-out is still in flight (end of a replay, shutdown)
    void flush();                                   // (deferred_wait: also the frame that was enqueued and not yet waited for)

    uint64_t frames_published() const { return frames_; }
    // how the fused frames were computed (cm_result.path_flags): on the one-pass quantile route / handed back and redone
    uint64_t frames_quantile() const { return n_quantile_; }
    uint64_t frames_redone() const { return n_redone_; }
    uint64_t clouds_dropped_for_sync() const { return dropped_; }
    // cluster_tolerance > 0: clusters of the frame waited for last, and the label of each of its voxels (CM_CLUSTER_NONE:
    // in no cluster), in the order of the published cloud. Read from the thread that calls spin_once.
    uint64_t cluster_count() const { return n_clusters_; }
    const std::vector<uint32_t>& cluster_labels() const { return cluster_labels_; }
    // cluster_box_angles > 0 as well: the oriented box of each of those clusters, cluster_count() entries.
    const std::vector<cm_cluster_box>& cluster_boxes() const { return cluster_boxes_; }
    // grid_cell > 0: the grid map of the frame waited for last, grid_nx * grid_ny entries, cell (ix, iy) at ix + iy * grid_nx, and
    // its occupancy image (-1 unknown, 0 free, 100 occupied); both empty where the frame has no voxel grid.
    const std::vector<cm_grid_cell>& grid_cells() const { return grid_cells_; }
    const std::vector<int8_t>& grid_occupancy() const { return grid_occupancy_; }
    // grid_raycast as well: the ray table of that frame and the cleared image, laid out like the two above; both empty where
    // the frame has no voxel grid.
    const std::vector<cm_grid_ray_cell>& grid_ray_cells() const { return grid_ray_cells_; }
    const std::vector<int8_t>& grid_cleared() const { return grid_cleared_; }
    // map_cell > 0: the occupancy map after the frame waited for last, map_nx * map_ny entries, window cell (ix, iy) at
    // ix + iy * map_nx, its image (-1 unknown, 0 free, 100 occupied) and its info (the window's anchor among them); the two
    // tables are empty until the first frame with a voxel grid.
    const std::vector<cm_map_cell>& map_cells() const { return map_cells_; }
    const std::vector<int8_t>& map_image() const { return map_image_; }
    const cm_map_info& map_info() const { return map_info_; }
    // map_inflation with a radius > 0: the inflated cost (254 lethal, 253 inscribed, 255 unknown) and the squared distance in
    // cells to the nearest occupied cell (CM_MAP_DIST_NONE: none in the window) of the same window cells, after the same frame.
    const std::vector<uint8_t>& map_cost() const { return map_cost_; }
    const std::vector<uint32_t>& map_dist2() const { return map_dist2_; }
    // map_plan with neutral > 0 and a goal: the potential of the same window cells to the goal (CM_PLAN_UNREACHABLE: none) and
    // the path from the vehicle cell, window cell indices ix + iy * nx, start first (map_path_info(): its status and cost), after
    // the same frame. Both empty while there is no goal, and after a frame whose goal or vehicle lay outside the window
    // (error() says which). set_goal replaces the configured goal from the next tick on; CM_BAD_ARG if it is not finite.
    int set_goal(float x, float y);
    const std::vector<uint32_t>& map_potential() const { return map_potential_; }
    const std::vector<uint32_t>& map_path() const { return map_path_; }
    const cm_plan_info& map_plan_info() const { return map_plan_info_; }
    const cm_path_info& map_path_info() const { return map_path_info_; }
    // map_frontier with min_cells > 0 and a plan: the table of the frontiers of the same window after the same frame, its info,
    // and the world centre of the best frontier's min_pot_cell, the place to drive to next. Empty (explore_goal false) while
    // there is no plan and after a frame that left no frontier with a reachable cell (error() says so; the frame stands).
    const std::vector<cm_frontier>& frontiers() const { return frontiers_; }
    const cm_frontier_info& frontier_info() const { return frontier_info_; }
    bool explore_goal(float* x, float* y) const;
    // traj with nv > 0, behind a plan: the score of every velocity sample from the pose of the same frame, entry i * nw + j, and
    // the best of them. Empty (best_command false) while there is no plan, and after a frame whose goal or vehicle lay outside
    // the window (error() says which).
    const std::vector<cm_traj_score>& traj_scores() const { return traj_scores_; }
    const cm_traj_info& traj_info() const { return traj_info_; }
    bool best_command(float* v, float* w) const;
    // match 1: whether the frame waited for last was matched against the map, the match and the pose it was integrated under
    // (the prior where it was not matched).
    bool matched() const { return matched_; }
    const cm_match_result& match_result() const { return match_result_; }
    const float* matched_pose() const { return matched_pose_; }
    // match_search 1: the statistics of the search behind match_result() (zeros where the frame was not matched, the overflow
    // where a capacity was exceeded).
    const cm_match_search_info& match_search_info() const { return match_search_info_; }
    // mcl 1: whether the particles are initialised, the info of the last update (zeros until the first) and the particles
    // after the last call of the layer.
    bool mcl_started() const { return mcl_started_; }
    const cm_mcl_info& mcl_info() const { return mcl_info_; }
    // mcl_beam 1: the outcome counts of the last update (zeros until the first).
    const cm_mcl_beam_info& mcl_beam_info() const { return mcl_beam_info_; }
    // mcl_hyp 1: the hypotheses of the last update, the heaviest first, and their info (empty and zeros until the first).
    const std::vector<cm_mcl_hyp>& mcl_hypotheses() const { return mcl_hyp_; }
    const cm_mcl_hyp_info& mcl_hyp_info() const { return mcl_hyp_info_; }
    const std::vector<cm_mcl_particle>& mcl_particles() const { return mcl_particles_; }
    // cast 1: the rays of the virtual scan behind the last frame's cost update (empty where the library refused the cast) and
    // their counts by status.
    const std::vector<cm_cast_ray>& cast_rays() const { return cast_rays_; }
    const cm_cast_info& cast_info() const { return cast_info_; }
    // normals_k > 0: the normal and curvature of each voxel of the frame waited for last, in the order of the published cloud.
    const std::vector<cm_voxel_normal>& normals() const { return normals_; }
    // align_prev: the registration of the previous frame's published records against the frame waited for last; false while
    // there is none (the first frame, a frame without a voxel grid, or one after such a frame).
    bool has_alignment() const { return has_alignment_; }
    const cm_align_result& alignment() const { return alignment_; }
    // align_method ndt: the call's own outcome; alignment() then carries its pose, H, g, pivot, n_corr, iterations and flags
    // (the CM_NDT_* flags are the CM_ALIGN_* ones), sse and rms 0.
    const cm_ndt_result& ndt_alignment() const { return ndt_alignment_; }

private:
    NodeConfig cfg_;
    cm_ctx* ctx_ = nullptr;
    std::vector<std::atomic<bool>> have_tf_;
    Publisher publish_;
    Clock clock_;
    mutable std::mutex err_mu_;                     // on_cloud runs on several threads at once
    std::string error_;
    void set_error(const std::string& e) { std::lock_guard<std::mutex> lk(err_mu_); error_ = e; }
    std::atomic<uint64_t> frames_{0};
    std::atomic<uint64_t> n_quantile_{0}, n_redone_{0};
    uint32_t seq_ = 0;
    PointCloud2 out_msg_, side_msg_;               // reused from frame to frame (no 3 MB zero-fill per publish)
    PointCloud2 pipe_msg_[2];                       // pipelined publish: the message being filled by the copy-out, and the one before
    void* pipe_registered_[2] = {nullptr, nullptr}; // ... their payload buffers, made DMA-able once (cm_host_register)
    int pipe_cur_ = 0;
    bool pipe_in_flight_ = false;
    bool frame_pending_ = false;                    // deferred_wait: a frame is enqueued on the context and not yet waited for
    uint64_t enq_stamp_ = 0;                        // pipelined modes: newest input stamp when the frame in flight was enqueued
    uint64_t newest_stamp() const;
    void flush_published();
    int spin_once_deferred(cm_result* res);
    int collect_pending(cm_result* res);
    int collect_and_publish_async(cm_result* res);
    int spin_once_pipelined(cm_result* res);
    // what both paths do once a frame has been waited for, and to its message
    int after_wait(const cm_result& r);
    void shape_message(PointCloud2& msg, const cm_result& r, int st);
    void stamp_message(PointCloud2& msg, uint64_t input_stamp);
    std::vector<std::atomic<uint64_t>> stamp_ns_;   // stamp of the cloud each sensor slot currently holds
    // A slot holds a cloud no fuse has consumed yet when more submits were accepted for it than the last fuse had seen
    // (cm_frame_stats.generation): exact, whichever way a callback and the fuse interleave.
    std::vector<std::atomic<uint64_t>> submitted_, consumed_;
    bool fresh(size_t s) const { return submitted_[s].load() > consumed_[s].load(); }
    std::atomic<uint64_t> dropped_{0};
    // one lock per sensor: a callback's submit + bookkeeping and the loop thread's drop of that sensor's cloud (approximate
    // time synchronisation) exclude each other, so a cloud accepted in between is neither marked consumed nor loses its stamp
    std::vector<std::mutex> slot_mu_;
    // ego-motion compensation: the twist, and the stamp the frame enqueued last is expressed at (and published with)
    std::mutex twist_mu_;
    float twist_v_[3] = {0, 0, 0}, twist_w_[3] = {0, 0, 0};
    uint64_t motion_t_ref_ = 0;
    uint64_t n_clusters_ = 0;
    std::vector<uint32_t> cluster_labels_;
    std::vector<cm_cluster_box> cluster_boxes_;
    int clusters_of_frame(const cm_result& r);     // after cm_wait: cm_result_clusters (and the boxes) when the config asks for it
    std::vector<cm_grid_cell> grid_cells_;
    std::vector<int8_t> grid_occupancy_;
    std::vector<cm_grid_ray_cell> grid_ray_cells_;
    std::vector<int8_t> grid_cleared_;
    int grid_of_frame(const cm_result& r);         // after cm_wait: cm_result_grid_map and the image when the config asks for it
    std::mutex pose_mu_;
    float pose_[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<cm_map_cell> map_cells_;
    std::vector<int8_t> map_image_;
    cm_map_info map_info_{};
    std::vector<uint8_t> map_cost_;
    std::vector<uint32_t> map_dist2_;
    float goal_[2] = {0.0f, 0.0f};                 // (under pose_mu_)
    bool has_goal_ = false;
    std::vector<uint32_t> map_potential_, map_path_;
    cm_plan_info map_plan_info_{};
    cm_path_info map_path_info_{};
    std::vector<cm_frontier> frontiers_;
    cm_frontier_info frontier_info_{};
    std::vector<cm_traj_score> traj_scores_;
    cm_traj_info traj_info_{};
    bool matched_ = false;
    cm_match_result match_result_{};
    cm_match_search_info match_search_info_{};
    float matched_pose_[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    bool mcl_started_ = false;
    float mcl_prev_[3] = {0.0f, 0.0f, 0.0f};         // x, y, yaw of the set pose at the last init or predict
    cm_mcl_info mcl_info_{};
    cm_mcl_beam_info mcl_beam_info_{};
    std::vector<cm_mcl_hyp> mcl_hyp_;
    cm_mcl_hyp_info mcl_hyp_info_{};
    std::vector<cm_mcl_particle> mcl_particles_;
    std::vector<cm_cast_ray> cast_rays_;
    cm_cast_info cast_info_{};
    int map_of_frame(const cm_result& r);          // after cm_wait: cm_map_integrate and the two copies (the cost layer's update and its two) when the config asks for it
    std::vector<cm_voxel_normal> normals_;
    int normals_of_frame(const cm_result& r);      // after cm_wait: cm_result_normals when the config asks for it
    bool has_alignment_ = false;
    cm_align_result alignment_{};
    cm_ndt_result ndt_alignment_{};
    std::vector<float> prev_records_;              // the records published for the previous frame (16 bytes each)
    int align_of_frame(const cm_result& r);        // after cm_wait: cm_result_align of prev_records_ when the config asks for it
    int enqueue_frame(bool wait, cm_result* r);   // cm_merge_voxelize(_async), with the motion of the frame set under the slot locks
};

}  // namespace cloudmerge
