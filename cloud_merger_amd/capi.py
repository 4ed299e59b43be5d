"""ctypes binding of include/cloudmerge.h (libcloudmerge_hip.so).

This is plumbing for tests and bench.py: every call goes straight through the C-ABI. The library
is loaded from the in-tree build (cloud_merger_amd/lib/); a missing library is an error — there is
no Python or CPU fallback for the path.
"""
import ctypes as C
import os

import numpy as np

from .types import MergeParams, SensorCloud, XYZI_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libcloudmerge_hip.so")

MAX_SENSORS = 16
NO_FIELD = 0xFFFFFFFF
MAX_STAGES = 48

OK, EMPTY_INPUT, GRID_OVERFLOW, NOT_READY, SKIPPED = 0, 1, 2, 3, 4
BAD_ARG, HIP_ERROR, NO_DEVICE, CAPACITY, INTERNAL = -1, -2, -3, -4, -5
FLAG_PROFILE, FLAG_LATEST_WINS, FLAG_OCCUPANCY = 0x1, 0x2, 0x4
# cm_result.path_flags (CM_PATH_*)
PATH_LDS_RANK, PATH_BUCKET, PATH_PREDICTED, PATH_REDONE, PATH_PACKED, PATH_SPLIT, PATH_QUANTILE = 1, 2, 4, 8, 16, 32, 64
PATH_MOTION = 128
PATH_SOR = 256
SOR_MAX_K = 64
# per-point time field types of cm_set_sensor_time_field (CM_TIME_*)
TIME_NONE, TIME_F32_S, TIME_U32_NS = 0, 1, 2

# Every symbol include/cloudmerge.h declares (tests/test_capi_symbols.py checks both directions).
SYMBOLS = [
    "cm_create", "cm_destroy", "cm_set_stream", "cm_set_sensor_transform", "cm_set_sensor_matrix",
    "cm_get_sensor_matrix", "cm_submit_cloud", "cm_submit_cloud_device", "cm_clear_sensor",
    "cm_merge_voxelize", "cm_merge_voxelize_async", "cm_wait", "cm_result_copy", "cm_result_device",
    "cm_result_copy_cells", "cm_merged_copy", "cm_get_stage_times", "cm_status_string",
    "cm_last_error", "cm_version", "cm_host_alloc", "cm_host_free",
    "cm_local_bounds", "cm_merge_partial", "cm_partial_device", "cm_partial_copy", "cm_merge_tables",
    "cm_set_ground_removal", "cm_ground_copy", "cm_ground_planes",
    "cm_submit_cloud_async", "cm_result_copy_async", "cm_sync", "cm_get_frame_stats",
    "cm_result_publish_async", "cm_publish_wait", "cm_host_register", "cm_host_unregister",
    "cm_set_sensor_time_field", "cm_set_ego_motion",
    "cm_result_voxel_cov", "cm_result_voxel_cov_device",
    "cm_set_statistical_outlier", "cm_get_sor_stats", "cm_sor_distances_copy",
    "cm_result_clusters", "cm_result_clusters_device",
    "cm_box_directions", "cm_result_cluster_boxes", "cm_result_cluster_boxes_device",
    "cm_result_grid_map", "cm_result_grid_map_device", "cm_grid_occupancy_copy",
    "cm_result_grid_rays", "cm_result_grid_rays_device", "cm_grid_ray_occupancy_copy",
    "cm_map_configure", "cm_map_integrate", "cm_map_copy", "cm_map_device", "cm_map_occupancy_copy", "cm_map_load",
    "cm_map_cost_configure", "cm_map_cost_update", "cm_map_cost_copy", "cm_map_dist_copy", "cm_map_cost_device", "cm_map_cost_table_copy",
    "cm_map_plan_configure", "cm_map_plan_update", "cm_map_plan_copy", "cm_map_plan_device", "cm_map_plan_path",
    "cm_map_traj_configure", "cm_map_traj_evaluate", "cm_map_traj_copy", "cm_map_traj_device", "cm_traj_directions",
    "cm_map_frontier_configure", "cm_map_frontier_update", "cm_map_frontier_copy", "cm_map_frontier_labels_copy", "cm_map_frontier_device",
    "cm_map_match_configure", "cm_map_match_evaluate", "cm_map_match_copy", "cm_map_match_device", "cm_map_match_table_copy", "cm_match_table",
    "cm_map_match_search_configure", "cm_map_match_search", "cm_map_match_search_result", "cm_map_match_search_level_copy",
    "cm_map_mcl_configure", "cm_map_mcl_init_pose", "cm_map_mcl_init_uniform", "cm_map_mcl_predict", "cm_map_mcl_update", "cm_map_mcl_copy",
    "cm_map_mcl_weights_copy", "cm_map_mcl_device", "cm_mcl_draws", "cm_map_mcl_beam_configure", "cm_map_mcl_beam_info_copy", "cm_mcl_beam_table",
    "cm_map_mcl_hyp_configure", "cm_map_mcl_hyp_copy", "cm_mcl_kld_bound",
    "cm_map_cast_configure", "cm_map_cast_evaluate", "cm_map_cast_evaluate_mcl", "cm_map_cast_copy", "cm_map_cast_device", "cm_cast_directions",
    "cm_result_normals", "cm_result_normals_device",
    "cm_result_align", "cm_result_align_device", "cm_align_correspondences_copy",
    "cm_result_ndt_align", "cm_result_ndt_align_device", "cm_ndt_correspondences_copy",
]
MAX_ZONES = 8

# cm_partial_entry (32 bytes)
ENTRY_DTYPE = np.dtype([("key", "<u4"), ("count", "<u4"), ("sx", "<f4"), ("sy", "<f4"), ("sz", "<f4"),
                        ("si", "<f4"), ("_pad", "<u4", (2,))])
assert ENTRY_DTYPE.itemsize == 32


class Limits(C.Structure):
    _fields_ = [("max_sensors", C.c_uint32), ("flags", C.c_uint32), ("max_points_total", C.c_uint64)]


class Params(C.Structure):
    _fields_ = [("leaf", C.c_float * 3), ("min_points_per_voxel", C.c_uint32),
                ("downsample_all_data", C.c_int32), ("crop_enable", C.c_int32),
                ("crop_min", C.c_float * 3), ("crop_max", C.c_float * 3),
                ("required_sensor_mask", C.c_uint32), ("outlier_enable", C.c_int32),
                ("outlier_radius", C.c_float), ("outlier_min_neighbors", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_sensors", C.c_uint32), ("n_in", C.c_uint64),
                ("n_merged", C.c_uint64), ("n_out", C.c_uint64),
                ("min_b", C.c_int32 * 3), ("max_b", C.c_int32 * 3), ("div_b", C.c_int32 * 3),
                ("min_p", C.c_float * 3), ("max_p", C.c_float * 3),
                ("bounds_from_crop", C.c_uint32), ("key_bits", C.c_uint32), ("sort_passes", C.c_uint32),
                ("path_flags", C.c_uint32), ("device_ms", C.c_float)]


class Zone(C.Structure):
    _fields_ = [("x_min", C.c_float), ("x_length", C.c_float), ("z_max_ground", C.c_float)]


class GroundParams(C.Structure):
    _fields_ = [("max_iterations", C.c_uint32), ("distance_threshold", C.c_float), ("probability", C.c_float),
                ("optimize_coefficients", C.c_int32), ("z_keep_max", C.c_float), ("outlier_radius", C.c_float),
                ("outlier_min_neighbors", C.c_uint32), ("_pad", C.c_uint32), ("seed", C.c_uint64),
                ("n_zones", C.c_uint32 * MAX_SENSORS), ("zones", (Zone * MAX_ZONES) * MAX_SENSORS)]


class GroundPlane(C.Structure):
    _fields_ = [("plane", C.c_float * 4), ("band_points", C.c_uint32), ("inliers", C.c_uint32),
                ("iterations", C.c_uint32), ("found", C.c_int32)]


def make_ground_params(zones_per_sensor, max_iterations=1000, distance_threshold=0.3, probability=0.99,
                       optimize=True, z_keep_max=3.0, seed=12345, outlier_radius=0.0, outlier_min_neighbors=1):
    """zones_per_sensor: list (one entry per sensor) of lists of (x_min, x_length, z_max_ground); a negative
    z_max_ground keeps the slab whole. Defaults: the reference's Parameter.h:35-42."""
    g = GroundParams()
    g.max_iterations, g.distance_threshold, g.probability = max_iterations, distance_threshold, probability
    g.optimize_coefficients, g.z_keep_max, g.seed = int(optimize), z_keep_max, seed
    g.outlier_radius, g.outlier_min_neighbors = outlier_radius, outlier_min_neighbors
    for s, zs in enumerate(zones_per_sensor):
        g.n_zones[s] = len(zs)
        for k, (x0, ln, zm) in enumerate(zs):
            g.zones[s][k] = Zone(x0, ln, zm)
    return g


class Motion(C.Structure):
    """cm_motion: ego twist in the common frame, the reference instant and the header stamp of every slot's cloud."""
    _fields_ = [("v", C.c_float * 3), ("w", C.c_float * 3), ("t_ref_ns", C.c_int64), ("stamp_ns", C.c_int64 * MAX_SENSORS)]


def make_motion(v, w, t_ref_ns, stamp_ns):
    """stamp_ns: one stamp per sensor slot (a sequence, or a dict slot -> stamp); slots not named get t_ref_ns."""
    m = Motion()
    m.v = (C.c_float * 3)(*[float(x) for x in v])
    m.w = (C.c_float * 3)(*[float(x) for x in w])
    m.t_ref_ns = int(t_ref_ns)
    items = stamp_ns.items() if isinstance(stamp_ns, dict) else enumerate(stamp_ns)
    st = [int(t_ref_ns)] * MAX_SENSORS
    for s, t in items:
        st[int(s)] = int(t)
    m.stamp_ns = (C.c_int64 * MAX_SENSORS)(*st)
    return m


# per-voxel covariance (cm_result_voxel_cov): cm_voxel_cov.flags
COV_VALID, COV_INFLATED = 1, 2


class CovParams(C.Structure):
    _fields_ = [("min_points", C.c_uint32), ("eig_mult", C.c_float)]


class VoxelCov(C.Structure):
    """cm_voxel_cov (80 bytes): cov / icov hold (0,0) (1,0) (2,0) (1,1) (2,1) (2,2)."""
    _fields_ = [("mean", C.c_float * 3), ("count", C.c_uint32), ("cov", C.c_float * 6), ("icov", C.c_float * 6),
                ("evals", C.c_float * 3), ("flags", C.c_uint32)]


VOXEL_COV_DTYPE = np.dtype([("mean", "<f4", (3,)), ("count", "<u4"), ("cov", "<f4", (6,)), ("icov", "<f4", (6,)),
                            ("evals", "<f4", (3,)), ("flags", "<u4")])
assert VOXEL_COV_DTYPE.itemsize == C.sizeof(VoxelCov) == 80


# Euclidean cluster extraction on the result (cm_result_clusters)
CLUSTER_NONE = 0xFFFFFFFF


class ClusterParams(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("min_cluster_size", C.c_uint32), ("max_cluster_size", C.c_uint32), ("_pad", C.c_uint32)]


class Cluster(C.Structure):
    """cm_cluster (40 bytes): members at indices[first : first + n_voxels]; min / max: the box of their centroids."""
    _fields_ = [("first", C.c_uint32), ("n_voxels", C.c_uint32), ("n_points", C.c_uint32), ("_pad", C.c_uint32),
                ("min", C.c_float * 3), ("max", C.c_float * 3)]


CLUSTER_DTYPE = np.dtype([("first", "<u4"), ("n_voxels", "<u4"), ("n_points", "<u4"), ("_pad", "<u4"),
                          ("min", "<f4", (3,)), ("max", "<f4", (3,))])
assert CLUSTER_DTYPE.itemsize == C.sizeof(Cluster) == 40 and C.sizeof(ClusterParams) == 16

# oriented boxes of the clusters (cm_result_cluster_boxes)
BOX_MAX_ANGLES, BOX_CHUNK, BOX_MAX_EXTENT = 180, 256, 1.0e6
BOX_AREA, BOX_CLOSENESS = 0, 1
BOX_VALID = 1


class BoxParams(C.Structure):
    _fields_ = [("cluster", ClusterParams), ("n_angles", C.c_uint32), ("criterion", C.c_uint32), ("d_min", C.c_float),
                ("_pad", C.c_uint32)]


class ClusterBox(C.Structure):
    """cm_cluster_box (48 bytes): entry k belongs to cluster k; size along the heading, across it, height."""
    _fields_ = [("center", C.c_float * 3), ("size", C.c_float * 3), ("yaw", C.c_float), ("angle", C.c_uint32),
                ("score", C.c_double), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


BOX_DTYPE = np.dtype([("center", "<f4", (3,)), ("size", "<f4", (3,)), ("yaw", "<f4"), ("angle", "<u4"), ("score", "<f8"),
                      ("flags", "<u4"), ("_pad", "<u4")])
assert BOX_DTYPE.itemsize == C.sizeof(ClusterBox) == 48 and C.sizeof(BoxParams) == 32

# 2-D grid map of the frame (cm_result_grid_map)
GRID_MAX_CELLS = 1 << 22
GRID_UNKNOWN, GRID_FREE, GRID_OCCUPIED = 0, 1, 2


class GridParams(C.Structure):
    _fields_ = [("origin", C.c_float * 2), ("cell", C.c_float), ("nx", C.c_uint32), ("ny", C.c_uint32), ("z_min", C.c_float),
                ("z_max", C.c_float), ("obstacle_height", C.c_float), ("min_points", C.c_uint32)]


class GridCell(C.Structure):
    """cm_grid_cell (32 bytes): cell (ix, iy) is entry ix + iy * nx."""
    _fields_ = [("n", C.c_uint32), ("n_ground", C.c_uint32), ("z_lo", C.c_float), ("z_hi", C.c_float), ("g_lo", C.c_float),
                ("g_hi", C.c_float), ("i_max", C.c_float), ("state", C.c_uint32)]


GRID_DTYPE = np.dtype([("n", "<u4"), ("n_ground", "<u4"), ("z_lo", "<f4"), ("z_hi", "<f4"), ("g_lo", "<f4"), ("g_hi", "<f4"),
                       ("i_max", "<f4"), ("state", "<u4")])
assert GRID_DTYPE.itemsize == C.sizeof(GridCell) == 32 and C.sizeof(GridParams) == 36


# free-space ray casting over the grid map (cm_result_grid_rays)
class RayParams(C.Structure):
    """cm_ray_params: min_pass (>= 1), max_range_cells (0: to the end cell)."""
    _fields_ = [("min_pass", C.c_uint32), ("max_range_cells", C.c_uint32)]


class GridRayCell(C.Structure):
    """cm_grid_ray_cell (8 bytes): cell (ix, iy) is entry ix + iy * nx."""
    _fields_ = [("n_pass", C.c_uint32), ("n_end", C.c_uint32)]


RAY_DTYPE = np.dtype([("n_pass", "<u4"), ("n_end", "<u4")])
assert RAY_DTYPE.itemsize == C.sizeof(GridRayCell) == 8 and C.sizeof(RayParams) == 8


# rolling log-odds occupancy map accumulated over frames (cm_map_configure, cm_map_integrate)
MAP_MAX_LOGODDS = 1 << 20


class MapParams(C.Structure):
    """cm_map_params (48 bytes): the window, the height band (vehicle frame), the log-odds steps, clamps and image thresholds."""
    _fields_ = [("cell", C.c_float), ("nx", C.c_uint32), ("ny", C.c_uint32), ("z_min", C.c_float), ("z_max", C.c_float),
                ("l_hit", C.c_int32), ("l_miss", C.c_int32), ("l_min", C.c_int32), ("l_max", C.c_int32), ("l_free", C.c_int32),
                ("l_occ", C.c_int32), ("max_range_cells", C.c_uint32)]


class MapCell(C.Structure):
    """cm_map_cell (8 bytes): window cell (ix, iy) is entry ix + iy * nx."""
    _fields_ = [("logodds", C.c_int32), ("n_obs", C.c_uint32)]


class MapInfo(C.Structure):
    """cm_map_info (32 bytes): the window's anchor (absolute cell of window cell (0, 0)) and size, the integrations since the
    configure call, the descriptor sensors that cast rays in the last one (a bit mask)."""
    _fields_ = [("anchor", C.c_int32 * 2), ("nx", C.c_uint32), ("ny", C.c_uint32), ("n_frames", C.c_uint64),
                ("sensors_cast", C.c_uint32), ("_pad", C.c_uint32)]


MAP_DTYPE = np.dtype([("logodds", "<i4"), ("n_obs", "<u4")])
assert MAP_DTYPE.itemsize == C.sizeof(MapCell) == 8 and C.sizeof(MapParams) == 48 and C.sizeof(MapInfo) == 32

# cost layer over the occupancy map: exact distance field and inflated costmap (cm_map_cost_configure, cm_map_cost_update)
MAP_DIST_NONE = 0xFFFFFFFF
COST_LETHAL = 254
COST_INSCRIBED = 253
COST_NO_INFORMATION = 255
COST_INFLATE_UNKNOWN = 1
COST_MAX_RADIUS_CELLS = 256
COST_MAX_AXIS = 2048


class CostParams(C.Structure):
    """cm_cost_params (16 bytes): the two radii in metres, the decay per metre, CM_COST_INFLATE_UNKNOWN or 0."""
    _fields_ = [("inscribed_radius", C.c_float), ("inflation_radius", C.c_float), ("cost_scaling", C.c_float), ("flags", C.c_uint32)]


assert C.sizeof(CostParams) == 16

# plan layer behind the cost layer: navigation function and path extraction (cm_map_plan_configure, cm_map_plan_update, cm_map_plan_path)
PLAN_UNREACHABLE = 0xFFFFFFFF
PLAN_ALLOW_UNKNOWN = 1
PATH_FOUND = 0
PATH_UNREACHABLE = 1
PATH_TRUNCATED = 2


class PlanParams(C.Structure):
    """cm_plan_params (16 bytes): neutral 1..255, the cost byte's factor in 1/256 (0..256), CM_PLAN_ALLOW_UNKNOWN or 0, the longest
    path in cells."""
    _fields_ = [("neutral", C.c_uint32), ("cost_factor_q8", C.c_uint32), ("flags", C.c_uint32), ("max_path_cells", C.c_uint32)]


class PlanInfo(C.Structure):
    """cm_plan_info (16 bytes): the goal's window cell and the number of sweeps of the last update."""
    _fields_ = [("goal", C.c_uint32 * 2), ("n_sweeps", C.c_uint32), ("_pad", C.c_uint32)]


class PathInfo(C.Structure):
    """cm_path_info (32 bytes): the start's and the goal's window cells, the cells written, PATH_FOUND / PATH_UNREACHABLE /
    PATH_TRUNCATED, pot(start)."""
    _fields_ = [("start", C.c_uint32 * 2), ("goal", C.c_uint32 * 2), ("n_cells", C.c_uint32), ("status", C.c_uint32),
                ("pot_start", C.c_uint32), ("_pad", C.c_uint32)]


assert C.sizeof(PlanParams) == 16 and C.sizeof(PlanInfo) == 16 and C.sizeof(PathInfo) == 32

# rollout layer behind the plan layer: sampled velocity commands scored over cost and pot (cm_map_traj_configure, cm_map_traj_evaluate)
TRAJ_MAX_SAMPLES = 16384
TRAJ_MAX_STEPS = 256
TRAJ_MAX_FOOT = 256
TRAJ_HEADINGS = 4096
TRAJ_ALLOW_UNKNOWN = 1
TRAJ_NONE = 0xFFFFFFFF
TRAJ_VALID = 0
TRAJ_COLLISION = 1
TRAJ_OFF_MAP = 2
TRAJ_NO_POTENTIAL = 3


class TrajParams(C.Structure):
    """cm_traj_params (24 bytes): the sample counts nv x nw (at most TRAJ_MAX_SAMPLES together), the steps of a rollout
    (1..TRAJ_MAX_STEPS), the two weights of the total, CM_TRAJ_ALLOW_UNKNOWN or 0."""
    _fields_ = [("nv", C.c_uint32), ("nw", C.c_uint32), ("n_steps", C.c_uint32), ("occ_scale", C.c_uint32), ("goal_scale", C.c_uint32),
                ("flags", C.c_uint32)]


class TrajWindow(C.Structure):
    """cm_traj_window (32 bytes): the start pose (x, y, yaw), the velocity window v_lo..v_hi and w_lo..w_hi, dt per step."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("yaw", C.c_float), ("v_lo", C.c_float), ("v_hi", C.c_float), ("w_lo", C.c_float),
                ("w_hi", C.c_float), ("dt", C.c_float)]


class TrajScore(C.Structure):
    """cm_traj_score (32 bytes): TRAJ_VALID / TRAJ_COLLISION / TRAJ_OFF_MAP / TRAJ_NO_POTENTIAL, the pose that ended the
    trajectory, the largest cost byte met, pot at the end, the total, the last (or the bad) pose's centre."""
    _fields_ = [("status", C.c_uint32), ("bad_step", C.c_uint32), ("occ", C.c_uint32), ("pot_end", C.c_uint32), ("total", C.c_uint64),
                ("end_x", C.c_float), ("end_y", C.c_float)]


class TrajInfo(C.Structure):
    """cm_traj_info (24 bytes): the best entry (TRAJ_NONE: no valid one), the number of valid entries, the best entry's
    command, the start's window cell."""
    _fields_ = [("best", C.c_uint32), ("n_valid", C.c_uint32), ("best_v", C.c_float), ("best_w", C.c_float), ("start", C.c_uint32 * 2)]


TRAJ_SCORE_DTYPE = np.dtype([("status", "<u4"), ("bad_step", "<u4"), ("occ", "<u4"), ("pot_end", "<u4"), ("total", "<u8"),
                             ("end_x", "<f4"), ("end_y", "<f4")])
assert C.sizeof(TrajParams) == 24 and C.sizeof(TrajWindow) == 32 and C.sizeof(TrajScore) == 32 == TRAJ_SCORE_DTYPE.itemsize and C.sizeof(TrajInfo) == 24

# frontier layer behind the plan layer: connected frontiers of the occupancy map (cm_map_frontier_configure, cm_map_frontier_update)
FRONTIER_NONE = 0xFFFFFFFF
FRONTIER_MAX_TABLE = 1 << 16


class FrontierParams(C.Structure):
    """cm_frontier_params (20 bytes): the smallest component that is a frontier (>= 1), the table's entries
    (1..FRONTIER_MAX_TABLE), the largest cost byte of a frontier cell (0..252), the two weights of the score."""
    _fields_ = [("min_cells", C.c_uint32), ("max_frontiers", C.c_uint32), ("max_cost", C.c_uint32), ("pot_scale", C.c_uint32),
                ("gain_scale", C.c_uint32)]


class Frontier(C.Structure):
    """cm_frontier (40 bytes): the smallest cell and the cell count, the sums of ix and iy, the smallest pot and the lowest cell
    that has it (PLAN_UNREACHABLE and FRONTIER_NONE: none reachable), the closed bounding box."""
    _fields_ = [("first_cell", C.c_uint32), ("n_cells", C.c_uint32), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64),
                ("min_pot", C.c_uint32), ("min_pot_cell", C.c_uint32), ("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16),
                ("y1", C.c_uint16)]


class FrontierInfo(C.Structure):
    """cm_frontier_info (32 bytes): frontier cells, components, frontiers, table entries written, the best entry
    (FRONTIER_NONE: none) and its score."""
    _fields_ = [("n_frontier_cells", C.c_uint32), ("n_components", C.c_uint32), ("n_frontiers", C.c_uint32), ("n_written", C.c_uint32),
                ("best", C.c_uint32), ("_pad", C.c_uint32), ("best_score", C.c_int64)]


FRONTIER_DTYPE = np.dtype([("first_cell", "<u4"), ("n_cells", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("min_pot", "<u4"),
                           ("min_pot_cell", "<u4"), ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")])
assert C.sizeof(FrontierParams) == 20 and C.sizeof(Frontier) == 40 == FRONTIER_DTYPE.itemsize and C.sizeof(FrontierInfo) == 32

# scan matching of the frame against the occupancy map, behind the cost layer (cm_map_match_configure, cm_map_match_evaluate)
MATCH_MAX_RADIUS_CELLS = 64
MATCH_MAX_SHIFT = 64
MATCH_MAX_ANGLES = 127
MATCH_MAX_CANDIDATES = 1 << 22
MATCH_SUBCELL = 1


class MatchParams(C.Structure):
    """cm_match_params (28 bytes): the field's sigma and cut (metres), angle candidates -n_a..n_a at a_stride heading-table
    entries, shifts -wx..wx and -wy..wy cells, MATCH_SUBCELL or 0."""
    _fields_ = [("sigma", C.c_float), ("max_dist", C.c_float), ("n_a", C.c_uint32), ("a_stride", C.c_uint32), ("wx", C.c_uint32),
                ("wy", C.c_uint32), ("flags", C.c_uint32)]


class MatchResult(C.Structure):
    """cm_match_result (96 bytes): the best entry, its angle candidate and shift, its score, the cells of that candidate and
    255 times their number, the candidate's rotation, the sub-cell offsets, the matched pose (3 x 4, row-major)."""
    _fields_ = [("best", C.c_uint32), ("k", C.c_int32), ("i", C.c_int32), ("j", C.c_int32), ("score", C.c_uint32), ("n_cells", C.c_uint32),
                ("max_score", C.c_uint32), ("yaw", C.c_float), ("sub", C.c_double * 2), ("pose", C.c_float * 12)]


assert C.sizeof(MatchParams) == 28 and C.sizeof(MatchResult) == 96 and MatchResult.sub.offset == 32 and MatchResult.pose.offset == 48

# branch-and-bound scan matching over wide windows, the search layer behind the cost layer (cm_map_match_search_configure, cm_map_match_search)
MATCH_SEARCH_MAX_SHIFT = 1024
MATCH_SEARCH_MAX_DEPTH = 7
MATCH_SEARCH_MAX_NODES = 1 << 22
MATCH_SEARCH_OVERFLOW_CELLS = -2


class MatchSearchParams(C.Structure):
    """cm_match_search_params (40 bytes): MatchParams' sigma, max_dist, n_a, a_stride, shifts -wx..wx and -wy..wy cells of up to
    MATCH_SEARCH_MAX_SHIFT, the roots' level, the room of a level's node list and of a candidate's cell list, MATCH_SUBCELL or 0."""
    _fields_ = [("sigma", C.c_float), ("max_dist", C.c_float), ("n_a", C.c_uint32), ("a_stride", C.c_uint32), ("wx", C.c_uint32),
                ("wy", C.c_uint32), ("depth", C.c_uint32), ("max_nodes", C.c_uint32), ("max_cells", C.c_uint32), ("flags", C.c_uint32)]


class MatchSearchInfo(C.Structure):
    """cm_match_search_info (84 bytes): depth, the number of roots, the bound B, per level the nodes scored in the level loop and
    those kept, the nodes scored for B beyond the roots, and the level whose node list overflowed (-1: none,
    MATCH_SEARCH_OVERFLOW_CELLS: a candidate's cell list)."""
    _fields_ = [("depth", C.c_uint32), ("n_roots", C.c_uint32), ("bound", C.c_uint32), ("scored", C.c_uint32 * 8), ("live", C.c_uint32 * 8),
                ("n_probe", C.c_uint32), ("overflow_level", C.c_int32)]


assert C.sizeof(MatchSearchParams) == 40 and C.sizeof(MatchSearchInfo) == 84

# the localisation layer: a particle filter against the occupancy map, behind the cost layer (cm_map_mcl_configure, cm_map_mcl_update)
MCL_MAX_PARTICLES = 65536
MCL_MAX_BEAMS = 8192
MCL_MAX_RANGE_CELLS = 1024
MCL_WEIGHT_ONE = 65536
MCL_RESAMPLE_ALWAYS = 1


class MclParams(C.Structure):
    """cm_mcl_params (40 bytes): the particles, the most beams of an update and the reach of a beam in body cells, the field's
    sigma and cut (metres) as MatchParams', the temperature of the weights, the fraction of n_particles below which n_eff
    triggers resampling, MCL_RESAMPLE_ALWAYS or 0, the seed of the draws."""
    _fields_ = [("n_particles", C.c_uint32), ("max_beams", C.c_uint32), ("range_cells", C.c_uint32), ("sigma", C.c_float), ("max_dist", C.c_float),
                ("tau", C.c_float), ("resample_frac", C.c_float), ("flags", C.c_uint32), ("seed", C.c_uint64)]


class MclInfo(C.Structure):
    """cm_mcl_info (176 bytes): the particles, the distinct body cells, the stride and the beams of the update, its gen, whether
    it resampled, the best particle and its pose before resampling, the exact integer sums, n_eff, the weighted means and the
    three spread terms (m^2)."""
    _fields_ = [("n_particles", C.c_uint32), ("n_cells", C.c_uint32), ("stride", C.c_uint32), ("n_beams", C.c_uint32), ("gen", C.c_uint64),
                ("resampled", C.c_uint32), ("best", C.c_uint32), ("best_x", C.c_float), ("best_y", C.c_float), ("best_h", C.c_uint32),
                ("_pad", C.c_uint32), ("sum_w", C.c_uint64), ("sum_w2", C.c_uint64), ("sum_wqx", C.c_int64), ("sum_wqy", C.c_int64),
                ("sum_wc", C.c_int64), ("sum_ws", C.c_int64), ("sum_wdxx", C.c_int64), ("sum_wdyy", C.c_int64), ("sum_wdxy", C.c_int64),
                ("n_eff", C.c_double), ("mean_x", C.c_double), ("mean_y", C.c_double), ("mean_yaw", C.c_double), ("var_xx", C.c_double),
                ("var_yy", C.c_double), ("var_xy", C.c_double)]


MCL_PARTICLE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("h", "<u4"), ("parent", "<u4"), ("acc", "<u8")])
MCL_WEIGHT_DTYPE = np.dtype([("score", "<u4"), ("weight", "<u4")])
assert C.sizeof(MclParams) == 40 and MclParams.seed.offset == 32 and C.sizeof(MclInfo) == 176 and MclInfo.sum_w.offset == 48
assert MclInfo.n_eff.offset == 120 and MCL_PARTICLE_DTYPE.itemsize == 24 and MCL_WEIGHT_DTYPE.itemsize == 8

# the beam model of the localisation layer: rays cast per beam (cm_map_mcl_beam_configure)
MCL_BEAM_MAX_OVER = 64
MCL_BEAM_MAX_D = 1450
MCL_BEAM_PLAIN = 1


class MclBeamParams(C.Structure):
    """cm_mcl_beam_params (24 bytes): how many cells past its measured end a ray is followed, the hit term's sigma (metres), the
    weights of the hit, short and random terms (their sum at most 1), MCL_BEAM_PLAIN or 0."""
    _fields_ = [("over_cells", C.c_uint32), ("sigma", C.c_float), ("z_hit", C.c_float), ("z_short", C.c_float), ("z_rand", C.c_float),
                ("flags", C.c_uint32)]


class MclBeamInfo(C.Structure):
    """cm_mcl_beam_info (56 bytes): the rays of the update (n_particles * n_beams) and how they ended: an occupied cell before,
    at or after the measured end, none within reach, off the window, or not cast at all."""
    _fields_ = [("n_rays", C.c_uint64), ("n_early", C.c_uint64), ("n_at", C.c_uint64), ("n_late", C.c_uint64), ("n_beyond", C.c_uint64),
                ("n_off", C.c_uint64), ("n_skipped", C.c_uint64)]


assert C.sizeof(MclBeamParams) == 24 and MclBeamParams.flags.offset == 20 and C.sizeof(MclBeamInfo) == 56

# pose hypotheses and random-particle recovery of the localisation layer (cm_map_mcl_hyp_configure)
MCL_HYP_MAX = 64
MCL_NO_PARENT = 0xFFFFFFFF


class MclHypParams(C.Structure):
    """cm_mcl_hyp_params (40 bytes): the bin width in 1/1024 m and the bits of the heading bins, the most hypotheses reported,
    the most particles one update may inject (0: none), the rates of the slow and the fast average of the score, the error and
    the quantile of the KLD bound, flags and padding (0)."""
    _fields_ = [("bin_q", C.c_uint32), ("heading_bits", C.c_uint32), ("max_hyp", C.c_uint32), ("inject_max", C.c_uint32), ("alpha_slow", C.c_float),
                ("alpha_fast", C.c_float), ("kld_err", C.c_float), ("kld_z", C.c_float), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class MclHyp(C.Structure):
    """cm_mcl_hyp (136 bytes): one connected component of the occupied bins: its smallest key, its particles and the heaviest
    of them, the integer sums of the estimate over its particles, its share of the total weight and its mean and spread."""
    _fields_ = [("label", C.c_uint64), ("n", C.c_uint32), ("top", C.c_uint32), ("sum_w", C.c_uint64), ("sum_wqx", C.c_int64), ("sum_wqy", C.c_int64),
                ("sum_wc", C.c_int64), ("sum_ws", C.c_int64), ("sum_wdxx", C.c_int64), ("sum_wdyy", C.c_int64), ("sum_wdxy", C.c_int64),
                ("share", C.c_double), ("mean_x", C.c_double), ("mean_y", C.c_double), ("mean_yaw", C.c_double), ("var_xx", C.c_double),
                ("var_yy", C.c_double), ("var_xy", C.c_double)]


class MclHypInfo(C.Structure):
    """cm_mcl_hyp_info (72 bytes): the update's gen, the occupied bins, their components, the hypotheses reported, the KLD bound
    for that many bins, the particles injected, the free cells they were drawn from, the sum of the scores, their average, its
    slow and fast average and the share of the particles the recovery asked for."""
    _fields_ = [("gen", C.c_uint64), ("n_bins", C.c_uint32), ("n_components", C.c_uint32), ("n_hyp", C.c_uint32), ("n_kld", C.c_uint32),
                ("n_inject", C.c_uint32), ("n_free", C.c_uint32), ("sum_s", C.c_uint64), ("w_avg", C.c_double), ("w_slow", C.c_double),
                ("w_fast", C.c_double), ("p_inject", C.c_double)]


assert C.sizeof(MclHypParams) == 40 and C.sizeof(MclHyp) == 136 and MclHyp.share.offset == 80 and C.sizeof(MclHypInfo) == 72

# the cast layer: expected ranges from many poses in the map, behind the cost layer (cm_map_cast_configure, cm_map_cast_evaluate)
CAST_MAX_POSES = 65536
CAST_MAX_BEARINGS = 4096
CAST_MAX_RANGE_CELLS = 1024
CAST_MAX_RAYS = 1 << 24
CAST_PLAIN = 1
CAST_MAX, CAST_HIT, CAST_OFF_MAP, CAST_NO_ORIGIN = 0, 1, 2, 3            # status values of a ray, not bits


class CastParams(C.Structure):
    """cm_cast_params (16 bytes): the most poses of an evaluate, the bearings per pose, the reach of a ray in cells, CAST_PLAIN or 0."""
    _fields_ = [("max_poses", C.c_uint32), ("n_bearings", C.c_uint32), ("range_cells", C.c_uint32), ("flags", C.c_uint32)]


class CastInfo(C.Structure):
    """cm_cast_info (24 bytes): the poses and bearings of the last evaluate and its rays by status."""
    _fields_ = [("n_poses", C.c_uint32), ("n_bearings", C.c_uint32), ("n_max", C.c_uint32), ("n_hit", C.c_uint32), ("n_off_map", C.c_uint32),
                ("n_no_origin", C.c_uint32)]


CAST_POSE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("h", "<u4")])
CAST_RAY_DTYPE = np.dtype([("k", "<u2"), ("status", "u1"), ("_pad", "u1"), ("jx", "<i2"), ("jy", "<i2")])
assert C.sizeof(CastParams) == 16 and C.sizeof(CastInfo) == 24 and CAST_POSE_DTYPE.itemsize == 12 and CAST_RAY_DTYPE.itemsize == 8


# normals and curvature of the result (cm_result_normals)
NORMAL_MAX_K = 64
NORMAL_VALID = 1


class NormalParams(C.Structure):
    _fields_ = [("k", C.c_uint32), ("viewpoint", C.c_float * 3), ("search_cell", C.c_float), ("_pad", C.c_uint32)]


VOXEL_NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("curvature", "<f4"), ("r2_k", "<f4"), ("n_neighbors", "<u4"),
                               ("last", "<u4"), ("flags", "<u4")])
assert VOXEL_NORMAL_DTYPE.itemsize == 32 and C.sizeof(NormalParams) == 24


# registration of a cloud against the result (cm_result_align)
ALIGN_MAX_ITER = 64
ALIGN_NONE = 0xFFFFFFFF
ALIGN_PIVOT_MIN = 1e-9
ALIGN_CONVERGED, ALIGN_MAX_ITER_HIT, ALIGN_FEW, ALIGN_SINGULAR = 1, 2, 4, 8


class AlignParams(C.Structure):
    _fields_ = [("max_corr_dist", C.c_float), ("max_iterations", C.c_uint32), ("normals_k", C.c_uint32),
                ("min_correspondences", C.c_uint32), ("trans_eps", C.c_double), ("rot_eps", C.c_double), ("guess", C.c_double * 12)]


class AlignResult(C.Structure):
    _fields_ = [("pose", C.c_double * 12), ("H", C.c_double * 21), ("g", C.c_double * 6), ("sse", C.c_double), ("rms", C.c_double),
                ("pivot", C.c_double * 3), ("n_corr", C.c_uint64), ("iterations", C.c_uint32), ("flags", C.c_uint32)]

    def pose_matrix(self):
        """(3, 4) float64 [R|t]."""
        return np.array(self.pose[:], np.float64).reshape(3, 4)


ALIGN_CORR_DTYPE = np.dtype([("idx", "<u4"), ("d2", "<f4")])
assert C.sizeof(AlignParams) == 128 and C.sizeof(AlignResult) == 368 and ALIGN_CORR_DTYPE.itemsize == 8


# NDT registration of a cloud against the covariance table (cm_result_ndt_align)
NDT_MAX_ITER = 64
NDT_NONE = 0xFFFFFFFF
NDT_CONVERGED, NDT_MAX_ITER_HIT, NDT_FEW, NDT_SINGULAR = 1, 2, 4, 8


class NdtParams(C.Structure):
    _fields_ = [("outlier_ratio", C.c_float), ("neighborhood", C.c_uint32), ("max_iterations", C.c_uint32),
                ("min_correspondences", C.c_uint32), ("cov", CovParams), ("trans_eps", C.c_double), ("rot_eps", C.c_double),
                ("guess", C.c_double * 12)]


class NdtResult(C.Structure):
    _fields_ = [("pose", C.c_double * 12), ("H", C.c_double * 21), ("g", C.c_double * 6), ("score", C.c_double),
                ("gauss_d1", C.c_double), ("gauss_d2", C.c_double), ("pivot", C.c_double * 3), ("n_corr", C.c_uint64),
                ("iterations", C.c_uint32), ("flags", C.c_uint32)]

    def pose_matrix(self):
        """(3, 4) float64 [R|t]."""
        return np.array(self.pose[:], np.float64).reshape(3, 4)


NDT_CORR_DTYPE = np.dtype([("idx", "<u4"), ("n_used", "<u4"), ("score", "<f8")])
assert C.sizeof(NdtParams) == 136 and C.sizeof(NdtResult) == 376 and NDT_CORR_DTYPE.itemsize == 16


def sym6_to_3x3(a):
    """(..., 6) lower-triangle entries in cm_voxel_cov order -> (..., 3, 3) symmetric matrices."""
    a = np.asarray(a)
    m = np.empty(a.shape[:-1] + (3, 3), dtype=a.dtype)
    for q, (i, j) in enumerate(((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))):
        m[..., i, j] = a[..., q]
        m[..., j, i] = a[..., q]
    return m


class SorParams(C.Structure):
    """cm_sor_params: pcl::StatisticalOutlierRemoval's setMeanK / setStddevMulThresh and the search grid's cell (0: auto)."""
    _fields_ = [("mean_k", C.c_uint32), ("std_mul", C.c_float), ("search_cell", C.c_float), ("_pad", C.c_uint32)]


class SorStats(C.Structure):
    _fields_ = [("n_valid", C.c_uint64), ("n_removed", C.c_uint64), ("mean", C.c_double), ("stddev", C.c_double),
                ("threshold", C.c_double)]


class FrameStats(C.Structure):
    _fields_ = [("n_sensors", C.c_uint32), ("_pad", C.c_uint32), ("sensor", C.c_uint32 * MAX_SENSORS),
                ("n_in", C.c_uint32 * MAX_SENSORS), ("n_kept", C.c_uint32 * MAX_SENSORS), ("fresh", C.c_uint32 * MAX_SENSORS),
                ("generation", C.c_uint64 * MAX_SENSORS), ("bytes_h2d", C.c_uint64 * MAX_SENSORS), ("bytes_h2d_total", C.c_uint64), ("bytes_d2h_total", C.c_uint64),
                ("bytes_algorithmic", C.c_uint64)]


class StageTimes(C.Structure):
    _fields_ = [("n_stages", C.c_uint32), ("_pad", C.c_uint32),
                ("name", (C.c_char * 24) * MAX_STAGES), ("ms", C.c_float * MAX_STAGES)]


class CloudMergeError(RuntimeError):
    def __init__(self, status, what=""):
        super().__init__(f"{status_string(status)} ({status}) {what}".strip())
        self.status = status


_lib = None


def load():
    """Load the in-tree HIP library; raises if it has not been built.

    A process that also uses PyTorch must `import torch` BEFORE this is called: torch bundles its
    own libamdhip64/libhsa-runtime64, and the first HIP runtime loaded serves the whole process
    (same soname). Loaded the other way round torch finds no GPU."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if os.environ.get("CM_LIB_VARIANT") == "testhooks":      # the test build (python -m cloud_merger_amd.build --test-hooks)
        path = os.path.join(HERE, "lib", "libcloudmerge_hip_testhooks.so")
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: build it with `python -m cloud_merger_amd.build` "
                      "(the path has no fallback implementation)")
    L = C.CDLL(path)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.cm_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Limits)]
    L.cm_destroy.argtypes = [vp]
    L.cm_set_stream.argtypes = [vp, vp]
    L.cm_set_sensor_transform.argtypes = [vp, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.cm_set_sensor_matrix.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.cm_get_sensor_matrix.argtypes = [vp, u32, C.POINTER(C.c_float)]
    L.cm_submit_cloud.argtypes = [vp, u32, vp, u32, u32, u32, u32, u32, u32]
    L.cm_submit_cloud_device.argtypes = [vp, u32, vp, u32, u32, u32, u32, u32, u32]
    L.cm_result_publish_async.argtypes = [vp, vp, u64, u32]
    L.cm_publish_wait.argtypes = [vp]
    L.cm_host_register.argtypes = [vp, C.c_size_t]
    L.cm_host_unregister.argtypes = [vp]
    L.cm_submit_cloud_async.argtypes = [vp, u32, vp, u32, u32, u32, u32, u32, u32]
    L.cm_result_copy_async.argtypes = [vp, vp, u64]
    L.cm_sync.argtypes = [vp]
    L.cm_get_frame_stats.argtypes = [vp, C.POINTER(FrameStats)]
    L.cm_clear_sensor.argtypes = [vp, u32]
    L.cm_merge_voxelize.argtypes = [vp, C.POINTER(Params), C.POINTER(Result)]
    L.cm_merge_voxelize_async.argtypes = [vp, C.POINTER(Params)]
    L.cm_wait.argtypes = [vp, C.POINTER(Result)]
    L.cm_result_copy.argtypes = [vp, vp, u64, u32]
    L.cm_result_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.cm_result_copy_cells.argtypes = [vp, vp, vp, u64]
    L.cm_merged_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_get_stage_times.argtypes = [vp, C.POINTER(StageTimes)]
    L.cm_status_string.argtypes = [C.c_int]
    L.cm_status_string.restype = C.c_char_p
    L.cm_last_error.argtypes = [vp]
    L.cm_last_error.restype = C.c_char_p
    L.cm_version.argtypes = []
    L.cm_local_bounds.argtypes = [vp, C.POINTER(Params), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(u64)]
    L.cm_merge_partial.argtypes = [vp, C.POINTER(Params), C.POINTER(C.c_float), C.POINTER(Result)]
    L.cm_partial_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    L.cm_partial_copy.argtypes = [vp, vp, u64]
    L.cm_merge_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), u32, C.POINTER(Params), C.POINTER(Result)]
    L.cm_set_ground_removal.argtypes = [vp, C.POINTER(GroundParams)]
    L.cm_ground_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_ground_planes.argtypes = [vp, C.POINTER(GroundPlane), u32]
    L.cm_host_alloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.cm_host_free.argtypes = [vp]
    L.cm_set_sensor_time_field.argtypes = [vp, u32, u32, u32]
    L.cm_set_ego_motion.argtypes = [vp, C.POINTER(Motion)]
    L.cm_set_statistical_outlier.argtypes = [vp, C.POINTER(SorParams)]
    L.cm_get_sor_stats.argtypes = [vp, C.POINTER(SorStats)]
    L.cm_sor_distances_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_result_voxel_cov.argtypes = [vp, C.POINTER(CovParams), vp, u64]
    L.cm_result_voxel_cov_device.argtypes = [vp, C.POINTER(CovParams), C.POINTER(vp), C.POINTER(u64)]
    L.cm_result_clusters.argtypes = [vp, C.POINTER(ClusterParams), vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.cm_result_clusters_device.argtypes = [vp, C.POINTER(ClusterParams), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                            C.POINTER(u64), C.POINTER(u64)]
    L.cm_box_directions.argtypes = [u32, vp, u64]
    L.cm_result_cluster_boxes.argtypes = [vp, C.POINTER(BoxParams), vp, u64, C.POINTER(u64)]
    L.cm_result_cluster_boxes_device.argtypes = [vp, C.POINTER(BoxParams), C.POINTER(vp), C.POINTER(u64)]
    L.cm_result_grid_map.argtypes = [vp, C.POINTER(GridParams), vp, u64]
    L.cm_result_grid_map_device.argtypes = [vp, C.POINTER(GridParams), C.POINTER(vp), C.POINTER(u64)]
    L.cm_grid_occupancy_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_result_grid_rays.argtypes = [vp, C.POINTER(GridParams), C.POINTER(RayParams), vp, u64]
    L.cm_result_grid_rays_device.argtypes = [vp, C.POINTER(GridParams), C.POINTER(RayParams), C.POINTER(vp), C.POINTER(u64)]
    L.cm_grid_ray_occupancy_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_map_configure.argtypes = [vp, C.POINTER(MapParams)]
    L.cm_map_integrate.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(MapInfo)]
    L.cm_map_copy.argtypes = [vp, vp, u64, C.POINTER(MapInfo)]
    L.cm_map_device.argtypes = [vp, C.POINTER(vp), C.POINTER(MapInfo)]
    L.cm_map_occupancy_copy.argtypes = [vp, vp, u64, C.POINTER(MapInfo)]
    L.cm_map_cost_configure.argtypes = [vp, C.POINTER(CostParams)]
    L.cm_map_cost_update.argtypes = [vp, C.POINTER(MapInfo)]
    L.cm_map_cost_copy.argtypes = [vp, vp, u64, C.POINTER(MapInfo)]
    L.cm_map_dist_copy.argtypes = [vp, vp, u64, C.POINTER(MapInfo)]
    L.cm_map_cost_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(MapInfo)]
    L.cm_map_cost_table_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_map_plan_configure.argtypes = [vp, C.POINTER(PlanParams)]
    L.cm_map_plan_update.argtypes = [vp, C.c_float, C.c_float, C.POINTER(PlanInfo), C.POINTER(MapInfo)]
    L.cm_map_plan_copy.argtypes = [vp, vp, u64, C.POINTER(PlanInfo), C.POINTER(MapInfo)]
    L.cm_map_plan_device.argtypes = [vp, C.POINTER(vp), C.POINTER(PlanInfo), C.POINTER(MapInfo)]
    L.cm_map_plan_path.argtypes = [vp, C.c_float, C.c_float, vp, u64, C.POINTER(PathInfo)]
    L.cm_map_traj_configure.argtypes = [vp, C.POINTER(TrajParams), vp, u32]
    L.cm_map_traj_evaluate.argtypes = [vp, C.POINTER(TrajWindow), C.POINTER(TrajInfo)]
    L.cm_map_traj_copy.argtypes = [vp, vp, u64, C.POINTER(TrajInfo)]
    L.cm_map_traj_device.argtypes = [vp, C.POINTER(vp), C.POINTER(TrajInfo)]
    L.cm_traj_directions.argtypes = [vp, u64]
    L.cm_map_frontier_configure.argtypes = [vp, C.POINTER(FrontierParams)]
    L.cm_map_frontier_update.argtypes = [vp, C.POINTER(FrontierInfo), C.POINTER(MapInfo)]
    L.cm_map_frontier_copy.argtypes = [vp, vp, u64, C.POINTER(FrontierInfo)]
    L.cm_map_frontier_labels_copy.argtypes = [vp, vp, u64, C.POINTER(FrontierInfo)]
    L.cm_map_frontier_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(FrontierInfo)]
    L.cm_map_match_configure.argtypes = [vp, C.POINTER(MatchParams)]
    L.cm_map_match_evaluate.argtypes = [vp, vp, C.POINTER(MatchResult)]
    L.cm_map_match_copy.argtypes = [vp, vp, u64, C.POINTER(MatchResult)]
    L.cm_map_match_device.argtypes = [vp, C.POINTER(vp), C.POINTER(MatchResult)]
    L.cm_map_match_table_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_match_table.argtypes = [C.c_float, C.c_float, C.c_float, vp, u64, C.POINTER(u64)]
    L.cm_map_match_search_configure.argtypes = [vp, C.POINTER(MatchSearchParams)]
    L.cm_map_match_search.argtypes = [vp, vp, C.POINTER(MatchResult), C.POINTER(MatchSearchInfo)]
    L.cm_map_match_search_result.argtypes = [vp, C.POINTER(MatchResult), C.POINTER(MatchSearchInfo)]
    L.cm_map_match_search_level_copy.argtypes = [vp, C.c_uint32, vp, u64, C.POINTER(C.c_uint32 * 2)]
    L.cm_map_load.argtypes = [vp, vp, u64, C.POINTER(C.c_int32 * 2), C.POINTER(MapInfo)]
    L.cm_map_mcl_configure.argtypes = [vp, C.POINTER(MclParams)]
    L.cm_map_mcl_init_pose.argtypes = [vp] + [C.c_float] * 6
    L.cm_map_mcl_init_uniform.argtypes = [vp]
    L.cm_map_mcl_predict.argtypes = [vp] + [C.c_float] * 6
    L.cm_map_mcl_update.argtypes = [vp, C.POINTER(MclInfo)]
    L.cm_map_mcl_copy.argtypes = [vp, vp, u64]
    L.cm_map_mcl_weights_copy.argtypes = [vp, vp, u64, C.POINTER(MclInfo)]
    L.cm_map_mcl_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(MclInfo)]
    L.cm_mcl_draws.argtypes = [u64, u64, u32, u32, u32, vp]
    L.cm_map_mcl_beam_configure.argtypes = [vp, C.POINTER(MclBeamParams)]
    L.cm_map_mcl_beam_info_copy.argtypes = [vp, C.POINTER(MclBeamInfo)]
    L.cm_mcl_beam_table.argtypes = [C.POINTER(MclBeamParams), C.c_float, vp, u64]
    L.cm_map_mcl_hyp_configure.argtypes = [vp, C.POINTER(MclHypParams)]
    L.cm_map_mcl_hyp_copy.argtypes = [vp, C.POINTER(MclHyp), u64, C.POINTER(MclHypInfo)]
    L.cm_mcl_kld_bound.argtypes = [u32, C.c_float, C.c_float, C.POINTER(u32)]
    L.cm_map_cast_configure.argtypes = [vp, C.POINTER(CastParams), vp]
    L.cm_map_cast_evaluate.argtypes = [vp, vp, u32, C.POINTER(CastInfo)]
    L.cm_map_cast_evaluate_mcl.argtypes = [vp, C.POINTER(CastInfo)]
    L.cm_map_cast_copy.argtypes = [vp, vp, u64, C.POINTER(CastInfo)]
    L.cm_map_cast_device.argtypes = [vp, C.POINTER(vp), C.POINTER(CastInfo)]
    L.cm_cast_directions.argtypes = [u32, vp, u64]
    L.cm_result_normals.argtypes = [vp, C.POINTER(NormalParams), vp, u64]
    L.cm_result_normals_device.argtypes = [vp, C.POINTER(NormalParams), C.POINTER(vp), C.POINTER(u64)]
    L.cm_result_align.argtypes = [vp, C.POINTER(AlignParams), vp, u64, C.POINTER(AlignResult)]
    L.cm_result_align_device.argtypes = [vp, C.POINTER(AlignParams), vp, u64, C.POINTER(AlignResult)]
    L.cm_align_correspondences_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.cm_result_ndt_align.argtypes = [vp, C.POINTER(NdtParams), vp, u64, C.POINTER(NdtResult)]
    L.cm_result_ndt_align_device.argtypes = [vp, C.POINTER(NdtParams), vp, u64, C.POINTER(NdtResult)]
    L.cm_ndt_correspondences_copy.argtypes = [vp, vp, u64, C.POINTER(u64)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("cm_status_string", "cm_last_error"):
            fn.restype = C.c_int
    if hasattr(L, "cm_test_device_allocations"):             # the test build only: not in SYMBOLS, the shipped library has no such symbol
        L.cm_test_device_allocations.argtypes = [C.POINTER(u64), C.POINTER(u64)]
        L.cm_test_device_allocations.restype = C.c_int
    _lib = L
    return L


def device_allocations():
    """(live, total): allocations of the library's contexts alive in this process, and made so far. The test build only
    (CM_LIB_VARIANT=testhooks); the shipped library does not count."""
    live, total = C.c_uint64(), C.c_uint64()
    st = load().cm_test_device_allocations(C.byref(live), C.byref(total))
    if st != OK:
        raise CloudMergeError(st, "cm_test_device_allocations")
    return live.value, total.value


def box_directions(n):
    """(n, 2) float32: (cos, sin) of the n headings a box call tries — the table it uploads (cm_box_directions)."""
    out = np.empty((max(int(n), 1), 2), dtype=np.float32)
    st = load().cm_box_directions(int(n), out.ctypes.data, out.shape[0])
    if st != OK:
        raise CloudMergeError(st, "cm_box_directions")
    return out[: int(n)]


def traj_directions():
    """(TRAJ_HEADINGS, 2) float32: (cos, sin) of the rollout layer's binary headings — the table it uploads (cm_traj_directions)."""
    out = np.empty((TRAJ_HEADINGS, 2), dtype=np.float32)
    st = load().cm_traj_directions(out.ctypes.data, out.shape[0])
    if st != OK:
        raise CloudMergeError(st, "cm_traj_directions")
    return out


def match_table(cell, sigma, max_dist):
    """(R * R + 1,) uint8: the scan matching layer's field byte by squared distance in cells (cm_match_table)."""
    out = np.empty(MATCH_MAX_RADIUS_CELLS * MATCH_MAX_RADIUS_CELLS + 1, dtype=np.uint8)
    n = C.c_uint64(0)
    st = load().cm_match_table(float(cell), float(sigma), float(max_dist), out.ctypes.data, out.shape[0], C.byref(n))
    if st != OK:
        raise CloudMergeError(st, "cm_match_table")
    return out[: n.value].copy()


def mcl_draws(seed, gen, first_p, n_p, i):
    """(n_p,) uint64: the localisation layer's draw(p, i) for p = first_p .. first_p + n_p - 1 of the call gen (cm_mcl_draws)."""
    out = np.empty(int(n_p), dtype=np.uint64)
    st = load().cm_mcl_draws(int(seed) & (2**64 - 1), int(gen) & (2**64 - 1), int(first_p), int(n_p), int(i), out.ctypes.data if n_p else None)
    if st != OK and n_p:
        raise CloudMergeError(st, "cm_mcl_draws")
    return out


def mcl_kld_bound(k, err=0.05, z=2.326):
    """The KLD bound on the particle count for k occupied bins (cm_mcl_kld_bound): with probability given by the quantile z the
    divergence between the sampled and the true belief stays below err."""
    out = C.c_uint32()
    st = load().cm_mcl_kld_bound(int(k), float(err), float(z), C.byref(out))
    if st != OK:
        raise CloudMergeError(st, "cm_mcl_kld_bound")
    return out.value


def mcl_beam_table(cell, over_cells=8, sigma=0.1, z_hit=0.75, z_short=0.125, z_rand=0.125, plain=False):
    """(2 * over_cells + 3,) uint8: the beam model's table over a map of this cell (cm_mcl_beam_table): a hit at -over_cells ..
    over_cells steps from the measured end, then no hit within reach, then off the window."""
    p = MclBeamParams(int(over_cells), float(sigma), float(z_hit), float(z_short), float(z_rand), MCL_BEAM_PLAIN if plain else 0)
    out = np.empty(2 * int(over_cells) + 3, dtype=np.uint8)
    st = load().cm_mcl_beam_table(C.byref(p), float(cell), out.ctypes.data, out.shape[0])
    if st != OK:
        raise CloudMergeError(st, "cm_mcl_beam_table")
    return out


def cast_directions(range_cells):
    """(TRAJ_HEADINGS, 2) int16: the cast layer's direction table for range_cells, rint(range_cells * (cos, sin)) (cm_cast_directions)."""
    out = np.empty((TRAJ_HEADINGS, 2), dtype=np.int16)
    st = load().cm_cast_directions(int(range_cells), out.ctypes.data, out.shape[0])
    if st != OK:
        raise CloudMergeError(st, "cm_cast_directions")
    return out


def cast_heading(yaw):
    """The binary angle of a yaw in radians: rint(yaw * 2^32 / (2 pi)) mod 2^32, the rollout layer's conversion."""
    return int(np.rint(float(yaw) * (4294967296.0 / 6.283185307179586))) & 0xFFFFFFFF


def status_string(status):
    return load().cm_status_string(int(status)).decode()


def make_params(p: MergeParams) -> Params:
    cp = Params()
    cp.leaf = (C.c_float * 3)(*[float(v) for v in p.leaf])
    cp.min_points_per_voxel = int(p.min_points_per_voxel)
    cp.downsample_all_data = int(bool(p.downsample_all_data))
    if p.crop_min is not None:
        cp.crop_enable = 1
        cp.crop_min = (C.c_float * 3)(*[float(v) for v in p.crop_min])
        cp.crop_max = (C.c_float * 3)(*[float(v) for v in p.crop_max])
    cp.required_sensor_mask = int(p.required_sensor_mask)
    if getattr(p, "outlier_radius", None):
        cp.outlier_enable = 1
        cp.outlier_radius = float(p.outlier_radius)
        cp.outlier_min_neighbors = int(p.outlier_min_neighbors)
    return cp


def pinned_array(nbytes):
    """uint8 numpy view of nbytes of pinned host memory (cm_host_alloc); keep the returned holder alive
    and call holder.free() when done."""
    L = load()
    ptr = C.c_void_p()
    st = L.cm_host_alloc(C.byref(ptr), int(nbytes))
    if st != OK:
        raise CloudMergeError(st, "cm_host_alloc")
    buf = (C.c_uint8 * int(nbytes)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=np.uint8)

    class _Holder:
        def __init__(self):
            self.array, self.ptr = arr, ptr

        def free(self):
            if self.ptr:
                L.cm_host_free(self.ptr)
                self.ptr = None

    return _Holder()


class CloudMerger:
    """Thin object wrapper over a cm_ctx. Mirrors the calling pattern of the reference node:
    set the static transforms once (:556-561), submit one cloud per sensor (callbacks :318-508),
    then merge_voxelize() (main loop :574-577) and fetch the voxel cloud (:215-219)."""

    def __init__(self, max_points_total, max_sensors=MAX_SENSORS, device=0, flags=0):
        self._lib = load()
        self._ctx = C.c_void_p()
        lim = Limits(int(max_sensors), int(flags), int(max_points_total))
        st = self._lib.cm_create(C.byref(self._ctx), int(device), C.byref(lim))
        if st != OK:
            self._ctx = None
            raise CloudMergeError(st, "cm_create")
        self.flags = flags
        self.max_points_total = int(max_points_total)
        self._keep = {}

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.cm_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st, what, ok=(OK,)):
        if st not in ok:
            raise CloudMergeError(st, f"{what}: {self._lib.cm_last_error(self._ctx).decode()}")
        return st

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.cm_set_stream(self._ctx, C.c_void_p(hip_stream_ptr)), "cm_set_stream")

    def set_transform(self, sensor, q_xyzw, t_xyz):
        q = (C.c_double * 4)(*[float(v) for v in q_xyzw])
        t = (C.c_double * 3)(*[float(v) for v in t_xyz])
        self._check(self._lib.cm_set_sensor_transform(self._ctx, sensor, q, t), "cm_set_sensor_transform")

    def set_matrix(self, sensor, m):
        mm = (C.c_float * 12)(*np.asarray(m, dtype=np.float32).reshape(-1))
        self._check(self._lib.cm_set_sensor_matrix(self._ctx, sensor, mm), "cm_set_sensor_matrix")

    def get_matrix(self, sensor):
        mm = (C.c_float * 12)()
        self._check(self._lib.cm_get_sensor_matrix(self._ctx, sensor, mm), "cm_get_sensor_matrix")
        return np.array(mm, dtype=np.float32).reshape(3, 4)

    def submit(self, sensor, cloud: SensorCloud):
        data = np.ascontiguousarray(cloud.data)
        off_i = NO_FIELD if cloud.off_i is None else cloud.off_i
        return self._check(self._lib.cm_submit_cloud(self._ctx, sensor, data.ctypes.data, cloud.n, cloud.point_step,
                                                     cloud.off_x, cloud.off_y, cloud.off_z, off_i), "cm_submit_cloud",
                           ok=(OK, SKIPPED))

    def submit_async(self, sensor, cloud: SensorCloud, host_ptr=None):
        """cm_submit_cloud_async: the payload (cloud.data, or host_ptr: e.g. pinned memory) must stay alive and unchanged
        until the frame that consumes it has been waited for."""
        ptr = host_ptr if host_ptr is not None else np.ascontiguousarray(cloud.data).ctypes.data
        off_i = NO_FIELD if cloud.off_i is None else cloud.off_i
        return self._check(self._lib.cm_submit_cloud_async(self._ctx, sensor, C.c_void_p(ptr), cloud.n, cloud.point_step,
                                                           cloud.off_x, cloud.off_y, cloud.off_z, off_i), "cm_submit_cloud_async",
                           ok=(OK, SKIPPED))

    def result_async(self, host_ptr, capacity):
        self._check(self._lib.cm_result_copy_async(self._ctx, C.c_void_p(host_ptr), int(capacity)), "cm_result_copy_async")

    def sync(self):
        self._check(self._lib.cm_sync(self._ctx), "cm_sync")

    def publish_async(self, host_ptr, capacity, step_out=16):
        """Copy-out of the last waited-for frame on the context's publish stream (cm_result_publish_async)."""
        self._check(self._lib.cm_result_publish_async(self._ctx, C.c_void_p(host_ptr), int(capacity), int(step_out)),
                    "cm_result_publish_async")

    def publish_wait(self):
        self._check(self._lib.cm_publish_wait(self._ctx), "cm_publish_wait")

    def frame_stats(self):
        fs = FrameStats()
        self._check(self._lib.cm_get_frame_stats(self._ctx, C.byref(fs)), "cm_get_frame_stats")
        k = fs.n_sensors
        return {"sensor": list(fs.sensor[:k]), "n_in": list(fs.n_in[:k]), "n_kept": list(fs.n_kept[:k]), "fresh": list(fs.fresh[:k]),
                "generation": list(fs.generation[:k]), "bytes_h2d": list(fs.bytes_h2d[:k]), "bytes_h2d_total": fs.bytes_h2d_total, "bytes_d2h_total": fs.bytes_d2h_total,
                "bytes_algorithmic": fs.bytes_algorithmic}

    def submit_device(self, sensor, dev_ptr, n, point_step=16, off_x=0, off_y=4, off_z=8, off_i=12):
        off_i = NO_FIELD if off_i is None else off_i
        return self._check(self._lib.cm_submit_cloud_device(self._ctx, sensor, C.c_void_p(dev_ptr), n, point_step,
                                                            off_x, off_y, off_z, off_i), "cm_submit_cloud_device",
                           ok=(OK, SKIPPED))

    def clear(self, sensor):
        self._check(self._lib.cm_clear_sensor(self._ctx, sensor), "cm_clear_sensor")

    def submit_all(self, sensors):
        for s, cloud in enumerate(sensors):
            self.set_transform(s, cloud.q_xyzw, cloud.t_xyz)
            self.submit(s, cloud)

    def merge_voxelize(self, params: MergeParams) -> Result:
        res = Result()
        st = self._lib.cm_merge_voxelize(self._ctx, C.byref(make_params(params)), C.byref(res))
        self._check(st, "cm_merge_voxelize", ok=(OK, EMPTY_INPUT, GRID_OVERFLOW, NOT_READY))
        return res

    def merge_voxelize_async(self, cparams: Params):
        return self._check(self._lib.cm_merge_voxelize_async(self._ctx, C.byref(cparams)),
                           "cm_merge_voxelize_async", ok=(OK, NOT_READY))

    def wait(self) -> Result:
        res = Result()
        self._check(self._lib.cm_wait(self._ctx, C.byref(res)), "cm_wait", ok=(OK, EMPTY_INPUT, GRID_OVERFLOW))
        return res

    def result(self, n_out, point_step=16):
        """(n_out,) structured XYZI array (step 16) or (n_out, 8) float32 PointXYZI images (step 32)."""
        n_out = int(n_out)
        if point_step == 16:
            out = np.zeros(n_out, dtype=XYZI_DTYPE)
        else:
            out = np.zeros((n_out, 8), dtype=np.float32)
        self._check(self._lib.cm_result_copy(self._ctx, out.ctypes.data if n_out else None, n_out, point_step),
                    "cm_result_copy")
        return out

    def result_device(self):
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_result_device(self._ctx, C.byref(ptr), C.byref(n)), "cm_result_device")
        return ptr.value, n.value

    def cells(self, n_out):
        n_out = int(n_out)
        ijk = np.zeros((n_out, 3), dtype=np.int32)
        cnt = np.zeros(n_out, dtype=np.uint32)
        self._check(self._lib.cm_result_copy_cells(self._ctx, ijk.ctypes.data, cnt.ctypes.data, n_out),
                    "cm_result_copy_cells")
        return ijk, cnt

    def merged(self, capacity):
        out = np.zeros(int(capacity), dtype=XYZI_DTYPE)
        n = C.c_uint64()
        self._check(self._lib.cm_merged_copy(self._ctx, out.ctypes.data, int(capacity), C.byref(n)), "cm_merged_copy")
        return out[: n.value].copy()

    # ---- fused cloud across GPUs ----
    def set_ground_removal(self, gparams):
        """gparams: GroundParams (make_ground_params) or None to switch the stage off."""
        self._check(self._lib.cm_set_ground_removal(self._ctx, C.byref(gparams) if gparams is not None else None),
                    "cm_set_ground_removal")

    def ground(self, capacity):
        out = np.zeros(int(capacity), dtype=XYZI_DTYPE)
        n = C.c_uint64()
        self._check(self._lib.cm_ground_copy(self._ctx, out.ctypes.data, int(capacity), C.byref(n)), "cm_ground_copy")
        return out[:n.value]

    def ground_planes(self):
        arr = (GroundPlane * (MAX_SENSORS * MAX_ZONES))()
        self._check(self._lib.cm_ground_planes(self._ctx, arr, MAX_SENSORS * MAX_ZONES), "cm_ground_planes")
        return arr

    def local_bounds(self, params: MergeParams):
        mn, mx, n = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint64()
        self._check(self._lib.cm_local_bounds(self._ctx, C.byref(make_params(params)), mn, mx, C.byref(n)),
                    "cm_local_bounds")
        return np.array(mn, dtype=np.float32), np.array(mx, dtype=np.float32), n.value

    def merge_partial(self, params: MergeParams, global_min_max=None) -> Result:
        res = Result()
        b = None if global_min_max is None else (C.c_float * 6)(*[float(v) for v in global_min_max])
        st = self._lib.cm_merge_partial(self._ctx, C.byref(make_params(params)), b, C.byref(res))
        self._check(st, "cm_merge_partial", ok=(OK, EMPTY_INPUT, NOT_READY))
        return res

    def partial_device(self):
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_partial_device(self._ctx, C.byref(ptr), C.byref(n)), "cm_partial_device")
        return ptr.value, n.value

    def partial(self, n_entries):
        out = np.zeros(int(n_entries), dtype=ENTRY_DTYPE)
        self._check(self._lib.cm_partial_copy(self._ctx, out.ctypes.data if n_entries else None, int(n_entries)),
                    "cm_partial_copy")
        return out

    def partial_to_device(self, dst_ptr, capacity):
        self._check(self._lib.cm_partial_copy(self._ctx, C.c_void_p(dst_ptr), int(capacity)), "cm_partial_copy")

    def merge_tables(self, table_ptrs, counts, params: MergeParams) -> Result:
        n = len(table_ptrs)
        ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in table_ptrs])
        cnts = (C.c_uint64 * n)(*[int(v) for v in counts])
        res = Result()
        st = self._lib.cm_merge_tables(self._ctx, ptrs, cnts, n, C.byref(make_params(params)), C.byref(res))
        self._check(st, "cm_merge_tables", ok=(OK, EMPTY_INPUT))
        return res

    # ---- ego-motion compensation (cm_set_ego_motion) ----
    def set_time_field(self, sensor, offset, type_):
        """Per-point time field of a sensor's clouds: byte offset and TIME_NONE / TIME_F32_S / TIME_U32_NS."""
        self._check(self._lib.cm_set_sensor_time_field(self._ctx, int(sensor), int(offset), int(type_)), "cm_set_sensor_time_field")

    def set_ego_motion(self, motion):
        """motion: Motion (make_motion) or None to switch compensation off."""
        self._check(self._lib.cm_set_ego_motion(self._ctx, C.byref(motion) if motion is not None else None), "cm_set_ego_motion")

    # ---- per-voxel covariance of the last result (cm_result_voxel_cov) ----
    def voxel_covariance(self, n_out, min_points=6, eig_mult=0.01):
        """(n_out,) VOXEL_COV_DTYPE array: entry k belongs to result record k (pcl::VoxelGridCovariance's statistics)."""
        n_out = int(n_out)
        out = np.zeros(n_out, dtype=VOXEL_COV_DTYPE)
        p = CovParams(int(min_points), float(eig_mult))
        self._check(self._lib.cm_result_voxel_cov(self._ctx, C.byref(p), out.ctypes.data if n_out else None, n_out),
                    "cm_result_voxel_cov")
        return out

    def voxel_covariance_device(self, min_points=6, eig_mult=0.01):
        """(device pointer, entries) of the same table, owned by the context and valid until the next merge."""
        ptr, n = C.c_void_p(), C.c_uint64()
        p = CovParams(int(min_points), float(eig_mult))
        self._check(self._lib.cm_result_voxel_cov_device(self._ctx, C.byref(p), C.byref(ptr), C.byref(n)),
                    "cm_result_voxel_cov_device")
        return ptr.value, n.value

    # ---- Euclidean cluster extraction on the last result (cm_result_clusters) ----
    def clusters(self, tolerance, min_size=1, max_size=2**32 - 1):
        """(labels, clusters, indices) of the last result: labels (n_out,) uint32, CLUSTER_NONE where the size filter dropped
        the voxel's component; clusters (n_clusters,) CLUSTER_DTYPE; indices (n_clustered,) uint32, the member voxels grouped
        by cluster and ascending inside one (pcl::EuclideanClusterExtraction, numbered by smallest member)."""
        p = ClusterParams(float(tolerance), int(min_size), int(max_size), 0)
        _, n_out = self.result_device()
        cap = max(int(n_out), 1)
        labels = np.empty(cap, dtype=np.uint32)
        table = np.empty(cap, dtype=CLUSTER_DTYPE)
        indices = np.empty(cap, dtype=np.uint32)
        nc, nm = C.c_uint64(), C.c_uint64()
        self._check(self._lib.cm_result_clusters(self._ctx, C.byref(p), labels.ctypes.data, cap, table.ctypes.data, cap,
                                                 indices.ctypes.data, cap, C.byref(nc), C.byref(nm)), "cm_result_clusters")
        return labels[: int(n_out)].copy(), table[: nc.value].copy(), indices[: nm.value].copy()

    def clusters_device(self, tolerance, min_size=1, max_size=2**32 - 1):
        """(labels ptr, clusters ptr, indices ptr, n_clusters, n_clustered): the same tables in device memory, owned by the
        context and valid until the next merge or the next call."""
        p = ClusterParams(float(tolerance), int(min_size), int(max_size), 0)
        lp, cp, ip = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nc, nm = C.c_uint64(), C.c_uint64()
        self._check(self._lib.cm_result_clusters_device(self._ctx, C.byref(p), C.byref(lp), C.byref(cp), C.byref(ip), C.byref(nc),
                                                        C.byref(nm)), "cm_result_clusters_device")
        return lp.value, cp.value, ip.value, nc.value, nm.value

    # ---- oriented boxes of the last result's clusters (cm_result_cluster_boxes) ----
    @staticmethod
    def box_params(tolerance, min_size=1, max_size=2**32 - 1, n_angles=90, criterion=BOX_CLOSENESS, d_min=0.01):
        return BoxParams(ClusterParams(float(tolerance), int(min_size), int(max_size), 0), int(n_angles), int(criterion),
                         float(d_min), 0)

    def cluster_boxes(self, tolerance, min_size=1, max_size=2**32 - 1, n_angles=90, criterion=BOX_CLOSENESS, d_min=0.01):
        """(n_clusters,) BOX_DTYPE array: entry k is the oriented box of cluster k of clusters(tolerance, min_size, max_size) —
        the best of n_angles headings in [0, 90 deg) under the criterion. The context then holds those cluster tables."""
        p = self.box_params(tolerance, min_size, max_size, n_angles, criterion, d_min)
        _, n_out = self.result_device()
        out = np.empty(max(int(n_out), 1), dtype=BOX_DTYPE)
        n = C.c_uint64()
        self._check(self._lib.cm_result_cluster_boxes(self._ctx, C.byref(p), out.ctypes.data, out.shape[0], C.byref(n)),
                    "cm_result_cluster_boxes")
        return out[: n.value].copy()

    def cluster_boxes_device(self, tolerance, min_size=1, max_size=2**32 - 1, n_angles=90, criterion=BOX_CLOSENESS, d_min=0.01):
        """(device pointer, entries) of the same table, owned by the context and valid until the next merge or the next cluster
        or box call."""
        p = self.box_params(tolerance, min_size, max_size, n_angles, criterion, d_min)
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_result_cluster_boxes_device(self._ctx, C.byref(p), C.byref(ptr), C.byref(n)),
                    "cm_result_cluster_boxes_device")
        return ptr.value, n.value

    # ---- 2-D grid map of the last frame (cm_result_grid_map) ----
    @staticmethod
    def grid_params(origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1):
        return GridParams((C.c_float * 2)(float(origin[0]), float(origin[1])), float(cell), int(nx), int(ny), float(z_band[0]),
                          float(z_band[1]), float(obstacle_height), int(min_points))

    def grid_map(self, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1):
        """(ny, nx) GRID_DTYPE array: per cell of the grid whose cell (0, 0) has its corner at origin the counts of the frame's
        kept and ground points inside z_band, their lowest and highest z, the largest intensity and the state
        (GRID_UNKNOWN / GRID_FREE / GRID_OCCUPIED). Row iy, column ix."""
        p = self.grid_params(origin, cell, nx, ny, z_band, obstacle_height, min_points)
        n = int(nx) * int(ny)
        out = np.empty(n if 0 < n <= GRID_MAX_CELLS else 1, dtype=GRID_DTYPE)     # (a grid the library refuses: one entry)
        self._check(self._lib.cm_result_grid_map(self._ctx, C.byref(p), out.ctypes.data, out.shape[0]), "cm_result_grid_map")
        self._grid_shape = (int(ny), int(nx))
        return out.reshape(int(ny), int(nx))

    def grid_map_device(self, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1):
        """(device pointer, cells) of the same table, owned by the context and valid until the next merge or the next grid call."""
        p = self.grid_params(origin, cell, nx, ny, z_band, obstacle_height, min_points)
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_result_grid_map_device(self._ctx, C.byref(p), C.byref(ptr), C.byref(n)), "cm_result_grid_map_device")
        self._grid_shape = (int(ny), int(nx))
        return ptr.value, n.value

    def grid_occupancy(self):
        """(ny, nx) int8 image of the last grid call since the last merge: -1 unknown, 0 free, 100 occupied
        (nav_msgs/OccupancyGrid::data, row-major)."""
        n = C.c_uint64()
        st = self._lib.cm_grid_occupancy_copy(self._ctx, None, 0, C.byref(n))
        if st != CAPACITY:
            self._check(st, "cm_grid_occupancy_copy")
        out = np.empty(max(n.value, 1), dtype=np.int8)
        self._check(self._lib.cm_grid_occupancy_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(n)), "cm_grid_occupancy_copy")
        ny, nx = self._grid_shape
        return out[: n.value].reshape(ny, nx)

    # ---- free-space ray casting over the grid map of the last frame (cm_result_grid_rays) ----
    def grid_rays(self, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1, min_pass=1,
                  max_range_cells=0):
        """(ny, nx) RAY_DTYPE array: per cell the rays that cross it (n_pass) and that end in it (n_end), a ray being an
        integer line from a sensor's cell to a distinct cell that holds one of that sensor's counted points. The grid map of
        the same parameters is computed first (grid_occupancy() returns its image); grid_ray_occupancy() returns the image in
        which an unknown cell crossed by at least min_pass rays is free."""
        p = self.grid_params(origin, cell, nx, ny, z_band, obstacle_height, min_points)
        r = RayParams(int(min_pass), int(max_range_cells))
        n = int(nx) * int(ny)
        out = np.empty(n if 0 < n <= GRID_MAX_CELLS else 1, dtype=RAY_DTYPE)      # (a grid the library refuses: one entry)
        self._check(self._lib.cm_result_grid_rays(self._ctx, C.byref(p), C.byref(r), out.ctypes.data, out.shape[0]),
                    "cm_result_grid_rays")
        self._grid_shape = (int(ny), int(nx))
        return out.reshape(int(ny), int(nx))

    def grid_rays_device(self, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1, min_pass=1,
                         max_range_cells=0):
        """(device pointer, cells) of the same table, owned by the context and valid until the next merge, grid or ray call."""
        p = self.grid_params(origin, cell, nx, ny, z_band, obstacle_height, min_points)
        r = RayParams(int(min_pass), int(max_range_cells))
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_result_grid_rays_device(self._ctx, C.byref(p), C.byref(r), C.byref(ptr), C.byref(n)),
                    "cm_result_grid_rays_device")
        self._grid_shape = (int(ny), int(nx))
        return ptr.value, n.value

    def grid_ray_occupancy(self):
        """(ny, nx) int8 cleared image of the last ray call since the last merge or grid call: -1 unknown, 0 free, 100 occupied."""
        n = C.c_uint64()
        st = self._lib.cm_grid_ray_occupancy_copy(self._ctx, None, 0, C.byref(n))
        if st != CAPACITY:
            self._check(st, "cm_grid_ray_occupancy_copy")
        out = np.empty(max(n.value, 1), dtype=np.int8)
        self._check(self._lib.cm_grid_ray_occupancy_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(n)),
                    "cm_grid_ray_occupancy_copy")
        ny, nx = self._grid_shape
        return out[: n.value].reshape(ny, nx)

    # ---- rolling log-odds occupancy map accumulated over frames (cm_map_configure / cm_map_integrate) ----
    @staticmethod
    def map_params(cell, nx, ny, z_band=(-np.inf, np.inf), l_hit=85, l_miss=40, l_min=-200, l_max=350, l_free=-40, l_occ=85,
                   max_range_cells=0):
        return MapParams(float(cell), int(nx), int(ny), float(z_band[0]), float(z_band[1]), int(l_hit), int(l_miss), int(l_min),
                         int(l_max), int(l_free), int(l_occ), int(max_range_cells))

    def map_configure(self, cell=None, nx=0, ny=0, z_band=(-np.inf, np.inf), l_hit=85, l_miss=40, l_min=-200, l_max=350, l_free=-40,
                      l_occ=85, max_range_cells=0):
        """Allocates and clears the occupancy map: a window of nx x ny cells of edge `cell` that scrolls with the vehicle over a
        lattice fixed in the world frame. The log-odds are integers (the defaults are octomap's 0.85 / -0.4 / clamps -2 and 3.5,
        times 100). cell None frees the map."""
        if cell is None:
            self._check(self._lib.cm_map_configure(self._ctx, None), "cm_map_configure")
            return
        p = self.map_params(cell, nx, ny, z_band, l_hit, l_miss, l_min, l_max, l_free, l_occ, max_range_cells)
        self._check(self._lib.cm_map_configure(self._ctx, C.byref(p)), "cm_map_configure")
        self._map_cell = float(p.cell)                 # (the fp32 cell the library uses, for map_cast_ranges)

    def map_integrate(self, pose=None):
        """Integrates the last frame into the map: pose is the 3 x 4 matrix (fp32) that takes the vehicle frame at the frame's
        reference instant into the world frame, None the identity. Each frame is integrated at most once. Returns the MapInfo."""
        m = np.eye(3, 4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32).reshape(3, 4)
        mm = (C.c_float * 12)(*m.reshape(-1))
        info = MapInfo()
        self._check(self._lib.cm_map_integrate(self._ctx, mm, C.byref(info)), "cm_map_integrate")
        return info

    def map(self):
        """((ny, nx) MAP_DTYPE array, MapInfo): the log-odds and observation count of every window cell."""
        info = MapInfo()
        st = self._lib.cm_map_copy(self._ctx, None, 0, C.byref(info))
        if st != CAPACITY:
            self._check(st, "cm_map_copy")
        out = np.empty(info.nx * info.ny, dtype=MAP_DTYPE)
        self._check(self._lib.cm_map_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_copy")
        return out.reshape(info.ny, info.nx), info

    def map_device(self):
        """(device pointer, MapInfo) of the same table, owned by the context and valid until the next integrate or configure call."""
        ptr, info = C.c_void_p(), MapInfo()
        self._check(self._lib.cm_map_device(self._ctx, C.byref(ptr), C.byref(info)), "cm_map_device")
        return ptr.value, info

    def map_occupancy(self):
        """((ny, nx) int8 image, MapInfo): -1 unknown, 0 free, 100 occupied (nav_msgs/OccupancyGrid::data, row-major)."""
        info = MapInfo()
        st = self._lib.cm_map_occupancy_copy(self._ctx, None, 0, C.byref(info))
        if st != CAPACITY:
            self._check(st, "cm_map_occupancy_copy")
        out = np.empty(info.nx * info.ny, dtype=np.int8)
        self._check(self._lib.cm_map_occupancy_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_occupancy_copy")
        return out.reshape(info.ny, info.nx), info

    def map_load(self, table, anchor):
        """Puts a recorded map back: table is what map() returned ((ny, nx) MAP_DTYPE), anchor its MapInfo's anchor. The layers
        behind go stale as after an integration. Returns the MapInfo."""
        t = np.ascontiguousarray(table, dtype=MAP_DTYPE).reshape(-1)
        a = (C.c_int32 * 2)(int(anchor[0]), int(anchor[1]))
        info = MapInfo()
        self._check(self._lib.cm_map_load(self._ctx, t.ctypes.data, t.shape[0], C.byref(a), C.byref(info)), "cm_map_load")
        return info

    # ---- cost layer over the occupancy map (cm_map_cost_configure / cm_map_cost_update) ----
    def map_cost_configure(self, inscribed_radius=None, inflation_radius=0.0, cost_scaling=0.0, inflate_unknown=False):
        """Allocates the cost layer behind the configured map and builds its table: costmap_2d's inflation layer (254 lethal, 253
        within inscribed_radius, an exponential decay at cost_scaling per metre out to inflation_radius, 255 unknown) over the
        exact distance field. inscribed_radius None frees the layer."""
        if inscribed_radius is None:
            self._check(self._lib.cm_map_cost_configure(self._ctx, None), "cm_map_cost_configure")
            return
        p = CostParams(float(inscribed_radius), float(inflation_radius), float(cost_scaling), COST_INFLATE_UNKNOWN if inflate_unknown else 0)
        self._check(self._lib.cm_map_cost_configure(self._ctx, C.byref(p)), "cm_map_cost_configure")

    def map_cost_update(self):
        """Computes both tables from the map's current image. Returns the MapInfo."""
        info = MapInfo()
        self._check(self._lib.cm_map_cost_update(self._ctx, C.byref(info)), "cm_map_cost_update")
        return info

    def map_cost(self):
        """((ny, nx) uint8 cost, (ny, nx) uint32 dist2, MapInfo) of the last update: the inflated cost and the squared distance
        in cells to the nearest occupied cell of the window (MAP_DIST_NONE where the window holds none)."""
        info = MapInfo()
        st = self._lib.cm_map_cost_copy(self._ctx, None, 0, C.byref(info))
        if st != CAPACITY:
            self._check(st, "cm_map_cost_copy")
        n = info.nx * info.ny
        cost, dist2 = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint32)
        self._check(self._lib.cm_map_cost_copy(self._ctx, cost.ctypes.data, n, C.byref(info)), "cm_map_cost_copy")
        self._check(self._lib.cm_map_dist_copy(self._ctx, dist2.ctypes.data, n, C.byref(info)), "cm_map_dist_copy")
        return cost.reshape(info.ny, info.nx), dist2.reshape(info.ny, info.nx), info

    def map_cost_device(self):
        """(cost device pointer, dist2 device pointer, MapInfo) of the same tables, owned by the context and valid until the next
        update, integrate or configure call."""
        cost, dist2, info = C.c_void_p(), C.c_void_p(), MapInfo()
        self._check(self._lib.cm_map_cost_device(self._ctx, C.byref(cost), C.byref(dist2), C.byref(info)), "cm_map_cost_device")
        return cost.value, dist2.value, info

    def map_cost_table(self):
        """(R * R + 1,) uint8: the cost of a free cell by its squared distance in cells, as cm_map_cost_configure built it."""
        n = C.c_uint64(0)
        st = self._lib.cm_map_cost_table_copy(self._ctx, None, 0, C.byref(n))
        if st != CAPACITY:
            self._check(st, "cm_map_cost_table_copy")
        out = np.empty(n.value, dtype=np.uint8)
        self._check(self._lib.cm_map_cost_table_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(n)), "cm_map_cost_table_copy")
        return out

    # ---- plan layer behind the cost layer (cm_map_plan_configure / cm_map_plan_update / cm_map_plan_path) ----
    def map_plan_configure(self, neutral=50, cost_factor_q8=205, allow_unknown=False, max_path_cells=None):
        """Allocates the plan layer behind the configured cost layer: the shortest-path potential to a goal over the cost table
        (a cell weighs neutral + ((cost * cost_factor_q8) >> 8), 5 per straight and 7 per diagonal step, 253..255 impassable,
        255 as 252 with allow_unknown) and paths of at most max_path_cells cells (None: nx * ny). neutral None frees the layer."""
        if neutral is None:
            self._check(self._lib.cm_map_plan_configure(self._ctx, None), "cm_map_plan_configure")
            return
        if max_path_cells is None:
            info = MapInfo()
            st = self._lib.cm_map_copy(self._ctx, None, 0, C.byref(info))
            if st != CAPACITY:
                self._check(st, "cm_map_copy")
            max_path_cells = info.nx * info.ny
        p = PlanParams(int(neutral), int(cost_factor_q8), PLAN_ALLOW_UNKNOWN if allow_unknown else 0, int(max_path_cells))
        self._check(self._lib.cm_map_plan_configure(self._ctx, C.byref(p)), "cm_map_plan_configure")
        self._plan_max_path_cells = p.max_path_cells

    def map_plan_update(self, x, y):
        """Computes the potential of every window cell to the goal at world (x, y) from the cost layer's fresh table. Returns the
        PlanInfo."""
        info = PlanInfo()
        self._check(self._lib.cm_map_plan_update(self._ctx, float(x), float(y), C.byref(info), None), "cm_map_plan_update")
        return info

    def map_plan(self):
        """((ny, nx) uint32 pot, PlanInfo) of the last update: the exact cost of the cheapest path to the goal (PLAN_UNREACHABLE
        where there is none)."""
        info, m = PlanInfo(), MapInfo()
        st = self._lib.cm_map_plan_copy(self._ctx, None, 0, C.byref(info), C.byref(m))
        if st != CAPACITY:
            self._check(st, "cm_map_plan_copy")
        n = m.nx * m.ny
        pot = np.empty(n, dtype=np.uint32)
        self._check(self._lib.cm_map_plan_copy(self._ctx, pot.ctypes.data, n, C.byref(info), C.byref(m)), "cm_map_plan_copy")
        return pot.reshape(m.ny, m.nx), info

    def map_plan_device(self):
        """(pot device pointer, PlanInfo, MapInfo) of the same table, owned by the context and valid until the next update,
        integrate or configure call."""
        pot, info, m = C.c_void_p(), PlanInfo(), MapInfo()
        self._check(self._lib.cm_map_plan_device(self._ctx, C.byref(pot), C.byref(info), C.byref(m)), "cm_map_plan_device")
        return pot.value, info, m

    def map_path(self, x, y):
        """((n_cells,) uint32 window cell indices ix + iy * nx, PathInfo): the path by descent from world (x, y) to the goal of
        the last update, start first; empty with PATH_UNREACHABLE, the first max_path_cells cells with PATH_TRUNCATED."""
        info = PathInfo()
        cells = np.empty(getattr(self, "_plan_max_path_cells", 0), dtype=np.uint32)      # (one walk: no path is longer)
        self._check(self._lib.cm_map_plan_path(self._ctx, float(x), float(y), cells.ctypes.data, cells.shape[0], C.byref(info)), "cm_map_plan_path")
        return cells[:info.n_cells].copy(), info

    # ---- rollout layer behind the plan layer (cm_map_traj_configure / cm_map_traj_evaluate) ----
    def map_traj_configure(self, nv=None, nw=1, n_steps=1, footprint=((0.0, 0.0),), occ_scale=1, goal_scale=1, allow_unknown=False):
        """Allocates the rollout layer behind the configured plan layer: nv x nw velocity samples rolled n_steps forward, the
        footprint ((n_foot, 2) body-frame points, x forward, y left, metres) checked against the cost table at every pose, a
        survivor's total occ_scale * (largest cost byte met) + goal_scale * pot(end). nv None frees the layer."""
        if nv is None:
            self._check(self._lib.cm_map_traj_configure(self._ctx, None, None, 0), "cm_map_traj_configure")
            return
        foot = np.ascontiguousarray(footprint, dtype=np.float32).reshape(-1, 2)
        p = TrajParams(int(nv), int(nw), int(n_steps), int(occ_scale), int(goal_scale), TRAJ_ALLOW_UNKNOWN if allow_unknown else 0)
        self._check(self._lib.cm_map_traj_configure(self._ctx, C.byref(p), foot.ctypes.data, foot.shape[0]), "cm_map_traj_configure")
        self._traj_n = p.nv * p.nw

    def map_traj_evaluate(self, x, y, yaw, v=(0.0, 0.0), w=(0.0, 0.0), dt=0.1):
        """Rolls and scores every sample from the pose (x, y, yaw) over the velocity window v = (lo, hi), w = (lo, hi) with steps
        of dt seconds, from the fresh cost table and pot. Returns the TrajInfo."""
        win = TrajWindow(float(x), float(y), float(yaw), float(v[0]), float(v[1]), float(w[0]), float(w[1]), float(dt))
        info = TrajInfo()
        self._check(self._lib.cm_map_traj_evaluate(self._ctx, C.byref(win), C.byref(info)), "cm_map_traj_evaluate")
        return info

    def map_traj(self):
        """((nv * nw,) TRAJ_SCORE_DTYPE scores, TrajInfo) of the last evaluate; sample (i, j) is entry i * nw + j."""
        info = TrajInfo()
        out = np.empty(getattr(self, "_traj_n", 0), dtype=TRAJ_SCORE_DTYPE)
        self._check(self._lib.cm_map_traj_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_traj_copy")
        return out, info

    def map_traj_device(self):
        """(scores device pointer, TrajInfo) of the same table, owned by the context and valid until the next evaluate, update,
        integrate or configure call."""
        ptr, info = C.c_void_p(), TrajInfo()
        self._check(self._lib.cm_map_traj_device(self._ctx, C.byref(ptr), C.byref(info)), "cm_map_traj_device")
        return ptr.value, info

    # ---- frontier layer behind the plan layer (cm_map_frontier_configure / cm_map_frontier_update) ----
    def map_frontier_configure(self, min_cells=1, max_frontiers=FRONTIER_MAX_TABLE, max_cost=252, pot_scale=1, gain_scale=0):
        """Allocates the frontier layer behind the configured plan layer: the free cells of the map's image with a cost byte of
        at most max_cost and an unknown edge neighbour, 8-connected, the components of at least min_cells cells numbered by
        their smallest cell, a table of at most max_frontiers of them and the one with the lowest pot_scale * min_pot -
        gain_scale * n_cells. min_cells None frees the layer."""
        if min_cells is None:
            self._check(self._lib.cm_map_frontier_configure(self._ctx, None), "cm_map_frontier_configure")
            return
        p = FrontierParams(int(min_cells), int(max_frontiers), int(max_cost), int(pot_scale), int(gain_scale))
        self._check(self._lib.cm_map_frontier_configure(self._ctx, C.byref(p)), "cm_map_frontier_configure")

    def map_frontier_update(self):
        """Computes labels, table and info from the map's image and the fresh cost table and pot. Returns the FrontierInfo."""
        info = FrontierInfo()
        self._check(self._lib.cm_map_frontier_update(self._ctx, C.byref(info), None), "cm_map_frontier_update")
        return info

    def map_frontiers(self):
        """((n_written,) FRONTIER_DTYPE table, FrontierInfo) of the last update; entry k is frontier k."""
        info = FrontierInfo()
        st = self._lib.cm_map_frontier_copy(self._ctx, None, 0, C.byref(info))
        if st != CAPACITY:
            self._check(st, "cm_map_frontier_copy")
        out = np.empty(info.n_written, dtype=FRONTIER_DTYPE)
        self._check(self._lib.cm_map_frontier_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_frontier_copy")
        return out, info

    def map_frontier_labels(self):
        """((ny, nx) uint32 labels, FrontierInfo) of the last update: a frontier's number, FRONTIER_NONE elsewhere."""
        info, m = FrontierInfo(), MapInfo()
        st = self._lib.cm_map_copy(self._ctx, None, 0, C.byref(m))
        if st != CAPACITY:
            self._check(st, "cm_map_copy")
        n = m.nx * m.ny
        out = np.empty(n, dtype=np.uint32)
        self._check(self._lib.cm_map_frontier_labels_copy(self._ctx, out.ctypes.data, n, C.byref(info)), "cm_map_frontier_labels_copy")
        return out.reshape(m.ny, m.nx), info

    def map_frontier_device(self):
        """(labels device pointer, table device pointer, FrontierInfo) of the same tables, owned by the context and valid until
        the next update, integrate or configure call."""
        labels, table, info = C.c_void_p(), C.c_void_p(), FrontierInfo()
        self._check(self._lib.cm_map_frontier_device(self._ctx, C.byref(labels), C.byref(table), C.byref(info)), "cm_map_frontier_device")
        return labels.value, table.value, info

    # ---- scan matching of the frame against the map, behind the cost layer (cm_map_match_configure / cm_map_match_evaluate) ----
    def map_match_configure(self, sigma=None, max_dist=0.5, n_a=0, a_stride=1, wx=0, wy=0, subcell=False):
        """Allocates the matching layer behind the configured cost layer: a likelihood field of standard deviation sigma cut at
        max_dist (metres), angle candidates -n_a..n_a at a_stride entries of the 4096-entry heading table, shifts -wx..wx and
        -wy..wy cells, the sub-cell offset with subcell. sigma None frees the layer."""
        if sigma is None:
            self._check(self._lib.cm_map_match_configure(self._ctx, None), "cm_map_match_configure")
            return
        p = MatchParams(float(sigma), float(max_dist), int(n_a), int(a_stride), int(wx), int(wy), MATCH_SUBCELL if subcell else 0)
        self._check(self._lib.cm_map_match_configure(self._ctx, C.byref(p)), "cm_map_match_configure")
        self._match_shape = (2 * p.n_a + 1, 2 * p.wy + 1, 2 * p.wx + 1)

    def map_match(self, pose):
        """Matches the last frame against the map around the prior pose (3 x 4, row-major). Returns the MatchResult."""
        p = np.ascontiguousarray(pose, dtype=np.float32).reshape(12)
        out = MatchResult()
        self._check(self._lib.cm_map_match_evaluate(self._ctx, p.ctypes.data, C.byref(out)), "cm_map_match_evaluate")
        return out

    def map_match_scores(self):
        """((2 n_a + 1, 2 wy + 1, 2 wx + 1) uint32 scores, MatchResult) of the last match: entry [k + n_a, j + wy, i + wx]."""
        res = MatchResult()
        out = np.empty(getattr(self, "_match_shape", (0, 0, 0)), dtype=np.uint32)
        self._check(self._lib.cm_map_match_copy(self._ctx, out.ctypes.data, out.size, C.byref(res)), "cm_map_match_copy")
        return out, res

    def map_match_device(self):
        """(scores device pointer, MatchResult) of the same volume, owned by the context and valid until the next evaluate,
        update, integrate, merge or configure call."""
        ptr, res = C.c_void_p(), MatchResult()
        self._check(self._lib.cm_map_match_device(self._ctx, C.byref(ptr), C.byref(res)), "cm_map_match_device")
        return ptr.value, res

    def map_match_table(self):
        """(R * R + 1,) uint8: the field byte by squared distance in cells, as cm_map_match_configure built it."""
        n = C.c_uint64(0)
        st = self._lib.cm_map_match_table_copy(self._ctx, None, 0, C.byref(n))
        if st != CAPACITY:
            self._check(st, "cm_map_match_table_copy")
        out = np.empty(n.value, dtype=np.uint8)
        self._check(self._lib.cm_map_match_table_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(n)), "cm_map_match_table_copy")
        return out

    # ---- the localisation layer: a particle filter against the map, behind the cost layer (cm_map_mcl_configure / cm_map_mcl_update) ----
    def map_mcl_configure(self, n_particles=None, max_beams=256, range_cells=256, sigma=0.1, max_dist=0.5, tau=8.0, resample_frac=0.5,
                          always=False, seed=0):
        """Allocates the localisation layer behind the configured cost layer: n_particles particles scored with at most max_beams
        beams (the frame's distinct body cells within range_cells, thinned by a stride) against map_match_configure's field of
        sigma and max_dist; weights exp(-(A - acc) / (255 tau)); resampling when n_eff < resample_frac * n_particles, or after
        every update with always. n_particles None frees the layer."""
        if n_particles is None:
            self._check(self._lib.cm_map_mcl_configure(self._ctx, None), "cm_map_mcl_configure")
            return
        p = MclParams(int(n_particles), int(max_beams), int(range_cells), float(sigma), float(max_dist), float(tau), float(resample_frac),
                      MCL_RESAMPLE_ALWAYS if always else 0, int(seed) & (2**64 - 1))
        self._check(self._lib.cm_map_mcl_configure(self._ctx, C.byref(p)), "cm_map_mcl_configure")
        self._mcl_n = p.n_particles

    def map_mcl_init_pose(self, x, y, yaw, sd_x=0.0, sd_y=0.0, sd_yaw=0.0):
        """Draws the particles around a pose of the map's world frame with the three standard deviations (metres, radians)."""
        self._check(self._lib.cm_map_mcl_init_pose(self._ctx, x, y, yaw, sd_x, sd_y, sd_yaw), "cm_map_mcl_init_pose")

    def map_mcl_init_uniform(self):
        """Draws the particles uniformly over the free cells of the map's image, headings uniform over the turn."""
        self._check(self._lib.cm_map_mcl_init_uniform(self._ctx), "cm_map_mcl_init_uniform")

    def map_mcl_predict(self, d_fwd, d_left, d_yaw, sd_fwd=0.0, sd_left=0.0, sd_yaw=0.0):
        """Moves every particle by the vehicle-frame motion since the last predict, with noise of the three standard deviations."""
        self._check(self._lib.cm_map_mcl_predict(self._ctx, d_fwd, d_left, d_yaw, sd_fwd, sd_left, sd_yaw), "cm_map_mcl_predict")

    def map_mcl_update(self):
        """Scores the particles with the last frame, weighs them, estimates and resamples where due. Returns the MclInfo."""
        info = MclInfo()
        self._check(self._lib.cm_map_mcl_update(self._ctx, C.byref(info)), "cm_map_mcl_update")
        return info

    def map_mcl_particles(self):
        """(n_particles,) MCL_PARTICLE_DTYPE: the particles after the last call of the layer."""
        out = np.empty(getattr(self, "_mcl_n", 0), dtype=MCL_PARTICLE_DTYPE)
        self._check(self._lib.cm_map_mcl_copy(self._ctx, out.ctypes.data, out.shape[0]), "cm_map_mcl_copy")
        return out

    def map_mcl_weights(self):
        """((n_particles,) MCL_WEIGHT_DTYPE, MclInfo) of the last update, in the order of the particles it found."""
        info = MclInfo()
        out = np.empty(getattr(self, "_mcl_n", 0), dtype=MCL_WEIGHT_DTYPE)
        self._check(self._lib.cm_map_mcl_weights_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_mcl_weights_copy")
        return out, info

    def map_mcl_device(self):
        """(particles device pointer, weights device pointer, MclInfo), owned by the context and valid until the next call of the
        layer or configure call."""
        parts, wts, info = C.c_void_p(), C.c_void_p(), MclInfo()
        self._check(self._lib.cm_map_mcl_device(self._ctx, C.byref(parts), C.byref(wts), C.byref(info)), "cm_map_mcl_device")
        return parts.value, wts.value, info

    def map_mcl_beam_configure(self, over_cells=8, sigma=0.1, z_hit=0.75, z_short=0.125, z_rand=0.125, plain=False):
        """Switches the localisation layer's beam model on: an update then casts a ray from every particle towards every beam's
        end cell and over_cells past it and scores where the first occupied cell lies (a Gaussian of sigma metres about the
        end weighted z_hit, z_short for what lies behind the end, z_rand everywhere). plain walks cell by cell instead of
        jumping. over_cells None goes back to the field score."""
        if over_cells is None:
            self._check(self._lib.cm_map_mcl_beam_configure(self._ctx, None), "cm_map_mcl_beam_configure")
            return
        p = MclBeamParams(int(over_cells), float(sigma), float(z_hit), float(z_short), float(z_rand), MCL_BEAM_PLAIN if plain else 0)
        self._check(self._lib.cm_map_mcl_beam_configure(self._ctx, C.byref(p)), "cm_map_mcl_beam_configure")

    def map_mcl_hyp_configure(self, bin_m=0.5, heading_bits=5, max_hyp=8, inject_max=0, alpha_slow=0.05, alpha_fast=0.5, kld_err=0.05, kld_z=2.326):
        """Switches the localisation layer's hypotheses on: every update then bins the particles (bin_m metres, 2^heading_bits
        heading bins), reports the connected components of the occupied bins by weight (map_mcl_hypotheses) and, with
        inject_max > 0, replaces up to that many particles by random ones while the fast average of the score lies below the
        slow one. bin_m None switches the mode off."""
        if bin_m is None:
            self._check(self._lib.cm_map_mcl_hyp_configure(self._ctx, None), "cm_map_mcl_hyp_configure")
            return
        p = MclHypParams(int(round(float(bin_m) * 1024.0)), int(heading_bits), int(max_hyp), int(inject_max), float(alpha_slow), float(alpha_fast),
                         float(kld_err), float(kld_z), 0, 0)
        self._check(self._lib.cm_map_mcl_hyp_configure(self._ctx, C.byref(p)), "cm_map_mcl_hyp_configure")

    def map_mcl_hypotheses(self):
        """(list of MclHyp, MclHypInfo) of the last update, which ran the hypotheses: the heaviest component first."""
        info = MclHypInfo()
        buf = (MclHyp * MCL_HYP_MAX)()
        self._check(self._lib.cm_map_mcl_hyp_copy(self._ctx, buf, MCL_HYP_MAX, C.byref(info)), "cm_map_mcl_hyp_copy")
        return [buf[k] for k in range(info.n_hyp)], info

    def map_mcl_beam_info(self):
        """The MclBeamInfo of the last update, which ran the beam model."""
        info = MclBeamInfo()
        self._check(self._lib.cm_map_mcl_beam_info_copy(self._ctx, C.byref(info)), "cm_map_mcl_beam_info_copy")
        return info

    # ---- the cast layer: expected ranges from many poses in the map, behind the cost layer (cm_map_cast_configure / cm_map_cast_evaluate) ----
    def map_cast_configure(self, max_poses=None, n_bearings=360, range_cells=256, plain=False, bearings=None):
        """Allocates the cast layer behind the configured cost layer: at most max_poses poses per evaluate, n_bearings rays per
        pose of at most range_cells cells; bearings are binary angles (a full turn is 2^32) added to a pose's heading, None
        spaces them evenly. plain walks cell by cell through the image; otherwise the walk skips by the distance field, with
        the same result. max_poses None frees the layer."""
        if max_poses is None:
            self._check(self._lib.cm_map_cast_configure(self._ctx, None, None), "cm_map_cast_configure")
            return
        b = None
        if bearings is not None:
            b = np.ascontiguousarray(np.asarray(bearings, dtype=np.uint64) & 0xFFFFFFFF, dtype=np.uint32).reshape(-1)
            if b.shape[0] != int(n_bearings):
                raise ValueError("bearings must hold n_bearings binary angles")
        p = CastParams(int(max_poses), int(n_bearings), int(range_cells), CAST_PLAIN if plain else 0)
        self._check(self._lib.cm_map_cast_configure(self._ctx, C.byref(p), b.ctypes.data if b is not None else None), "cm_map_cast_configure")
        self._cast_cap = p.max_poses * p.n_bearings

    def map_cast(self, poses):
        """Casts n_bearings rays from every pose. poses: a CAST_POSE_DTYPE array, or (n, 3) rows of x, y (metres, the map's
        world frame) and yaw (radians, converted by cast_heading). Returns the CastInfo."""
        if isinstance(poses, np.ndarray) and poses.dtype == CAST_POSE_DTYPE:
            q = np.ascontiguousarray(poses).reshape(-1)
        else:
            rows = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
            q = np.empty(rows.shape[0], dtype=CAST_POSE_DTYPE)
            q["x"], q["y"] = rows[:, 0], rows[:, 1]
            q["h"] = [cast_heading(v) for v in rows[:, 2]]
        info = CastInfo()
        self._check(self._lib.cm_map_cast_evaluate(self._ctx, q.ctypes.data if q.shape[0] else None, q.shape[0], C.byref(info)), "cm_map_cast_evaluate")
        return info

    def map_cast_particles(self):
        """Casts from the localisation layer's current particles in place. Returns the CastInfo."""
        info = CastInfo()
        self._check(self._lib.cm_map_cast_evaluate_mcl(self._ctx, C.byref(info)), "cm_map_cast_evaluate_mcl")
        return info

    def map_cast_rays(self):
        """((n_poses, n_bearings) CAST_RAY_DTYPE, CastInfo) of the last evaluate."""
        info = CastInfo()
        out = np.empty(getattr(self, "_cast_cap", 0), dtype=CAST_RAY_DTYPE)
        self._check(self._lib.cm_map_cast_copy(self._ctx, out.ctypes.data, out.shape[0], C.byref(info)), "cm_map_cast_copy")
        return out[: info.n_poses * info.n_bearings].reshape(info.n_poses, info.n_bearings), info

    def map_cast_ranges(self, cell=None):
        """((n_poses, n_bearings) float64 metric ranges cell * sqrt(jx^2 + jy^2), the rays, CastInfo) of the last evaluate; a ray
        without an origin has range 0. cell None: the cell map_configure was given."""
        rays, info = self.map_cast_rays()
        cell = float(self._map_cell if cell is None else cell)
        return cell * np.sqrt(rays["jx"].astype(np.float64) ** 2 + rays["jy"].astype(np.float64) ** 2), rays, info

    def map_cast_device(self):
        """(rays device pointer, CastInfo), owned by the context and valid until the next evaluate or configure call."""
        rays, info = C.c_void_p(), CastInfo()
        self._check(self._lib.cm_map_cast_device(self._ctx, C.byref(rays), C.byref(info)), "cm_map_cast_device")
        return rays.value, info

    # ---- branch-and-bound scan matching over wide windows, behind the cost layer (cm_map_match_search_configure / cm_map_match_search) ----
    def map_match_search_configure(self, sigma=None, max_dist=0.5, n_a=0, a_stride=1, wx=0, wy=0, depth=0, max_nodes=1 << 16, max_cells=1 << 16,
                                   subcell=False):
        """Allocates the search layer behind the configured cost layer: map_match_configure's field and angle candidates, shifts
        -wx..wx and -wy..wy cells of up to MATCH_SEARCH_MAX_SHIFT, roots at level depth, room for max_nodes nodes per level and
        max_cells cells per candidate. sigma None frees the layer."""
        if sigma is None:
            self._check(self._lib.cm_map_match_search_configure(self._ctx, None), "cm_map_match_search_configure")
            return
        p = MatchSearchParams(float(sigma), float(max_dist), int(n_a), int(a_stride), int(wx), int(wy), int(depth), int(max_nodes), int(max_cells),
                              MATCH_SUBCELL if subcell else 0)
        self._check(self._lib.cm_map_match_search_configure(self._ctx, C.byref(p)), "cm_map_match_search_configure")

    def map_match_search(self, pose):
        """Matches the last frame against the map around the prior pose (3 x 4, row-major) by branch and bound. Returns
        (MatchResult, MatchSearchInfo). A capacity overflow raises CloudMergeError with status CAPACITY and the info as its
        `info` attribute."""
        p = np.ascontiguousarray(pose, dtype=np.float32).reshape(12)
        out, info = MatchResult(), MatchSearchInfo()
        try:
            self._check(self._lib.cm_map_match_search(self._ctx, p.ctypes.data, C.byref(out), C.byref(info)), "cm_map_match_search")
        except CloudMergeError as e:
            e.info = info if e.status == CAPACITY else None
            raise
        return out, info

    def map_match_search_result(self):
        """(MatchResult, MatchSearchInfo) of the last search again."""
        out, info = MatchResult(), MatchSearchInfo()
        self._check(self._lib.cm_map_match_search_result(self._ctx, C.byref(out), C.byref(info)), "cm_map_match_search_result")
        return out, info

    def map_match_search_level(self, h):
        """(ny + 2^h - 1, nx + 2^h - 1) uint8: level h of the last search's pyramid; entry [y + 2^h - 1, x + 2^h - 1] is the
        largest field byte of the 2^h x 2^h cells from (x, y) on."""
        dims = (C.c_uint32 * 2)()
        st = self._lib.cm_map_match_search_level_copy(self._ctx, int(h), None, 0, C.byref(dims))
        if st != CAPACITY:
            self._check(st, "cm_map_match_search_level_copy")
        out = np.empty((dims[1], dims[0]), dtype=np.uint8)
        self._check(self._lib.cm_map_match_search_level_copy(self._ctx, int(h), out.ctypes.data, out.size, C.byref(dims)), "cm_map_match_search_level_copy")
        return out

    # ---- normals and curvature of the last result (cm_result_normals) ----
    def normals(self, k, viewpoint=(0.0, 0.0, 0.0), search_cell=0.0):
        """(n_out,) VOXEL_NORMAL_DTYPE array: entry i belongs to result record i (pcl::NormalEstimation with setKSearch(k),
        neighbours by (distance, result index), turned towards the viewpoint)."""
        p = NormalParams(int(k), (C.c_float * 3)(*[float(v) for v in viewpoint]), float(search_cell), 0)
        _, n_out = self.result_device()
        out = np.empty(max(int(n_out), 1), dtype=VOXEL_NORMAL_DTYPE)
        self._check(self._lib.cm_result_normals(self._ctx, C.byref(p), out.ctypes.data, out.shape[0]), "cm_result_normals")
        return out[: int(n_out)].copy()

    def normals_device(self, k, viewpoint=(0.0, 0.0, 0.0), search_cell=0.0):
        """(device pointer, entries) of the same table, owned by the context and valid until the next merge or the next call."""
        p = NormalParams(int(k), (C.c_float * 3)(*[float(v) for v in viewpoint]), float(search_cell), 0)
        ptr, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.cm_result_normals_device(self._ctx, C.byref(p), C.byref(ptr), C.byref(n)), "cm_result_normals_device")
        return ptr.value, n.value

    # ---- registration of a cloud against the last result (cm_result_align) ----
    @staticmethod
    def align_params(max_corr_dist, guess=None, max_iterations=30, normals_k=10, trans_eps=1e-6, rot_eps=1e-6,
                     min_correspondences=6):
        g = np.eye(3, 4) if guess is None else np.asarray(guess, np.float64).reshape(3, 4)
        return AlignParams(float(max_corr_dist), int(max_iterations), int(normals_k), int(min_correspondences), float(trans_eps),
                           float(rot_eps), (C.c_double * 12)(*g.ravel().tolist()))

    def align(self, source, max_corr_dist, guess=None, max_iterations=30, normals_k=10, trans_eps=1e-6, rot_eps=1e-6,
              min_correspondences=6):
        """Point-to-plane ICP of `source` — (n, 3) or (n, 4) float32, or a structured XYZI array as result() returns — against
        the last result: an AlignResult (pose_matrix() maps source coordinates onto the result). max_iterations 0 evaluates
        the guess alone: nearest neighbours (align_correspondences) and fitness."""
        src = np.asarray(source)
        if len(src) == 0:
            rec = np.zeros((0, 4), np.float32)
        elif src.dtype.names:
            rec = np.ascontiguousarray(src).view(np.float32).reshape(len(src), -1)[:, :4]
        else:
            src = np.asarray(src, np.float32).reshape(len(src), -1)
            rec = np.zeros((len(src), 4), np.float32)
            rec[:, :min(src.shape[1], 4)] = src[:, :4]
        rec = np.ascontiguousarray(rec, np.float32)
        p = self.align_params(max_corr_dist, guess, max_iterations, normals_k, trans_eps, rot_eps, min_correspondences)
        out = AlignResult()
        self._check(self._lib.cm_result_align(self._ctx, C.byref(p), rec.ctypes.data if len(rec) else None, len(rec), C.byref(out)),
                    "cm_result_align")
        return out

    def align_device(self, src_ptr, n_src, max_corr_dist, **kw):
        """The same with n_src 16-byte records already in device memory."""
        p = self.align_params(max_corr_dist, **kw)
        out = AlignResult()
        self._check(self._lib.cm_result_align_device(self._ctx, C.byref(p), C.c_void_p(src_ptr), int(n_src), C.byref(out)),
                    "cm_result_align_device")
        return out

    def align_correspondences(self, n):
        """(n,) ALIGN_CORR_DTYPE array of the last align call's final evaluation: entry i belongs to source record i."""
        out = np.zeros(max(int(n), 1), dtype=ALIGN_CORR_DTYPE)
        got = C.c_uint64()
        self._check(self._lib.cm_align_correspondences_copy(self._ctx, out.ctypes.data, int(n), C.byref(got)),
                    "cm_align_correspondences_copy")
        return out[: got.value].copy()

    # ---- NDT registration of a cloud against the last result's covariance table (cm_result_ndt_align) ----
    @staticmethod
    def ndt_params(guess=None, neighborhood=7, outlier_ratio=0.55, max_iterations=30, cov_min_points=6, cov_eig_mult=0.01,
                   trans_eps=1e-6, rot_eps=1e-6, min_correspondences=6):
        g = np.eye(3, 4) if guess is None else np.asarray(guess, np.float64).reshape(3, 4)
        return NdtParams(float(outlier_ratio), int(neighborhood), int(max_iterations), int(min_correspondences),
                         CovParams(int(cov_min_points), float(cov_eig_mult)), float(trans_eps), float(rot_eps),
                         (C.c_double * 12)(*g.ravel().tolist()))

    def ndt_align(self, source, guess=None, neighborhood=7, outlier_ratio=0.55, max_iterations=30, cov_min_points=6,
                  cov_eig_mult=0.01, trans_eps=1e-6, rot_eps=1e-6, min_correspondences=6):
        """NDT registration of `source` — (n, 3) or (n, 4) float32, or a structured XYZI array as result() returns — against
        the last result's voxel statistics (voxel_covariance at cov_min_points / cov_eig_mult): an NdtResult (pose_matrix()
        maps source coordinates onto the result). max_iterations 0 evaluates the guess alone (ndt_correspondences, score)."""
        src = np.asarray(source)
        if len(src) == 0:
            rec = np.zeros((0, 4), np.float32)
        elif src.dtype.names:
            rec = np.ascontiguousarray(src).view(np.float32).reshape(len(src), -1)[:, :4]
        else:
            src = np.asarray(src, np.float32).reshape(len(src), -1)
            rec = np.zeros((len(src), 4), np.float32)
            rec[:, :min(src.shape[1], 4)] = src[:, :4]
        rec = np.ascontiguousarray(rec, np.float32)
        p = self.ndt_params(guess, neighborhood, outlier_ratio, max_iterations, cov_min_points, cov_eig_mult, trans_eps, rot_eps,
                            min_correspondences)
        out = NdtResult()
        self._check(self._lib.cm_result_ndt_align(self._ctx, C.byref(p), rec.ctypes.data if len(rec) else None, len(rec),
                                                  C.byref(out)), "cm_result_ndt_align")
        return out

    def ndt_align_device(self, src_ptr, n_src, **kw):
        """The same with n_src 16-byte records already in device memory."""
        p = self.ndt_params(**kw)
        out = NdtResult()
        self._check(self._lib.cm_result_ndt_align_device(self._ctx, C.byref(p), C.c_void_p(src_ptr), int(n_src), C.byref(out)),
                    "cm_result_ndt_align_device")
        return out

    def ndt_correspondences(self, n):
        """(n,) NDT_CORR_DTYPE array of the last ndt_align call's final evaluation: entry i belongs to source record i."""
        out = np.zeros(max(int(n), 1), dtype=NDT_CORR_DTYPE)
        got = C.c_uint64()
        self._check(self._lib.cm_ndt_correspondences_copy(self._ctx, out.ctypes.data, int(n), C.byref(got)),
                    "cm_ndt_correspondences_copy")
        return out[: got.value].copy()

    # ---- statistical outlier removal before the voxel grid (cm_set_statistical_outlier) ----
    def set_statistical_outlier(self, mean_k, std_mul=1.0, search_cell=0.0):
        """mean_k None switches the stage off; takes effect with the next merge."""
        if mean_k is None:
            self._check(self._lib.cm_set_statistical_outlier(self._ctx, None), "cm_set_statistical_outlier")
            return
        p = SorParams(int(mean_k), float(std_mul), float(search_cell), 0)
        self._check(self._lib.cm_set_statistical_outlier(self._ctx, C.byref(p)), "cm_set_statistical_outlier")

    def sor_stats(self):
        """SorStats of the last waited-for frame: n_valid, n_removed, mean, stddev, threshold."""
        s = SorStats()
        self._check(self._lib.cm_get_sor_stats(self._ctx, C.byref(s)), "cm_get_sor_stats")
        return s

    def sor_distances(self, capacity):
        """float32 d_i of the stage's input in (sensor, point) order."""
        out = np.zeros(max(int(capacity), 1), dtype=np.float32)
        n = C.c_uint64()
        self._check(self._lib.cm_sor_distances_copy(self._ctx, out.ctypes.data, int(capacity), C.byref(n)),
                    "cm_sor_distances_copy")
        return out[: n.value].copy()

    def stage_times(self):
        t = StageTimes()
        self._check(self._lib.cm_get_stage_times(self._ctx, C.byref(t)), "cm_get_stage_times")
        return [(t.name[i].value.decode(), float(t.ms[i])) for i in range(t.n_stages)]
