/*
 * cloudmerge.h — C-ABI of the MI355X merge → voxel-grid library (libcloudmerge_hip.so).
 *
 * Drop-in boundary for ONE path of timspilak/cloud_merger: per-frame rigid transform of every
 * sensor cloud into the common frame, optional AABB crop, concatenation across sensors and the
 * PCL-VoxelGrid downsample.  The reference has no FFI layer for this path; its seam is the set of
 * free functions and third-party calls cited per entry point below (all file:line references are
 * into /root/reference/pcl_preprocessing/src/).  INTEGRATION.md shows the binding a maintainer of
 * the reference node adds around these calls.
 *
 * Conventions: plain pointers and sizes only; every function returns a cm_status (never throws);
 * the caller owns all host buffers; results live in the context until the next merge.
 * Threading: cm_submit_cloud* may be called concurrently for DIFFERENT sensor slots (the
 * reference's six subscriber threads, pc_preprocessing_main.cpp:513-525); cm_merge_voxelize* /
 * cm_wait / cm_result_* from one consumer thread (the reference's 10 Hz main loop, :549-584).
 * There is no CPU fallback: cm_create fails with CM_NO_DEVICE / CM_HIP_ERROR without a gfx950 GPU.
 */
#ifndef CLOUDMERGE_H
#define CLOUDMERGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define CM_API __attribute__((visibility("default")))
#else
#define CM_API
#endif

#define CM_VERSION 100            /* 0.1.0 */
#define CM_MAX_SENSORS 16
#define CM_NO_FIELD 0xFFFFFFFFu   /* off_i: the cloud has no intensity field (treated as 0) */

typedef struct cm_ctx cm_ctx;

typedef enum cm_status {
    CM_OK = 0,
    CM_EMPTY_INPUT = 1,    /* no point survived: PCL VoxelGrid returns width = height = 0 */
    CM_GRID_OVERFLOW = 2,  /* PCL's int32 index guard tripped: output = merged input, unvoxelised */
    CM_NOT_READY = 3,      /* a required sensor has no fresh cloud: the reference skips the tick (:134,:575) */
    CM_SKIPPED = 4,        /* cm_submit_cloud*: this sensor already holds an unconsumed cloud and the policy is
                              "first since the last fuse wins" (:330): the new one was dropped */
    CM_BAD_ARG = -1,
    CM_HIP_ERROR = -2,
    CM_NO_DEVICE = -3,
    CM_CAPACITY = -4,      /* more points than cm_limits allows, or the outlier stage's radius grid does not fit */
    CM_INTERNAL = -5
} cm_status;

/* cm_limits.flags */
#define CM_FLAG_PROFILE        0x1u  /* record a HIP event pair around every kernel (cm_get_stage_times) */
#define CM_FLAG_LATEST_WINS    0x2u  /* a newer cloud replaces an unconsumed one; default is the
                                        reference's "first cloud since the last fuse wins" (:330,:356,...) */
#define CM_FLAG_OCCUPANCY      0x4u  /* also keep (voxel index, point count) per output voxel for
                                        cm_result_copy_cells (+8 B of HBM writes per voxel) */

typedef struct cm_limits {
    uint32_t max_sensors;          /* 1..CM_MAX_SENSORS */
    uint32_t flags;
    uint64_t max_points_total;     /* per frame, summed over sensors (< 2^30) */
} cm_limits;

/* Runtime form of the reference's compile-time constants (Parameter.h:27-35) and of the
 * VoxelGrid settings at pc_preprocessing_main.cpp:173-175. */
typedef struct cm_params {
    float leaf[3];                 /* setLeafSize(v,v,v) :173; Parameter.h:28 */
    uint32_t min_points_per_voxel; /* setMinimumPointsNumberPerVoxel :175; Parameter.h:27 */
    int32_t downsample_all_data;   /* setDownsampleAllData(true) :174 */
    int32_t crop_enable;           /* getROI :20-40 */
    float crop_min[3];             /* x,y,z closed interval; Parameter.h:31-35 */
    float crop_max[3];
    uint32_t required_sensor_mask; /* bit s: sensor s must be fresh (:134); 0 = all submitted */
    /* pcl::RadiusOutlierRemoval on the fused cloud before VoxelGrid (my_cloud_fusion/src/
     * CloudFusionNode.h:74-85, called at cloud_fusion_node.cpp:72; live node outlierRemoval :184-192;
     * SURVEY.md §8f rank 2). A point stays iff more than outlier_min_neighbors points (itself
     * included) lie within outlier_radius (fp32 squared distance < float(r*r)). */
    int32_t outlier_enable;
    float outlier_radius;          /* setRadiusSearch; Parameter.h:23 (0.15), my_cloud_fusion Parameter.h:15 (0.1) */
    uint32_t outlier_min_neighbors;/* setMinNeighborsInRadius; Parameter.h:24 (1) */
} cm_params;

typedef struct cm_result {
    int32_t status;                /* cm_status of the frame */
    uint32_t n_sensors;            /* sensors that contributed */
    uint64_t n_in;                 /* points submitted */
    uint64_t n_merged;             /* after transform + crop (+ non-finite drop) */
    uint64_t n_out;                /* voxels written (or n_merged on CM_GRID_OVERFLOW) */
    int32_t min_b[3], max_b[3], div_b[3];   /* PCL's min_b_/max_b_/div_b_ (crop-box grid when
                                               bounds_from_crop) */
    float min_p[3], max_p[3];      /* getMinMax3D of the merged cloud (unset when bounds_from_crop) */
    uint32_t bounds_from_crop;     /* 1: grid origin taken from the crop box (same occupancy and
                                      order; the data min/max pass was skipped) */
    uint32_t key_bits;             /* bits of the linear voxel index */
    uint32_t sort_passes;          /* 8-bit radix passes over the whole frame that were run */
    uint32_t path_flags;           /* CM_PATH_* bits: how the frame was computed (same results either way) */
    float device_ms;               /* first kernel start -> last kernel end (CM_FLAG_PROFILE) */
} cm_result;

#define CM_PATH_LDS_RANK 1u    /* radix ranking by lane-ordered LDS adds (device probe at cm_create passed);
                                  otherwise ballot matching */
#define CM_PATH_BUCKET 2u      /* bucket path: point records sorted by the high index bits in sort_passes
                                  passes, the rest finished per bucket inside LDS (needs a box before the
                                  first point is read: the crop box or a predicted one) */
#define CM_PATH_PREDICTED 4u   /* ... the box was the previous frame's bounds plus a margin; every point was
                                  checked against it, min_b/max_b/div_b/min_p/max_p are the cloud's own */
#define CM_PATH_PACKED 16u    /* bucket path, crop box that dropped most of the last frame's points: the survivors' records were
                                  packed while counting, so the raw clouds were read once instead of twice */
#define CM_PATH_SPLIT 32u      /* bucket path, finish by k3_local + k3_compact (tiles stage their centroids, a second launch
                                  packs them: no look-back between tiles); otherwise k2_local. Summation order: a voxel of up
                                  to 17 points is added one point after the other in (sensor, point) order — pcl::VoxelGrid's
                                  own sum, bit for bit given that tie order; a longer one may be finished 64 points per step in
                                  a fixed tree order (deterministic, within 1e-4 m of the one-after-the-other sum, closer to the
                                  exact mean). CM_FINISH=v2 (k2_local) adds every voxel one after the other. */
#define CM_PATH_QUANTILE 64u   /* bucket path, ONE global pass (sort_passes == 1) into buckets cut at the quantiles of the previous
                                  frame's sorted records (same grid), one finish workgroup per bucket; bucket sizes are verified
                                  on the device, a frame whose buckets outgrew the finish is redone with the fixed-grid passes
                                  (CM_PATH_REDONE). The points of a voxel are added in the same (sensor, point) order: same results */
#define CM_PATH_REDONE 8u      /* the bucket path gave the frame back and it was computed a second time inside cm_wait: after
                                  a point outside the predicted box on the bucket path again, in a box around the bounds the
                                  first attempt measured (CM_PATH_BUCKET | CM_PATH_PREDICTED stay set); after a bucket too large
                                  for LDS, or more survivors of the crop than the last frame promised, on the general path */

#define CM_PATH_MOTION 128u    /* the frame's points were motion-compensated (cm_set_ego_motion) before anything else read them */
#define CM_PATH_SOR 256u       /* statistical outlier removal (cm_set_statistical_outlier) chose the points the voxel grid saw */

#define CM_MAX_STAGES 48
typedef struct cm_stage_times {
    uint32_t n_stages;
    uint32_t _pad;
    char name[CM_MAX_STAGES][24];  /* kernel name */
    float ms[CM_MAX_STAGES];       /* duration of that launch in the last profiled frame */
} cm_stage_times;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* Allocates the context, its stream and HBM work buffers on `device`. */
CM_API int cm_create(cm_ctx** out, int device, const cm_limits* limits);
CM_API int cm_destroy(cm_ctx* ctx);
/* Run on a caller-owned hipStream_t (NULL: back to the context's own stream). A handle of 0 is NULL: it does NOT name the
 * legacy default stream. torch.cuda.current_stream().cuda_stream is 0 on torch's default stream, so passing it selects the
 * context's own stream, which is non-blocking and therefore not ordered behind the default stream: a caller on the default
 * stream synchronises by hand (or creates a stream and passes that). Refused while a frame is in flight. */
CM_API int cm_set_stream(cm_ctx* ctx, void* hip_stream);

/* ---- static transforms: replaces tf::Transform(stf.getRotation(), stf.getOrigin()) (:320,:346,
 * :371,:397,:424,:463) and the tf->Eigen conversion inside pcl_ros::transformPointCloud --------- */
/* q/t are what tf::Transform::getRotation()/getOrigin() return (doubles). Converted on the host
 * exactly as Eigen::Quaternionf::toRotationMatrix does in fp32. */
CM_API int cm_set_sensor_transform(cm_ctx* ctx, uint32_t sensor, const double q_xyzw[4], const double t_xyz[3]);
/* Row-major 3x4 fp32 [R|t], used verbatim. */
CM_API int cm_set_sensor_matrix(cm_ctx* ctx, uint32_t sensor, const float m[12]);
CM_API int cm_get_sensor_matrix(cm_ctx* ctx, uint32_t sensor, float m[12]);

/* ---- ingest: replaces the subscriber callbacks' deserialise + transformPointCloud + getROI
 * (:318-337 and siblings); the arithmetic itself runs inside cm_merge_voxelize ---------------- */
/* Copies a sensor_msgs/PointCloud2 payload (n * point_step bytes, FLOAT32 fields at the given
 * byte offsets) into the sensor's HBM slot. Returns after the caller's buffer may be reused.
 * Never waits for a merge: every slot has two HBM buffers, the frame enqueued last (and its by-products:
 * cm_merged_copy, cm_ground_copy) reads one, submits fill the other — the reference's callbacks run
 * beside its 10 Hz loop on AsyncSpinner(6) (:513, :318-337, :549-584). Callable from one thread per sensor. */
CM_API int cm_submit_cloud(cm_ctx* ctx, uint32_t sensor, const void* host_data, uint32_t n,
                    uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i);
/* The same without waiting for the copy either: the H2D transfer is enqueued on the slot's own stream and
 * the frame that consumes the cloud waits for it ON THE DEVICE. `host_data` must stay valid and unchanged
 * until that frame has been enqueued and cm_wait (or cm_sync) has returned; memory from cm_host_alloc makes
 * the transfer a true DMA that overlaps the previous frame's kernels. */
CM_API int cm_submit_cloud_async(cm_ctx* ctx, uint32_t sensor, const void* host_data, uint32_t n,
                    uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i);
/* Zero-copy variant: `dev_data` is already resident in HBM and stays valid until the merge that
 * consumes it has completed. */
CM_API int cm_submit_cloud_device(cm_ctx* ctx, uint32_t sensor, const void* dev_data, uint32_t n,
                           uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i);
/* Forget a sensor's cloud (fresh or stale). */
CM_API int cm_clear_sensor(cm_ctx* ctx, uint32_t sensor);

/* ---- the path: replaces fusePointclouds (:131-160) + voxelgrid (:168-177) -------------------- */
/* Synchronous: enqueue, wait, fill `res`. Returns res->status. */
CM_API int cm_merge_voxelize(cm_ctx* ctx, const cm_params* p, cm_result* res);
/* Enqueue only (no host wait); pair with cm_wait. Returns CM_OK / CM_NOT_READY / error. */
CM_API int cm_merge_voxelize_async(cm_ctx* ctx, const cm_params* p);
CM_API int cm_wait(cm_ctx* ctx, cm_result* res);

/* ---- results: replaces pcl::toROSMsg of the voxel cloud (:215-216) --------------------------- */
/* Copies the n_out output points to host memory: point_step_out 16 (x,y,z,intensity) or 32 (the
 * pcl::PointXYZI image pcl::toROSMsg puts on the wire: x,y,z,1.0f,intensity,0,0,0). */
CM_API int cm_result_copy(cm_ctx* ctx, void* host_dst, uint64_t capacity_points, uint32_t point_step_out);
/* The same (16-byte records only) without waiting: the copy is enqueued behind the frame on the context's
 * stream; `host_dst` (cm_host_alloc memory for a true DMA) is complete when cm_sync returns. The next frame
 * may be enqueued right away (stream order keeps it off the result until the copy has read it). */
CM_API int cm_result_copy_async(cm_ctx* ctx, void* host_dst, uint64_t capacity_points);
/* Pipelined publish (the loop body of the reference publishes every tick, pc_preprocessing_main.cpp:199-220, :574-577): the
 * copy-out of the LAST WAITED-FOR frame — 16-byte records or the 32-byte pcl::PointXYZI images — is enqueued on a stream of
 * its own, and the next frame may be enqueued right away: its kernels run BESIDE the copy (the result buffers exist twice;
 * a frame only waits, on the device, for the copy that read the buffers it is about to write, i.e. the one of two frames
 * ago). `host_dst` — cm_host_alloc memory, or any buffer made DMA-able with cm_host_register — is complete when
 * cm_publish_wait (or cm_sync) returns. Call between cm_wait and the next cm_merge_voxelize_async. */
CM_API int cm_result_publish_async(cm_ctx* ctx, void* host_dst, uint64_t capacity_points, uint32_t point_step_out);
CM_API int cm_publish_wait(cm_ctx* ctx);
/* Waits for everything enqueued on the context's streams. */
CM_API int cm_sync(cm_ctx* ctx);
/* Device pointer of the compact 16-byte result records (valid until the next merge). */
CM_API int cm_result_device(cm_ctx* ctx, const void** dev_ptr, uint64_t* n_points);
/* Occupancy of the last CM_OK frame (needs CM_FLAG_OCCUPANCY): absolute voxel cell (i,j,k) and
 * point count of every output voxel, in output order. Either pointer may be NULL. */
CM_API int cm_result_copy_cells(cm_ctx* ctx, int32_t* ijk_host, uint32_t* counts_host, uint64_t capacity_voxels);
/* The merged (transformed + cropped + concatenated) cloud of the last frame as 16-byte
 * x,y,z,intensity records in sensor order — the reference's fused cloud (:137-142). */
CM_API int cm_merged_copy(cm_ctx* ctx, void* host_dst, uint64_t capacity_points, uint64_t* n_points);

/* ---- diagnostics --------------------------------------------------------------------------- */
/* Per-frame figures of the last frame that was waited for — what the reference logs per callback
 * (ROS_INFO of the cloud sizes, :334,:360,:386,:413,:452,:505) plus the bytes that moved. */
typedef struct cm_frame_stats {
    uint32_t n_sensors;                    /* sensors fused into the frame, in fuse order */
    uint32_t _pad;
    uint32_t sensor[CM_MAX_SENSORS];       /* the caller's sensor number */
    uint32_t n_in[CM_MAX_SENSORS];         /* points submitted */
    uint32_t n_kept[CM_MAX_SENSORS];       /* ... that were finite, inside the crop box and passed the pre-stages' masks,
                                              i.e. entered the voxel grid */
    uint32_t fresh[CM_MAX_SENSORS];        /* 1: a cloud submitted since the previous frame, 0: a stale one rode along (:141) */
    uint64_t generation[CM_MAX_SENSORS];   /* which accepted submit of that sensor the frame read (1 = its first; CM_SKIPPED ones
                                              do not count): a caller that counts its accepted submits knows exactly what was consumed */
    uint64_t bytes_h2d[CM_MAX_SENSORS];    /* payload bytes copied host -> HBM for this frame (0: device submit or stale) */
    uint64_t bytes_h2d_total, bytes_d2h_total;   /* d2h: result / merged / ground copies since the frame was enqueued */
    uint64_t bytes_algorithmic;            /* 16 B x points in + 16 B x voxels out */
} cm_frame_stats;
CM_API int cm_get_frame_stats(cm_ctx* ctx, cm_frame_stats* out);
CM_API int cm_get_stage_times(cm_ctx* ctx, cm_stage_times* out);
CM_API const char* cm_status_string(int status);
CM_API const char* cm_last_error(cm_ctx* ctx);
CM_API int cm_version(void);

/* ---- multi-GPU single fused cloud (nothing like it exists in the reference) ---
 * One process per GPU. Each rank voxelises ITS sensors into a partial table of per-voxel sums
 * (thresholding deferred: a voxel may hold one point on each of two GPUs), the host all-gathers the
 * tables (RCCL over xGMI), and the merge re-sorts the concatenated entries by voxel index, adds
 * them in rank order (deterministic), applies min_points_per_voxel and divides.
 * All ranks must index the SAME grid: the crop box fixes it when it fits PCL's int32 index;
 * otherwise pass the bounds of the whole fused cloud (cm_local_bounds on every rank, min/max
 * all-reduced by the host) as global_min_max = {min x,y,z, max x,y,z}. */
typedef struct cm_partial_entry {   /* 32 bytes */
    uint32_t key;                   /* linear voxel index in the shared grid (PCL order) */
    uint32_t count;
    float sx, sy, sz, si;           /* fp32 sums, stable point order */
    uint32_t _pad[2];
} cm_partial_entry;
/* fp32 min/max of this rank's transformed (+cropped) points; does not consume the clouds. */
CM_API int cm_local_bounds(cm_ctx* ctx, const cm_params* p, float min_xyz[3], float max_xyz[3], uint64_t* n_valid);
/* Like cm_merge_voxelize but stops before thresholding/division. res->n_out = table entries. */
CM_API int cm_merge_partial(cm_ctx* ctx, const cm_params* p, const float* global_min_max, cm_result* res);
CM_API int cm_partial_device(cm_ctx* ctx, const void** dev_entries, uint64_t* n_entries);
/* dst may be host or device memory (e.g. the send buffer of the all-gather). */
CM_API int cm_partial_copy(cm_ctx* ctx, cm_partial_entry* dst, uint64_t capacity);
/* Merge n_tables tables (16-byte aligned device pointers, rank order) into the context's result
 * buffer (cm_result_copy / cm_result_copy_cells read it; cells need the grid of the ranks'
 * cm_merge_partial results). Synchronous. res->n_merged = distinct voxels, res->n_out = kept. */
CM_API int cm_merge_tables(cm_ctx* ctx, const void* const* dev_tables, const uint64_t* n_entries,
                           uint32_t n_tables, const cm_params* p, cm_result* res);

/* ---- zone-wise ground removal before the fuse -------------------------------
 * What the live node does to every sensor's cloud between getROI and the fuse: proceedFront / proceedRear
 * (pc_preprocessing_main.cpp:228-312), the top-middle and Livox callbacks (:436-497) — the cropped cloud is
 * cut into x-slabs (getCloudPart :49-59), and in each slab removeGround (:71-122) takes the points of a z band,
 * fits one plane to them (RANSAC, Parameter.h:38-42) and calls its inliers ground; the rest of the band and the
 * part above it (up to z_keep_max) are "no ground". With this enabled the voxel grid (and cm_merged_copy) sees
 * the fused no-ground cloud (:137-142) and cm_ground_copy returns the fused ground cloud (:144-149).
 * Differences from the reference, all documented in DESIGN.md §10: RANSAC samples come from a counter-based
 * generator, not boost::mt19937 (planes agree statistically, not draw for draw); a point on the border of two
 * slabs goes to the first one only (the reference's closed intervals put it in both); points keep sensor order
 * (the reference concatenates slab by slab). The radius outlier filter that removeGround applies to the band's
 * non-ground points (:119) runs when outlier_radius > 0, among the points of the same slab, like there. */
#define CM_MAX_ZONES 8
typedef struct cm_zone {
    float x_min, x_length;         /* getCloudPart(cloud, part, length, deviation): x in [x_min, x_min + x_length] */
    float z_max_ground;            /* removeGround(.., -z, z, ..): band z in [-z, z]; negative: no ground removal,
                                      the slab is kept whole (top-middle's rear part, :440-441) */
} cm_zone;
typedef struct cm_ground_params {
    uint32_t max_iterations;       /* Parameter.h:38 (1000) */
    float distance_threshold;      /* :40 (0.3 m) */
    float probability;             /* :41 (0.99) */
    int32_t optimize_coefficients; /* :95 (true) */
    float z_keep_max;              /* roi_z_max (:35): the part above a band reaches from z_max_ground + 0.01 up to here (:91) */
    float outlier_radius;          /* > 0: RadiusOutlierRemoval on every band's non-ground points (:119, Parameter.h:23) */
    uint32_t outlier_min_neighbors;/* Parameter.h:24 */
    uint32_t _pad;
    uint64_t seed;                 /* of the sample generator */
    uint32_t n_zones[CM_MAX_SENSORS];
    cm_zone zones[CM_MAX_SENSORS][CM_MAX_ZONES];   /* in the order the reference processes them */
} cm_ground_params;
typedef struct cm_ground_plane {
    float plane[4];                /* a x + b y + c z + d = 0 */
    uint32_t band_points, inliers, iterations;
    int32_t found;
} cm_ground_plane;
/* NULL switches the stage off. Takes effect with the next cm_merge_voxelize; not combined with
 * cm_params.outlier_enable or cm_merge_partial. */
CM_API int cm_set_ground_removal(cm_ctx* ctx, const cm_ground_params* g);
/* Fused ground cloud of the last frame, 16-byte x,y,z,intensity records in (sensor, point) order. */
CM_API int cm_ground_copy(cm_ctx* ctx, void* host_dst, uint64_t capacity_points, uint64_t* n_points);
/* Planes of the last frame, indexed [sensor * CM_MAX_ZONES + zone]; capacity in entries. */
CM_API int cm_ground_planes(cm_ctx* ctx, cm_ground_plane* planes, uint32_t capacity);

/* ---- ego-motion compensation (deskew) before the merge (an extension: the reference has none) ----------------------
 * The merger otherwise fuses clouds as if every point were measured at one instant. With a twist set, every point of
 * sensor slot s measured at t = stamp_ns[s] + tau (tau: the point's own time field, 0 without one) is moved from the
 * vehicle frame of that instant into the vehicle frame at t_ref_ns, by the second-order expansion of exp(dt xi) for a
 * constant body twist xi = (v, w), dt = t - t_ref:
 *     q = M_s p,  c = w x q,  e = w x c,  k = w x v,  h = dt^2 / 2
 *     out = q + (dt (c + v) + h (e + k))      fp32, round-to-nearest, no contraction, in this order
 * with dt = dt0_s + tau in fp32, dt0_s = (float)((double)(stamp_ns[s] - t_ref_ns) * 1e-9). The difference of the two
 * stamps is taken modulo 2^64 and read as a signed 64-bit integer: stamps further apart than 2^63 ns wrap, they do not
 * overflow. A uint32 tau is converted to fp32 (round-to-nearest-even, the whole unsigned range) and multiplied by 1e-9f.
 * It runs as one pre-pass (k_motion) over all clouds of the frame, before the transform's consumers: the voxel grid, the
 * outlier and ground stages, cm_merged_copy, the CM_GRID_OVERFLOW fallback and a redo inside cm_wait all see the
 * compensated points. A point with a non-finite coordinate or time stays non-finite and is dropped as before.
 * Not combined with cm_local_bounds / cm_merge_partial (fused cloud across GPUs): they return CM_BAD_ARG while set. */
#define CM_TIME_NONE   0u   /* no per-point time: every point of the cloud is at its header stamp */
#define CM_TIME_F32_S  1u   /* float32 seconds relative to the header stamp (velodyne "time") */
#define CM_TIME_U32_NS 2u   /* uint32 nanoseconds relative to the header stamp (ouster "t") */
typedef struct cm_motion {
    float v[3];                        /* ego linear velocity, m/s, in the common frame */
    float w[3];                        /* ego angular velocity, rad/s, in the common frame */
    int64_t t_ref_ns;                  /* the instant the merged cloud is expressed at (the published stamp) */
    int64_t stamp_ns[CM_MAX_SENSORS];  /* header stamp of the cloud each sensor slot contributes (a stale one: its own) */
} cm_motion;
/* Per-point time field of a sensor's clouds: byte offset and CM_TIME_* type. Persistent per sensor, like the transform;
 * checked against each cloud's point_step when a frame is built (offset + 4 > point_step: that frame returns CM_BAD_ARG,
 * cm_last_error names the sensor, and the clouds stay fresh). */
CM_API int cm_set_sensor_time_field(cm_ctx* ctx, uint32_t sensor, uint32_t offset, uint32_t type);
/* The twist and stamps of the next frames; NULL switches compensation off. Takes effect with the next merge. Non-finite
 * v or w: CM_BAD_ARG. The compensated clouds' buffer (16 B per point of capacity) is allocated by the first non-NULL
 * call; if that fails the call returns CM_HIP_ERROR and compensation stays off. */
CM_API int cm_set_ego_motion(cm_ctx* ctx, const cm_motion* m);

/* ---- per-voxel covariance (NDT voxel statistics; an extension: the reference has none) ---------------------------
 * pcl::VoxelGridCovariance's statistics for every voxel of the last frame's result, computed on request after the frame
 * (DESIGN.md §12). Entry k belongs to cm_result_copy record k. With p_1..p_n the voxel's points in (sensor, point) order
 * (the order of cm_merged_copy), fp64, round-to-nearest, no contraction, sums taken one point after the other from 0:
 *     s_i = sum double(p_i),  S_ij = sum double(p_i) double(p_j),  m_i = s_i / n
 *     C_ij = ((S_ij - 2 (s_i m_j)) / n + m_i m_j) ((n - 1.0) / n)      i >= j, mirrored
 * The factor (n - 1) / n is PCL's (VoxelGridCovariance), not the textbook n / (n - 1). lambda_0 <= lambda_1 <= lambda_2 are the
 * eigenvalues of C. Valid: n >= min_points, lambda_0 >= 0, lambda_1 >= 0, lambda_2 > 0 and a finite inverse. Inflation
 * (Magnusson eq. 6.11): with mu = eig_mult lambda_2, lambda_0 < mu raises lambda_0 (and lambda_1 if below) to mu and C is rebuilt
 * as V diag(lambda) V^T (CM_COV_INFLATED). Outputs are rounded to fp32. Voxels below min_points keep an entry (count and mean
 * only, flags 0) so that the table lines up with the result; PCL leaves them out.
 * Refused with CM_BAD_ARG (cm_last_error says why): a context without CM_FLAG_OCCUPANCY, no result or a frame in flight, a
 * last status other than CM_OK, a result of cm_merge_partial / cm_merge_tables, min_points < 3, eig_mult outside [0, 1].
 * The table lives as long as the result (until the next merge); no later frame depends on whether it was asked for. */
typedef struct cm_cov_params {
    uint32_t min_points;               /* PCL's default 6, floor 3 */
    float eig_mult;                    /* PCL's default 0.01 */
} cm_cov_params;                       /* NULL: {6, 0.01f} */
#define CM_COV_VALID    1u
#define CM_COV_INFLATED 2u
typedef struct cm_voxel_cov {          /* 80 bytes */
    float mean[3];
    uint32_t count;
    float cov[6];                      /* (0,0) (1,0) (2,0) (1,1) (2,1) (2,2) of C, after inflation; zero below min_points */
    float icov[6];                     /* same order; zero unless valid */
    float evals[3];                    /* ascending, after inflation; zero unless valid */
    uint32_t flags;                    /* CM_COV_* */
} cm_voxel_cov;
/* The table copied to the host: capacity in entries (fewer than the result's voxels: CM_CAPACITY). */
CM_API int cm_result_voxel_cov(cm_ctx* ctx, const cm_cov_params* p, cm_voxel_cov* host_dst, uint64_t capacity);
/* The same table left in device memory owned by the context: *n entries of 80 bytes at *dev_ptr. */
CM_API int cm_result_voxel_cov_device(cm_ctx* ctx, const cm_cov_params* p, const void** dev_ptr, uint64_t* n);

/* ---- statistical outlier removal before the voxel grid (pcl::StatisticalOutlierRemoval) ----------------------------
 * PCL 1.8's StatisticalOutlierRemoval::applyFilterIndices restated (parity against libpcl is unpinned, as for
 * every other stage). The stage's input is the fused cloud after transform, crop, the non-finite drop and deskew when it is
 * on: P = p_1..p_n in (sensor, point) order, the order of cm_merged_copy.
 *   1. d2(q, p) = (dx*dx + dy*dy) + dz*dz, dx = q.x - p.x ..., fp32, round-to-nearest, no contraction, over every OTHER index
 *      (exact duplicates count, at distance 0).
 *   2. d_i: the k = mean_k smallest d2 of p_i, sqrtf of each correctly rounded, added in ascending order in fp64 from 0.0,
 *      d_i = float(sum / k).
 *   3. S = sum double(d_i), Q = sum double(fp32(d_i * d_i)), both exact and rounded once to fp64 (math.fsum; PCL adds in index
 *      order: a documented deviation that makes the result independent of launch geometry). fp64, no contraction:
 *      mean = S / n, var = (Q - S*S/n) / (n - 1), stddev = sqrt(var), threshold = mean + std_mul * stddev.
 *   4. p_i is removed iff double(d_i) > threshold (a NaN threshold, from a slightly negative variance, removes nothing).
 *   5. n <= mean_k: nothing is removed, d_i, mean and stddev are NaN, threshold is +inf. An empty input stays CM_EMPTY_INPUT.
 * The kept points go on in their order through the stage's keep-mask: cm_merged_copy, cm_result_*, cm_result_voxel_cov* and
 * cm_frame_stats.n_kept see the surviving cloud.
 * Refused at merge (CM_BAD_ARG, cm_last_error says why): with cm_params.outlier_enable, with ground removal, with
 * cm_merge_partial / cm_local_bounds. Deskew combines with it. */
#define CM_SOR_MAX_K 64
typedef struct cm_sor_params {
    uint32_t mean_k;       /* setMeanK, 1..CM_SOR_MAX_K */
    float std_mul;         /* setStddevMulThresh, finite (negative allowed) */
    float search_cell;     /* edge (m) of the search grid's cells: speed only, never the result; 0 = library's choice: the last
                              frame's mean distance, clamped to [0.05, 5] m, 0.5 m on the first frame. A cell whose grid
                              would exceed the row table or the 32-bit keys is doubled until it fits. The grid is over the
                              crop box when one is on, else over the cloud's own bounds; a crop box whose extent overflows
                              fp32 (e.g. +-2e38) fits no cell, and the grid is then over the cloud's own bounds as well. A
                              cloud whose own extent overflows fp32 is searched as one cell. */
    uint32_t _pad;
} cm_sor_params;
typedef struct cm_sor_stats {
    uint64_t n_valid, n_removed;
    double mean, stddev, threshold;
} cm_sor_stats;
/* NULL: off; takes effect with the next merge. Refused (CM_BAD_ARG): mean_k 0 or above 64, a non-finite std_mul, a negative or
 * non-finite search_cell. The stage's buffers are allocated by the first non-NULL call; if that fails the call returns
 * CM_HIP_ERROR and the stage stays off. */
CM_API int cm_set_statistical_outlier(cm_ctx* ctx, const cm_sor_params* p);
/* Figures of the last waited-for frame (of a frame without the stage: all zero). */
CM_API int cm_get_sor_stats(cm_ctx* ctx, cm_sor_stats* out);
/* d_i of the stage's input, in (sensor, point) order (n_valid entries): what the threshold was applied to. *n: the entries;
 * more than capacity: CM_CAPACITY. */
CM_API int cm_sor_distances_copy(cm_ctx* ctx, float* host_dst, uint64_t capacity, uint64_t* n);

/* ---- Euclidean cluster extraction on the result (pcl::EuclideanClusterExtraction; an extension) ----------------------
 * Obstacle segmentation of the cloud this library publishes, computed on request after a frame. Input: the
 * n_out records of the last result, c_0 .. c_{n-1} in the order of cm_result_copy, their x, y, z as fp32.
 *   1. Edge. i ~ j iff d2(c_i, c_j) < float(tolerance * tolerance), d2 = (dx*dx + dy*dy) + dz*dz, dx = c_i.x - c_j.x ..., fp32,
 *      round-to-nearest, no contraction: the distance and the strict < of the radius outlier stage. Symmetric bit for bit.
 *   2. Component. The connected components of that graph.
 *   3. Size filter. A component of m voxels is a cluster iff min_cluster_size <= m <= max_cluster_size. As in PCL the whole
 *      component is grown first and then kept or dropped as a whole. Sizes count voxels: points of the cloud being clustered.
 *   4. Numbering. The kept clusters are numbered 0, 1, ... by ascending smallest member index. (The one deviation: PCL then
 *      std::sorts its clusters by size, which is unstable for ties. The table carries the sizes; sort it if that order is
 *      wanted.)
 *   5. Outputs, owned by the context and valid until the next merge or the next call:
 *        labels[n_out]         entry k belongs to result record k: its cluster number, or CM_CLUSTER_NONE for a voxel whose
 *                              component the size filter dropped
 *        indices[n_clustered]  the member voxels grouped by cluster, ascending inside a cluster (PCL's
 *                              std::vector<PointIndices>, flattened)
 *        clusters[n_clusters]  one cm_cluster each: where its members start in indices, how many, the sum of their point
 *                              counts (context with CM_FLAG_OCCUPANCY; 0 without), and the axis-aligned box of the member
 *                              centroids (of two zeros of either sign, min takes -0 and max +0). No centroid: a floating
 *                              sum over a cluster depends on its order; min / max and integer sums do not.
 * The partition is independent of summation order and launch geometry. CM_FLAG_OCCUPANCY is not required.
 * Refused with CM_BAD_ARG (cm_last_error says why): a frame in flight, no result, a result of cm_merge_partial /
 * cm_merge_tables, a last status other than CM_OK (no voxel grid), a tolerance that is not finite and > 0 or whose fp32
 * square is 0 or not finite, min_cluster_size 0, min_cluster_size > max_cluster_size. A result in which no component
 * passes the filter is CM_OK with zero clusters and every label CM_CLUSTER_NONE. No later frame depends on whether the
 * tables were asked for; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists the stages of this call. */
#define CM_CLUSTER_NONE 0xFFFFFFFFu
typedef struct cm_cluster_params {
    float tolerance;                   /* setClusterTolerance, metres */
    uint32_t min_cluster_size;         /* setMinClusterSize, >= 1 */
    uint32_t max_cluster_size;         /* setMaxClusterSize */
    uint32_t _pad;
} cm_cluster_params;
typedef struct cm_cluster {            /* 40 bytes */
    uint32_t first;                    /* offset of the members in indices */
    uint32_t n_voxels;
    uint32_t n_points;                 /* sum of the members' point counts; 0 without CM_FLAG_OCCUPANCY */
    uint32_t _pad;
    float min[3], max[3];              /* box of the member centroids */
} cm_cluster;
/* Host copies; capacities in entries. A destination may be NULL with capacity 0 to skip it; one that is too small:
 * CM_CAPACITY (nothing is copied). *n_clusters / *n_clustered are always written (0 when the call is refused). */
CM_API int cm_result_clusters(cm_ctx* ctx, const cm_cluster_params* p, uint32_t* labels_host, uint64_t labels_capacity,
                              cm_cluster* clusters_host, uint64_t clusters_capacity, uint32_t* indices_host,
                              uint64_t indices_capacity, uint64_t* n_clusters, uint64_t* n_clustered);
/* The same three tables left in device memory owned by the context (n_out labels, *n_clusters entries of 40 bytes,
 * *n_clustered indices; a pointer is NULL where its table is empty). */
CM_API int cm_result_clusters_device(cm_ctx* ctx, const cm_cluster_params* p, const void** labels, const void** clusters,
                                     const void** indices, uint64_t* n_clusters, uint64_t* n_clustered);

/* ---- oriented bounding boxes of the clusters (search-based L-shape fitting; an extension) ------------------------------
 * A centre, a length, a width, a height and a heading per cluster, computed on request after a frame: every
 * heading in [0, pi/2) is tried, the rectangle it implies is scored, the best is kept (Zhang, Xu et al., IV 2017). The table
 * is a function of the result, the parameters and the direction table alone, bit for bit. All fp32 and fp64 operations are
 * rounded one at a time, round-to-nearest, no contraction.
 *   0. Directions. theta_a = double(a) * (1.5707963267948966 / double(n_angles)), a = 0 .. n_angles - 1;
 *      (ca, sa) = (float(cos theta_a), float(sin theta_a)), std::cos / std::sin on the host. cm_box_directions returns exactly
 *      the table the call uploads; that table is the definition. Entry 0 is (1, 0).
 *   1. Clusters. The call first computes the cluster tables at `cluster`, as cm_result_clusters does; afterwards the context
 *      holds those labels, indices and clusters. Cluster k has the members j_0 < j_1 < ... < j_{m-1} (its slice of indices)
 *      and the box min / max of the cluster table.
 *   2. Validity. ex = max[0] - min[0], ey = max[1] - min[1], fp32. The box is valid iff ex, ey and max[2] - min[2] are
 *      finite and ex, ey < CM_BOX_MAX_EXTENT. Otherwise flags = 0, angle = 0, every float field and score NaN. In a valid
 *      cluster nothing below overflows or becomes NaN.
 *   3. Projection of member j at angle a: dx = x_j - min[0], dy = y_j - min[1]; u = (dx*ca) + (dy*sa), v = (dy*ca) - (dx*sa).
 *      u0, u1, v0, v1: the minima and maxima of u and v over the members.
 *   4. Score. CM_BOX_AREA: score_a = -double((u1 - u0) * (v1 - v0)), the product in fp32. CM_BOX_CLOSENESS: per member
 *      d = max(min(min(u1 - u, u - u0), min(v1 - v, v - v0)), d_min) in fp32 and term = 1.0 / double(d). Member p of the
 *      cluster's list belongs to chunk p / CM_BOX_CHUNK; a chunk's terms are added one after the other from 0.0 in list
 *      order, the chunk sums one after the other from 0.0 in ascending chunk order; score_a is that total.
 *   5. Choice. a* is the smallest a with the largest score_a.
 *   6. Outputs, (ca, sa) and the extremes at a*: size = (u1 - u0, v1 - v0, max[2] - min[2]); uc = u0 + (u1 - u0) * 0.5f, vc
 *      likewise; center = (min[0] + ((uc*ca) - (vc*sa)), min[1] + ((uc*sa) + (vc*ca)), min[2] + (max[2] - min[2]) * 0.5f);
 *      yaw = float(theta_a*); angle = a*; score = score_a*.
 * Refused with CM_BAD_ARG (cm_last_error says why): everything cm_result_clusters refuses, n_angles 0 or above
 * CM_BOX_MAX_ANGLES, an unknown criterion, with CM_BOX_CLOSENESS a d_min that is not finite and > 0. Zero clusters: CM_OK
 * with zero boxes. The table is owned by the context and valid until the next merge or the next cluster or box call. No
 * later frame depends on whether it was asked for; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists the stages of
 * the cluster call followed by this call's own (k_box_*). */
#define CM_BOX_MAX_ANGLES 180
#define CM_BOX_CHUNK      256          /* members per partial sum, part of the semantics */
#define CM_BOX_MAX_EXTENT 1.0e6f       /* metres; a cluster wider than this in x or y gets no box */
#define CM_BOX_AREA       0u
#define CM_BOX_CLOSENESS  1u
#define CM_BOX_VALID      1u
typedef struct cm_box_params {         /* 32 bytes */
    cm_cluster_params cluster;         /* the clusters the boxes are fitted to (cm_result_clusters) */
    uint32_t n_angles;                 /* 1..CM_BOX_MAX_ANGLES headings in [0, pi/2) */
    uint32_t criterion;                /* CM_BOX_AREA | CM_BOX_CLOSENESS */
    float d_min;                       /* closeness: distances below it count as it; finite, > 0 (ignored for AREA) */
    uint32_t _pad;
} cm_box_params;
typedef struct cm_cluster_box {        /* 48 bytes, entry k belongs to cm_cluster k */
    float center[3];
    float size[3];                     /* along the heading, across it, height */
    float yaw;
    uint32_t angle;                    /* index of the chosen heading */
    double score;                      /* of the chosen heading */
    uint32_t flags;                    /* CM_BOX_VALID */
    uint32_t _pad;
} cm_cluster_box;
/* The direction table of n_angles headings: 2 floats (cos, sin) per heading into cos_sin. Host only, no context. CM_BAD_ARG:
 * NULL, n_angles 0 or above CM_BOX_MAX_ANGLES; CM_CAPACITY: capacity_pairs < n_angles (nothing is written). */
CM_API int cm_box_directions(uint32_t n_angles, float* cos_sin, uint64_t capacity_pairs);
/* Host copy; capacity in entries. *n_boxes is always written (0 when the call is refused); a destination that is too small:
 * CM_CAPACITY (nothing is copied; the table stays in the context, *n_boxes says how many entries it has). */
CM_API int cm_result_cluster_boxes(cm_ctx* ctx, const cm_box_params* p, cm_cluster_box* host_dst, uint64_t capacity,
                                   uint64_t* n_boxes);
/* The same table left in device memory owned by the context (*n_boxes entries of 48 bytes; NULL where there is none). */
CM_API int cm_result_cluster_boxes_device(cm_ctx* ctx, const cm_box_params* p, const void** dev_ptr, uint64_t* n_boxes);

/* ---- 2-D grid map of the frame: per-cell counts, heights, occupancy (an extension) -------------------------------------
 * What a planner takes instead of a cloud: a grid in the common frame that says per cell "nothing seen", "seen and
 * drivable" or "obstacle", with the cell's lowest and highest return beside it (a costmap / elevation-map layer; the image
 * of step 5 is nav_msgs/OccupancyGrid::data). Computed on request after a frame. Every quantity is
 * order-free — integer counts, minima, maxima — so the table is a function of the frame and the parameters alone, bit for
 * bit. All fp32 operations are rounded one at a time, round-to-nearest, no contraction.
 * Inputs, of the last frame: A, the cloud cm_merged_copy returns (the points that entered the voxel grid: after transform,
 * crop, non-finite drop, deskew, the outlier stages' masks, and ground removal where it is on), and G, the cloud
 * cm_ground_copy returns when the frame ran with ground removal (otherwise G is empty). A point is in at most one of the
 * two. A record is (x, y, z, intensity). The call reads the frame's clouds in place: they stay valid until the next frame is
 * enqueued, as for cm_result_voxel_cov.
 *   1. Cell of a point. inv = 1.0f / cell (an fp32 division). Per axis a in {x, y}: t = (p_a - origin_a) * inv (the
 *      subtraction rounded, then the product), c = floorf(t). The point is in the grid iff c >= 0.0f && c < float(n_a) on
 *      both axes, tested in float: a t of +-inf or NaN fails, -0.0f passes as cell 0. Then i_a = (int)c and the cell's index
 *      is ix + iy * nx: x is fastest, the row-major order of nav_msgs/OccupancyGrid.
 *   2. Band. A point in the grid is counted iff z_min <= z && z <= z_max (fp32 compares; infinite limits are allowed). The
 *      band applies to A and G alike.
 *   3. Per cell the record cm_grid_cell: n / n_ground count the counted points of A / G; z_lo, z_hi are the minimum and
 *      maximum z of A's counted points, g_lo, g_hi of G's; i_max is the largest intensity among the counted points of both
 *      clouds whose intensity is not NaN. Minima and maxima are taken in the order-preserving integer image of the float
 *      (bits b: b ^ 0xFFFFFFFF when the sign is set, else b ^ 0x80000000; the image of the cluster table's bounds): of two
 *      zeros of either sign the minimum is -0 and the maximum +0. A field with nothing to take an extreme of is the canonical
 *      quiet NaN 0x7FC00000.
 *   4. State. m = n + n_ground. m < min_points: CM_GRID_UNKNOWN. Otherwise n == 0: CM_GRID_FREE. Otherwise lo = z_lo when
 *      n_ground == 0, else the smaller of z_lo and g_lo in the same integer order; the cell is CM_GRID_OCCUPIED iff
 *      (z_hi - lo) >= obstacle_height, the subtraction in fp32, else CM_GRID_FREE. So with ground removal on and
 *      obstacle_height 0 any non-ground return occupies its cell; without ground removal the rule is the classic
 *      height-difference map.
 *   5. Occupancy image. One int8_t per cell in the same order: -1 UNKNOWN, 0 FREE, 100 OCCUPIED.
 * Refused with CM_BAD_ARG (cm_last_error says why): everything cm_result_clusters refuses about the result (a frame in
 * flight, no result, a result of cm_merge_partial / cm_merge_tables, a last status other than CM_OK); NULL parameters; an
 * origin that is not finite; a cell that is not finite and > 0, or whose inv is not finite and > 0; nx or ny 0, or
 * nx * ny > CM_GRID_MAX_CELLS; a NaN band limit or z_min > z_max; an obstacle_height that is not finite and >= 0; min_points
 * 0. The table and the image are owned by the context and valid until the next merge or the next grid call. No later frame
 * depends on whether they were asked for; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists this call's stages
 * (k_grid_bin, k_grid_finish). */
#define CM_GRID_MAX_CELLS (1u << 22)
#define CM_GRID_UNKNOWN   0u
#define CM_GRID_FREE      1u
#define CM_GRID_OCCUPIED  2u
typedef struct cm_grid_params {        /* 36 bytes, no padding */
    float origin[2];                   /* the corner of cell (0, 0), common frame; finite */
    float cell;                        /* edge of a cell (m); finite, > 0 */
    uint32_t nx, ny;                   /* cells along x and y; nx * ny <= CM_GRID_MAX_CELLS */
    float z_min, z_max;                /* closed height band; infinities allowed */
    float obstacle_height;             /* finite, >= 0 */
    uint32_t min_points;               /* >= 1 */
} cm_grid_params;
typedef struct cm_grid_cell {          /* 32 bytes, cell (ix, iy) is entry ix + iy * nx */
    uint32_t n;                        /* counted points of A */
    uint32_t n_ground;                 /* counted points of G */
    float z_lo, z_hi;                  /* of A's counted points; NaN when n == 0 */
    float g_lo, g_hi;                  /* of G's counted points; NaN when n_ground == 0 */
    float i_max;                       /* NaN when no counted point has an intensity that is not NaN */
    uint32_t state;                    /* CM_GRID_* */
} cm_grid_cell;
/* Host copy; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied; the table stays in the context). */
CM_API int cm_result_grid_map(cm_ctx* ctx, const cm_grid_params* p, cm_grid_cell* host_dst, uint64_t capacity_cells);
/* The same table left in device memory owned by the context (*n_cells entries of 32 bytes). */
CM_API int cm_result_grid_map_device(cm_ctx* ctx, const cm_grid_params* p, const void** dev_ptr, uint64_t* n_cells);
/* The occupancy image of the last grid call since the last merge; capacity in cells. *n_cells is always written (0 when
 * there is no such call: CM_BAD_ARG); a destination that is too small: CM_CAPACITY (nothing is copied). */
CM_API int cm_grid_occupancy_copy(cm_ctx* ctx, int8_t* host_dst, uint64_t capacity_cells, uint64_t* n_cells);

/* ---- free-space ray casting over the grid map: per-cell pass counts, the cleared image (an extension) -------------------
 * The grid map calls a cell FREE only where returns landed; every cell a beam flew through on its way to a return stays
 * UNKNOWN. This call clears them, as costmap_2d's obstacle layer and octomap's insertPointCloud do: per sensor it walks an
 * integer line from the sensor's cell to every distinct cell that holds one of that sensor's counted points, counts per cell
 * the rays that crossed it and the rays that ended in it, and emits a second occupancy image in which an UNKNOWN cell crossed
 * by enough rays is FREE. Computed on request after a frame; it never changes a frame. Every quantity is an
 * integer count over a set of distinct rays, so the tables are a function of the frame and the parameters alone, bit for bit.
 *   1. Base map. The call first computes the grid map of p exactly as cm_result_grid_map(ctx, p, ...) does: afterwards the
 *      context's grid table and image are those of p, and cm_grid_occupancy_copy returns them.
 *   2. Counted points: exactly the points the grid map counts — in A or G, inside the grid on both axes (step 1 of the
 *      grid), inside the band (its step 2). The cell of such a point of sensor s is an end cell of s. A sensor is an entry
 *      of the frame's descriptor: the sensors that have a cloud, in ascending order of their number.
 *   3. Origin cell. For sensor s, (x, y) is the fp32 translation of the matrix the frame transformed that sensor's cloud with
 *      (cm_set_sensor_transform's t, rounded per component), as it stood when the frame was assembled. Its cell is the grid's
 *      step 1 applied to that (x, y): the same fp32 subtraction, product and floorf, membership tested in float (-0.0f
 *      passes as cell 0). A sensor whose origin is outside the grid or not finite casts no rays. Under ego-motion
 *      compensation the origin is still that translation: the sensor's position at the cloud's own instant, not moved to
 *      t_ref — an approximation (at 20 m/s and 50 ms, 1 m).
 *   4. Ray set: the set of distinct pairs (s, end cell e of s) over the sensors that have an origin cell. Two points of one
 *      sensor in one cell are one ray; one cell reached by two sensors is two rays.
 *   5. Walk. For origin cell o and end cell e: dx = ex - ox, dy = ey - oy, L = max(|dx|, |dy|), K = L when max_range_cells
 *      is 0, else min(L, max_range_cells). For k = 0 .. K - 1 the ray crosses the cell
 *      (ox + rdiv(k * dx, L), oy + rdiv(k * dy, L)), where rdiv(a, L) = sign(a) * ((2 |a| + L) div 2 L) is the integer
 *      quotient rounded to nearest, a half away from zero. The origin cell is crossed (k = 0), the end cell is not, L = 0
 *      crosses nothing. Every crossed cell lies inside the grid and no ray crosses a cell twice (DESIGN.md §21 proves both).
 *      The rule is symmetric under mirroring either axis and under swapping them.
 *   6. Per cell the record cm_grid_ray_cell: n_pass, the rays of the set that cross the cell; n_end, the rays of the set
 *      whose end cell it is (whatever max_range_cells).
 *   7. Cleared image. One int8_t per cell, laid out like the grid's: base OCCUPIED gives 100 (a hit wins over any number of
 *      passes), base FREE gives 0, base UNKNOWN gives 0 iff n_pass >= min_pass, else -1.
 * NULL ray parameters mean {1, 0}. Refused with CM_BAD_ARG: everything cm_result_grid_map refuses, and min_pass 0. The
 * bitmaps of end cells (the frame's sensors x nx * ny bits, at most 8 MiB), the table and the cleared image are owned by the
 * context and valid until the next merge, the next grid call or the next ray call. No later frame depends on whether they
 * were asked for; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists this call's stages (the grid's, then ray_clear,
 * k_ray_mark, k_ray_cast, k_ray_finish). Not modelled: the height of a beam over a cell (2-D casting clears under an
 * overhang), rays of points outside the grid or the band. Accumulation over frames is the occupancy map's (cm_map_integrate
 * below), which casts the same rays. */
typedef struct cm_ray_params {         /* 8 bytes */
    uint32_t min_pass;                 /* rays that must cross an UNKNOWN cell to clear it; >= 1 */
    uint32_t max_range_cells;          /* steps of a ray from its origin that count; 0 = to the end cell */
} cm_ray_params;
typedef struct cm_grid_ray_cell {      /* 8 bytes, cell (ix, iy) is entry ix + iy * nx */
    uint32_t n_pass;                   /* rays that cross the cell */
    uint32_t n_end;                    /* rays that end in it */
} cm_grid_ray_cell;
/* Host copy; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied; the tables stay in the context). */
CM_API int cm_result_grid_rays(cm_ctx* ctx, const cm_grid_params* p, const cm_ray_params* r, cm_grid_ray_cell* host_dst,
                               uint64_t capacity_cells);
/* The same table left in device memory owned by the context (*n_cells entries of 8 bytes). */
CM_API int cm_result_grid_rays_device(cm_ctx* ctx, const cm_grid_params* p, const cm_ray_params* r, const void** dev_ptr,
                                      uint64_t* n_cells);
/* The cleared image of the last ray call since the last merge or grid call; capacity in cells. *n_cells is always written (0
 * when there is no such call: CM_BAD_ARG); a destination that is too small: CM_CAPACITY (nothing is copied). */
CM_API int cm_grid_ray_occupancy_copy(cm_ctx* ctx, int8_t* host_dst, uint64_t capacity_cells, uint64_t* n_cells);

/* ---- rolling log-odds occupancy map accumulated over frames (an extension) ---------------------------------------------
 * A single frame's clearing is noise to a planner. This is the persistent map of costmap_2d and octomap: every beam adds
 * evidence for "free" along its path and for "occupied" at its end, per cell an integer log-odds that is clamped, and the
 * map's window scrolls with the vehicle over a lattice fixed in a world frame. The caller passes the pose of every frame it
 * integrates, for example the one cm_result_align or cm_result_ndt_align returned, chained. Everything is
 * integer arithmetic over sets of distinct rays apart from the fp32 cell computation of step 1, every operation of which is
 * rounded on its own: the map is a function of the frames, the poses and the parameters alone, bit for bit.
 * Pose: a row-major 3 x 4 fp32 matrix P that takes the common (vehicle) frame at the frame's reference instant into a fixed
 * world frame; all twelve entries finite.
 *   1. World cell of a point. q = (x, y, z) is a point of the frame in the common frame, as the grid map sees it (after the
 *      sensor transform, deskew and validity). wx = ((P0*x + P1*y) + P2*z) + P3, wy = ((P4*x + P5*y) + P6*z) + P7. With
 *      inv = 1.0f / cell (an fp32 division), per axis c = floorf(w * inv), the product in fp32. The cell exists iff
 *      c > -1073741824.0f && c < 1073741824.0f, tested in float (NaN and +-inf fail); then g = (int)c, an absolute cell. No
 *      origin is subtracted: the lattice never moves.
 *   2. Window. The vehicle cell (vx, vy) is step 1 applied to (P3, P7). The anchor is a = (vx - (int)(nx / 2),
 *      vy - (int)(ny / 2)), the window ax <= gx < ax + nx and likewise in y; window cell (gx - ax, gy - ay) is entry
 *      ix + iy * nx.
 *   3. Counted points. A counted point lies in A (what cm_merged_copy returns) or G (what cm_ground_copy returns), has
 *      z_min <= q.z && q.z <= z_max (the band is in the vehicle frame) and a world cell inside the window. E_s is the set of
 *      distinct window cells of sensor s's counted points of A and G, H_s the same over A alone. A sensor is an entry of the
 *      frame's descriptor, as for cm_result_grid_rays.
 *   4. Origins. Sensor s's origin cell is step 1 applied to P times the full (x, y, z) translation of the matrix the frame
 *      transformed that sensor's cloud with. A sensor whose origin cell does not exist or lies outside the window casts no
 *      rays; its hits still count. Under ego-motion compensation the origin is still that translation, not moved to t_ref
 *      (the approximation of cm_result_grid_rays' step 3), and P is the pose at t_ref.
 *   5. Rays: those of cm_result_grid_rays' step 5, unchanged, over the window: from each origin cell to every cell of E_s,
 *      with max_range_cells. n_pass(c) is the number of rays that cross c.
 *   6. Evidence per window cell. n_hit = |{s : c in H_s}|, n_ground = |{s : c in E_s \ H_s}|, over all sensors of the frame.
 *      n_hit > 0: d = l_hit * n_hit (a hit wins over any number of passes). Otherwise d = -l_miss * (n_pass + n_ground), in
 *      int64.
 *   7. State, cm_map_cell. A cell of the new window that was not in the previous window starts {0, 0}: every cell on the
 *      first integration after cm_map_configure. A cell in both windows carries its state over. If d != 0,
 *      logodds = clamp(logodds + d, l_min, l_max) in int64 and n_obs is incremented, saturating.
 *   8. Image. One int8_t per window cell: n_obs == 0 gives -1, logodds >= l_occ gives 100, logodds <= l_free gives 0, anything
 *      else -1.
 * cm_map_configure refuses with CM_BAD_ARG (cm_last_error says why): a cell that is not finite and > 0, or whose inv is not
 * finite and > 0; nx or ny 0, or nx * ny > CM_GRID_MAX_CELLS; a NaN band limit or z_min > z_max; l_hit < 1 or l_miss < 1;
 * any of the six l_* above 2^20 in magnitude; anything that breaks l_min <= l_free < l_occ <= l_max and l_min <= 0 <= l_max;
 * a frame in flight. cm_map_integrate refuses everything cm_result_grid_map refuses about the result, and: no configured
 * map, a pose that is not finite, a vehicle cell that does not exist, and a frame that was already integrated into this map
 * (each frame is integrated at most once). Unlike every other by-product the map survives merges: it lives until the next
 * cm_map_configure or cm_destroy, uses buffers of its own (the grid map's and the rays' tables stay what they were), and no
 * later frame depends on whether it exists. All of its memory is taken by cm_map_configure. With CM_FLAG_PROFILE,
 * cm_get_stage_times after an integrate call lists map_clear, k_map_mark, k_ray_cast, k_map_update. Not modelled: 3-D
 * occupancy and the height of a beam over a cell, probabilities beyond the three-valued image, origins moved under deskew. */
#define CM_MAP_MAX_LOGODDS (1 << 20)
typedef struct cm_map_params {         /* 48 bytes, no padding */
    float cell;                        /* edge of a cell (m); finite, > 0 */
    uint32_t nx, ny;                   /* the window in cells; nx * ny <= CM_GRID_MAX_CELLS */
    float z_min, z_max;                /* closed height band in the vehicle frame; infinities allowed */
    int32_t l_hit, l_miss;             /* log-odds added per sensor that hits, subtracted per pass; >= 1 */
    int32_t l_min, l_max;              /* clamp limits; l_min <= 0 <= l_max */
    int32_t l_free, l_occ;             /* image thresholds; l_min <= l_free < l_occ <= l_max */
    uint32_t max_range_cells;          /* steps of a ray from its origin that count; 0 = to the end cell */
} cm_map_params;
typedef struct cm_map_cell {           /* 8 bytes, window cell (ix, iy) is entry ix + iy * nx */
    int32_t logodds;
    uint32_t n_obs;                    /* integrations that changed the cell's evidence (d != 0), saturating */
} cm_map_cell;
typedef struct cm_map_info {           /* 32 bytes */
    int32_t anchor[2];                 /* the absolute cell of window cell (0, 0) at the last integration */
    uint32_t nx, ny;
    uint64_t n_frames;                 /* integrations since cm_map_configure */
    uint32_t sensors_cast;             /* bit s: descriptor sensor s cast rays in the last integration */
    uint32_t _pad;
} cm_map_info;
/* Non-NULL parameters allocate the map and clear it (every cell {0, 0}, the image -1, no frame integrated); NULL frees it. */
CM_API int cm_map_configure(cm_ctx* ctx, const cm_map_params* p);
/* Integrates the last frame under the pose; *out (may be NULL) is the map's info afterwards. */
CM_API int cm_map_integrate(cm_ctx* ctx, const float pose[12], cm_map_info* out);
/* Host copy of the state table; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied). *info may be NULL. */
CM_API int cm_map_copy(cm_ctx* ctx, cm_map_cell* host_dst, uint64_t capacity_cells, cm_map_info* info);
/* The same table in device memory owned by the context, valid until the next cm_map_integrate or cm_map_configure. */
CM_API int cm_map_device(cm_ctx* ctx, const void** dev_ptr, cm_map_info* info);
/* Host copy of the image; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied). *info may be NULL. */
CM_API int cm_map_occupancy_copy(cm_ctx* ctx, int8_t* host_dst, uint64_t capacity_cells, cm_map_info* info);
/* Puts a recorded map back (localisation in a map that was built earlier): host_src is a state table as cm_map_copy returned it,
 * anchor the anchor it was recorded with. It replaces the state, recomputes the image by step 8, sets the anchor,
 * n_frames = 1 and sensors_cast = 0, and makes the layers behind stale exactly as an integration does. A frame held at the time
 * counts as not yet integrated. CM_BAD_ARG: no configured map, n_cells != nx * ny, a NULL table or anchor, a logodds outside
 * [l_min, l_max], |anchor| >= 2^30 on an axis, a frame in flight (nothing changes). *out (may be NULL) is the info afterwards.
 * No other function of the map changes. */
CM_API int cm_map_load(cm_ctx* ctx, const cm_map_cell* host_src, uint64_t n_cells, const int32_t anchor[2], cm_map_info* out);

/* ---- cost layer over the occupancy map: exact distance field and inflated costmap (an extension) -------------------------
 * The map's image is costmap_2d's obstacle layer. A planner plans on the layer above it, the inflation layer, and clearance
 * checks want the distance field under that. The cost layer is configured once behind the map and recomputed on request from
 * the map's current image; it yields two tables per window cell, dist2 (uint32_t) and cost (uint8_t), entry ix + iy * nx
 * (DESIGN.md §23). A squared distance in cells is an integer and the table of step 3 is built on the host from an exponential
 * that is spelled out (cm_ndt_math.hpp), so both tables are bit for bit a function of the image and the parameters.
 * Input: the map's image I as cm_map_occupancy_copy returns it (ny x nx, entry ix + iy * nx) and the map's `cell`.
 *   1. Obstacles. O = { c : I(c) == 100 }. Only cells of the window count: what scrolled out is forgotten, as the map
 *      forgets it.
 *   2. Distance field. dist2(c) = min over o in O of (cx - ox)^2 + (cy - oy)^2, in integer arithmetic; O empty gives
 *      CM_MAP_DIST_NONE in every cell. With nx, ny <= CM_COST_MAX_AXIS the largest value is 2 * 2047^2, so uint32_t holds it.
 *      The field is not truncated at the inflation radius: it is the whole window's exact transform.
 *   3. Cost table, built on the host in double from four fp32 values widened to double, the map's cell, inscribed_radius,
 *      inflation_radius and cost_scaling. R = (uint32_t)ceil(inflation_radius / cell); the table has R * R + 1 entries.
 *      lut[0] = 254. For d2 >= 1, m = sqrt((double)d2) * cell (each operation rounded once): m <= inscribed_radius gives 253,
 *      m > inflation_radius gives 0, anything else (uint8_t)floor(252.0 * cm_exp_neg(cost_scaling * (m - inscribed_radius))).
 *      A d2 beyond the table has cost 0 (sqrt(R * R + 1) lies far more than a rounding above R for R <= 256, so this agrees
 *      with the formula). This is costmap_2d::InflationLayer::computeCost with the exponential replaced by cm_exp_neg.
 *   4. Cost. infl = dist2 <= R * R ? lut[dist2] : 0. I == 100: 254. I == 0: infl. I == -1: infl if infl >= 253, else 255
 *      (NO_INFORMATION); with CM_COST_INFLATE_UNKNOWN the condition is infl > 0 (costmap_2d's inflate_unknown).
 * cm_map_cost_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured map; a radius or the scaling that is
 * not finite or is negative; inflation_radius < inscribed_radius; R > CM_COST_MAX_RADIUS_CELLS; unknown flag bits; a map
 * wider or taller than CM_COST_MAX_AXIS cells (step 2's bound; nx * ny alone admits a window of 1 x 2^22); a frame in flight.
 * R = 0 (a table of one entry) is legal. All memory of the layer is taken by cm_map_cost_configure (cost, dist2, the column
 * pass's two tables, the cost table): no update call allocates. cm_map_cost_update is allowed before any integration (the
 * image is all -1: dist2 all CM_MAP_DIST_NONE, cost all 255). The tables are stale from cm_map_cost_configure and from every
 * cm_map_integrate until the next cm_map_cost_update: the copies and cm_map_cost_device then refuse with CM_BAD_ARG.
 * cm_map_configure, in either form, frees the layer; like the map it survives merges, and neither the map's state, image and
 * info nor any frame depends on whether it exists. With CM_FLAG_PROFILE, cm_get_stage_times after an update lists
 * k_cost_colmask, k_cost_colcarry, k_cost_rows. Not modelled: a signed distance (inside obstacles dist2 is 0), the index of
 * the nearest obstacle, obstacles outside the window, a footprint other than the inscribed radius, unknown cells as
 * obstacles. */
#define CM_MAP_DIST_NONE 0xFFFFFFFFu
#define CM_COST_LETHAL 254
#define CM_COST_INSCRIBED 253
#define CM_COST_NO_INFORMATION 255
#define CM_COST_INFLATE_UNKNOWN 1u
#define CM_COST_MAX_RADIUS_CELLS 256
#define CM_COST_MAX_AXIS 2048
typedef struct cm_cost_params {        /* 16 bytes, no padding */
    float inscribed_radius;            /* metres; finite, >= 0 */
    float inflation_radius;            /* metres; finite, >= inscribed_radius; at most CM_COST_MAX_RADIUS_CELLS cells */
    float cost_scaling;                /* 1 / metres; finite, >= 0 */
    uint32_t flags;                    /* CM_COST_INFLATE_UNKNOWN or 0 */
} cm_cost_params;
/* Non-NULL parameters allocate the layer and build the table (the tables are stale until the first update); NULL frees it. */
CM_API int cm_map_cost_configure(cm_ctx* ctx, const cm_cost_params* p);
/* Computes dist2 and cost from the map's current image; *out (may be NULL) is the map's info. */
CM_API int cm_map_cost_update(cm_ctx* ctx, cm_map_info* out);
/* Host copies of the two tables; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied; *info, which may be
 * NULL, is still written). */
CM_API int cm_map_cost_copy(cm_ctx* ctx, uint8_t* host_dst, uint64_t capacity_cells, cm_map_info* info);
CM_API int cm_map_dist_copy(cm_ctx* ctx, uint32_t* host_dst, uint64_t capacity_cells, cm_map_info* info);
/* The same tables in device memory owned by the context, valid until the next cm_map_cost_update, cm_map_integrate,
 * cm_map_cost_configure or cm_map_configure. Either pointer argument may be NULL. */
CM_API int cm_map_cost_device(cm_ctx* ctx, const void** cost, const void** dist2, cm_map_info* info);
/* Host copy of the R * R + 1 bytes of step 3; *n (may be NULL) is that count. Fewer than that: CM_CAPACITY (nothing is
 * copied, *n is still written). The table exists from cm_map_cost_configure on: staleness does not concern it. */
CM_API int cm_map_cost_table_copy(cm_ctx* ctx, uint8_t* host_dst, uint64_t capacity, uint64_t* n);

/* ---- plan layer behind the cost layer: navigation function and path extraction (an extension) ---------------------------
 * In a costmap_2d stack the step behind the inflation layer is navfn / global_planner: a potential over the costmap from a
 * goal, then a path from any start by descent. The plan layer is configured once behind the cost layer and recomputed on
 * request; it yields one table per window cell, pot (uint32_t, entry ix + iy * nx), and paths over it. Every
 * step cost is a positive integer, so the Bellman equations of step 4 have exactly one solution: pot is bit for bit a
 * function of the cost table, the parameters and the goal, whatever the order in which the device relaxes cells.
 * Input: the cost layer's fresh cost table (ny x nx bytes, entry ix + iy * nx) and the map's info.
 *   1. Traversal weight w(c). v is the cost byte of c. v == 255 (unknown): impassable; with CM_PLAN_ALLOW_UNKNOWN, v := 252
 *      instead. v >= 253 (inscribed or lethal): impassable. Otherwise w = neutral + ((v * cost_factor_q8) >> 8) in integer
 *      arithmetic, so w >= 1 for every passable cell. navfn's 50 and 0.8 are neutral 50 and cost_factor_q8 205.
 *   2. Goal. (x, y) are fp32 world coordinates in the map's world frame. The absolute cell is step 1 of the map's semantics
 *      per axis, floorf(x * inv) with the same existence test; the window cell is that cell minus the map's anchor. A goal
 *      that is not finite, whose cell does not exist or that lies outside the window: CM_BAD_ARG. The goal cell has potential
 *      0 whatever its cost byte, and counts as passable in step 3's corner rule.
 *   3. Steps. Cells are 8-connected; direction d = 0..7 is (dx, dy) = (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1),
 *      (1,-1). A step costs k * w(the cell left behind when walking towards the goal), k = 5 for a straight step and 7 for a
 *      diagonal one. No corner cutting: a diagonal step between c and n exists only if both cells that share an edge with
 *      both of them are passable.
 *   4. Potential. pot(goal) = 0. For every other passable c, pot(c) is the minimum over the existing steps to a neighbour n
 *      with pot(n) defined of pot(n) + k * w(c). Impassable and unreachable cells hold CM_PLAN_UNREACHABLE. This is the exact
 *      shortest-path cost, and it is unique.
 *   5. Range. A simple path has at most nx * ny - 1 steps. With w_max = neutral + ((252 * cost_factor_q8) >> 8),
 *      cm_map_plan_configure refuses with CM_BAD_ARG if 7 * w_max * (nx * ny - 1) > 0xFFFFFFFE, evaluated in 64 bits: a
 *      potential could then not be told from CM_PLAN_UNREACHABLE. With 50 / 205 this admits about 2.4 M cells: 1000 x 1000
 *      passes, 2048 x 2048 needs a smaller neutral or factor.
 *   6. Path. The start is given like the goal; outside the window or not finite: CM_BAD_ARG. pot(start) ==
 *      CM_PLAN_UNREACHABLE: status CM_PATH_UNREACHABLE, zero cells. Otherwise c = start, and while c is not the goal the next
 *      cell is the neighbour n over the existing steps with pot(n) defined that minimises pot(n) + k * w(c); ties go to the
 *      lowest direction number. The output is the window cell indices ix + iy * nx, start first and goal last. By step 4 that
 *      minimum equals pot(c): the path's step costs sum to pot(start), pot strictly decreases along it, and it ends. A path
 *      longer than max_path_cells (1..nx * ny, given at configure time) writes its first max_path_cells cells with status
 *      CM_PATH_TRUNCATED.
 * cm_map_plan_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured cost layer; neutral outside 1..255;
 * cost_factor_q8 above 256; unknown flag bits; max_path_cells 0 or above nx * ny; step 5's range rule; a frame in flight.
 * All memory of the layer is taken by cm_map_plan_configure (pot, the tile flags and sweep counters, the path buffer and its
 * page-locked host words): no update or path call allocates. pot is stale from cm_map_plan_configure and from every
 * cm_map_integrate and cm_map_cost_update until the next cm_map_plan_update, which itself refuses a stale cost layer: the
 * copies, cm_map_plan_device and cm_map_plan_path then refuse with CM_BAD_ARG. cm_map_cost_configure and cm_map_configure,
 * in either form, free the layer; like the map it survives merges, and nothing else depends on whether it exists. With
 * CM_FLAG_PROFILE, cm_get_stage_times after an update lists k_plan_init and k_plan_sweep (all sweeps and the reads of their
 * counters as one stage), after a path call k_plan_path. Not modelled: navfn's quadratic interpolation and sub-cell gradient
 * paths, A*, path smoothing, several goals per update, goals or paths outside the window. */
#define CM_PLAN_UNREACHABLE 0xFFFFFFFFu
#define CM_PLAN_ALLOW_UNKNOWN 1u
/* cm_path_info.status (values, not bits; unrelated to cm_result.path_flags) */
#define CM_PATH_FOUND 0u
#define CM_PATH_UNREACHABLE 1u
#define CM_PATH_TRUNCATED 2u
typedef struct cm_plan_params {        /* 16 bytes, no padding */
    uint32_t neutral;                  /* 1..255 */
    uint32_t cost_factor_q8;           /* 0..256: the cost byte's factor in 1/256 */
    uint32_t flags;                    /* CM_PLAN_ALLOW_UNKNOWN or 0 */
    uint32_t max_path_cells;           /* 1..nx * ny: the longest path cm_map_plan_path writes */
} cm_plan_params;
typedef struct cm_plan_info {          /* 16 bytes */
    uint32_t goal[2];                  /* the goal's window cell (ix, iy) */
    uint32_t n_sweeps;                 /* launches of the sweep up to the first that changed nothing (not a function of the
                                          input alone: tiles of one sweep may or may not see one another's words) */
    uint32_t _pad;
} cm_plan_info;
typedef struct cm_path_info {          /* 32 bytes */
    uint32_t start[2], goal[2];        /* window cells (ix, iy) */
    uint32_t n_cells;                  /* cells of the path that were written (0: unreachable) */
    uint32_t status;                   /* CM_PATH_FOUND, CM_PATH_UNREACHABLE or CM_PATH_TRUNCATED */
    uint32_t pot_start;                /* pot(start) */
    uint32_t _pad;
} cm_path_info;
/* Non-NULL parameters allocate the layer (pot is stale until the first update); NULL frees it. */
CM_API int cm_map_plan_configure(cm_ctx* ctx, const cm_plan_params* p);
/* Computes pot for the goal at world (gx, gy) from the cost layer's fresh table. *out and *map (either may be NULL) are the
 * plan's and the map's info. CM_INTERNAL: nx * ny sweeps did not reach the fixed point (they provably do). */
CM_API int cm_map_plan_update(cm_ctx* ctx, float gx, float gy, cm_plan_info* out, cm_map_info* map);
/* Host copy of pot; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied; *info and *map, which may be
 * NULL, are still written). */
CM_API int cm_map_plan_copy(cm_ctx* ctx, uint32_t* host_dst, uint64_t capacity_cells, cm_plan_info* info, cm_map_info* map);
/* The same table in device memory owned by the context, valid until the next cm_map_plan_update, cm_map_cost_update,
 * cm_map_integrate or configure call of the three layers. */
CM_API int cm_map_plan_device(cm_ctx* ctx, const void** pot, cm_plan_info* info, cm_map_info* map);
/* The path of step 6 from world (sx, sy) to the goal of the last update; capacity in cells. A capacity below n_cells:
 * CM_CAPACITY (nothing is copied, *info is still written). *info may be NULL. */
CM_API int cm_map_plan_path(cm_ctx* ctx, float sx, float sy, uint32_t* host_dst, uint64_t capacity, cm_path_info* info);

/* ---- rollout layer behind the plan layer: sampled velocity commands scored over cost and pot (an extension) ----------------
 * In a costmap_2d stack the consumer behind the global planner is the local planner (base_local_planner, dwa_local_planner):
 * it samples velocity commands, rolls each forward, checks the robot's footprint against the costmap pose by pose, scores the
 * survivors by cost and by distance to the goal and picks one. The rollout layer is configured once behind the plan layer and
 * evaluated on request; it yields one cm_traj_score per sample and the best of them. The goal-distance grid
 * base_local_planner builds with a wavefront of its own is the plan layer's pot. Positions are fp32 with every operation
 * rounded on its own, headings are integers, scores are integers: the table is bit for bit a function of the cost table, pot,
 * the map's info and cell, the parameters, the footprint and the window.
 * Input: the cost layer's fresh cost table, the plan layer's fresh pot, the map's info; cm_traj_params and the footprint
 * (n_foot body-frame points (bx, by), x forward, y left, metres) given at configure time; per evaluate a cm_traj_window
 * (x, y, yaw, v_lo, v_hi, w_lo, w_hi, dt). Sample (i, j), 0 <= i < nv, 0 <= j < nw, is entry i * nw + j.
 *   1. Samples. In fp32, every operation rounded on its own: nv == 1 gives v_0 = v_lo, otherwise
 *      v_i = v_lo + (float)i * ((v_hi - v_lo) / (float)(nv - 1)); w_j likewise from w_lo, w_hi and nw. Step length
 *      s_i = v_i * dt in fp32. Headings are binary angles, a uint32_t in which a full turn is 2^32. With
 *      K = 4294967296.0 / 6.283185307179586, in double: dh_j = rint(((double)w_j * (double)dt) * K), an integer of magnitude
 *      at most 2^31 by the refusal below, reduced mod 2^32 (so +2^31 and -2^31 are the same increment; this is the one place
 *      that differs from a plain (int32_t) cast, which is undefined at +2^31). h0 = rint((double)yaw * K), reduced mod 2^32.
 *   2. Heading table. CM_TRAJ_HEADINGS pairs (cos, sin) in fp32, built once on the host: th = (double)a *
 *      (6.283185307179586 / 4096.0), cos and sin from libm, rounded to float; entries 0, 1024, 2048 and 3072 are set to the
 *      exact axes (1, 0), (0, 1), (-1, 0), (0, -1), so that driving along an axis stays in its row or column.
 *      cm_traj_directions returns the table. A heading H uses entry ((H + 0x80000) >> 20) & 4095, the sum wrapping.
 *   3. Rollout, forward Euler as in base_local_planner. p_0 = (x, y), H_0 = h0. For k = 0 .. n_steps - 1, with (c, s) the
 *      entry of H_k: x_{k+1} = x_k + s_i * c, y_{k+1} = y_k + s_i * s, H_{k+1} = H_k + dh_j (wrapping). One multiplication and
 *      one addition, each rounded; nothing is fused. Poses k = 1 .. n_steps are checked; pose 0 is not.
 *   4. Looked-up points of pose k. The centre (x_k, y_k), and per footprint point, with (c, s) the entry of H_k and every
 *      operation rounded: wx = (x_k + c * bx) - s * by, wy = (y_k + s * bx) + c * by. A point's cell is step 1 of the map's
 *      semantics per axis (floorf(w * inv), the same existence test) minus the map's anchor.
 *   5. Classes. A point whose cell does not exist or lies outside the window is off map. Otherwise v is the cost byte of its
 *      cell: v == 254 is a collision; v == 255 is a collision unless CM_TRAJ_ALLOW_UNKNOWN, and then contributes 0; at the
 *      centre only, v == 253 is a collision too; anything else contributes v. The first pose with an off-map or collision
 *      point ends the trajectory, bad_step = k; status is CM_TRAJ_OFF_MAP if any point of that pose is off map, else
 *      CM_TRAJ_COLLISION (a priority by class, not by point order).
 *   6. Score. Without a bad pose: occ = the largest contribution over all poses and points, (end_x, end_y) = p_{n_steps},
 *      pot_end = pot at the centre's cell of the last pose. pot_end == CM_PLAN_UNREACHABLE: status CM_TRAJ_NO_POTENTIAL, with
 *      bad_step = n_steps. Otherwise status CM_TRAJ_VALID, bad_step 0 and total = occ_scale * occ + goal_scale * pot_end in
 *      uint64_t. Every other entry holds occ 0, pot_end CM_PLAN_UNREACHABLE, total UINT64_MAX and the (end_x, end_y) of its
 *      bad pose.
 *   7. Best. The valid entry with the smallest total, ties to the lowest entry index; none valid: CM_TRAJ_NONE. best_v, best_w
 *      are v_i, w_j of that entry (0 when there is none), n_valid the number of valid entries.
 * cm_map_traj_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured plan layer; nv or nw 0 or nv * nw above
 * CM_TRAJ_MAX_SAMPLES; n_steps outside 1..CM_TRAJ_MAX_STEPS; unknown flag bits; n_foot outside 1..CM_TRAJ_MAX_FOOT; a NULL
 * footprint or a coordinate that is not finite; a frame in flight. cm_map_traj_evaluate refuses: no rollout layer; a stale pot
 * (or none yet); a window value that is not finite; v_hi < v_lo, w_hi < w_lo, dt <= 0; |yaw| > 1024; any
 * |(double)w_j * (double)dt| >= 3.141592653589793; a sample or a step length s_i that is not finite (they overflow fp32); a
 * start whose cell does not exist or lies outside the window; a frame in flight. All memory of the layer is taken by cm_map_traj_configure (the scores, the sample tables and info words, the heading
 * table and the footprint, the page-locked host words): no evaluate or copy allocates. The scores are stale from
 * cm_map_traj_configure and from every cm_map_integrate, cm_map_cost_update and cm_map_plan_update until the next
 * cm_map_traj_evaluate: cm_map_traj_copy and cm_map_traj_device then refuse with CM_BAD_ARG and say since which call.
 * cm_map_plan_configure, cm_map_cost_configure and cm_map_configure, in either form, free the layer; like the map it survives
 * merges, and nothing else depends on whether it exists. With CM_FLAG_PROFILE, cm_get_stage_times after an evaluate lists
 * k_traj_roll and k_traj_best. Not modelled: path-distance and heading-alignment terms, acceleration limits (the caller passes
 * the dynamic window), holonomic vy, oscillation suppression, the poses of a trajectory as an output. A stationary sample
 * (v = 0, dh = 0) is a valid trajectory like any other; a caller who does not want it sets v_lo > 0. */
#define CM_TRAJ_MAX_SAMPLES 16384
#define CM_TRAJ_MAX_STEPS 256
#define CM_TRAJ_MAX_FOOT 256
#define CM_TRAJ_HEADINGS 4096
#define CM_TRAJ_ALLOW_UNKNOWN 1u
#define CM_TRAJ_NONE 0xFFFFFFFFu
/* cm_traj_score.status (values, not bits) */
#define CM_TRAJ_VALID 0u
#define CM_TRAJ_COLLISION 1u
#define CM_TRAJ_OFF_MAP 2u
#define CM_TRAJ_NO_POTENTIAL 3u
typedef struct cm_traj_params {        /* 24 bytes, no padding */
    uint32_t nv, nw;                   /* linear and angular sample counts; each >= 1, nv * nw <= CM_TRAJ_MAX_SAMPLES */
    uint32_t n_steps;                  /* 1..CM_TRAJ_MAX_STEPS */
    uint32_t occ_scale, goal_scale;    /* the weights of step 6 */
    uint32_t flags;                    /* CM_TRAJ_ALLOW_UNKNOWN or 0 */
} cm_traj_params;
typedef struct cm_traj_window {        /* 32 bytes: 8 floats */
    float x, y, yaw;                   /* the start pose in the map's world frame; yaw in radians, |yaw| <= 1024 */
    float v_lo, v_hi;                  /* m/s; v_lo <= v_hi */
    float w_lo, w_hi;                  /* rad/s; w_lo <= w_hi */
    float dt;                          /* seconds per step; > 0 */
} cm_traj_window;
typedef struct cm_traj_score {         /* 32 bytes */
    uint32_t status;                   /* CM_TRAJ_VALID, CM_TRAJ_COLLISION, CM_TRAJ_OFF_MAP or CM_TRAJ_NO_POTENTIAL */
    uint32_t bad_step;                 /* the pose that ended the trajectory (0: valid) */
    uint32_t occ;                      /* the largest cost byte under the footprint along the way */
    uint32_t pot_end;                  /* pot at the last pose's centre */
    uint64_t total;                    /* occ_scale * occ + goal_scale * pot_end; UINT64_MAX unless valid */
    float end_x, end_y;                /* the last pose's centre, or the bad pose's */
} cm_traj_score;
typedef struct cm_traj_info {          /* 24 bytes */
    uint32_t best;                     /* entry index of step 7, or CM_TRAJ_NONE */
    uint32_t n_valid;                  /* entries with status CM_TRAJ_VALID */
    float best_v, best_w;              /* the command of the best entry (0, 0 when there is none) */
    uint32_t start[2];                 /* the start's window cell (ix, iy) */
} cm_traj_info;
/* Non-NULL parameters allocate the layer and take the footprint (the scores are stale until the first evaluate); NULL frees
 * it (foot_xy and n_foot are then ignored). foot_xy: 2 * n_foot floats, (bx, by) per point. */
CM_API int cm_map_traj_configure(cm_ctx* ctx, const cm_traj_params* p, const float* foot_xy, uint32_t n_foot);
/* Rolls and scores every sample from the window's pose. *out may be NULL. */
CM_API int cm_map_traj_evaluate(cm_ctx* ctx, const cm_traj_window* w, cm_traj_info* out);
/* Host copy of the nv * nw scores; capacity in entries. Fewer than nv * nw: CM_CAPACITY (nothing is copied; *info, which may
 * be NULL, is still written). */
CM_API int cm_map_traj_copy(cm_ctx* ctx, cm_traj_score* host_dst, uint64_t capacity, cm_traj_info* info);
/* The same table in device memory owned by the context, valid until the next cm_map_traj_evaluate, cm_map_plan_update,
 * cm_map_cost_update, cm_map_integrate or configure call of the four layers. */
CM_API int cm_map_traj_device(cm_ctx* ctx, const void** scores, cm_traj_info* info);
/* The heading table of step 2: 2 * CM_TRAJ_HEADINGS floats. A host function: no context, no GPU. A capacity below
 * CM_TRAJ_HEADINGS pairs: CM_CAPACITY. */
CM_API int cm_traj_directions(float* cos_sin, uint64_t capacity_pairs);

/* ---- correlative scan matching of a frame against the occupancy map (an extension) -----------------------------------------
 * Every layer above takes the vehicle's pose from outside. This one finds it: the last frame is registered against the one
 * thing accumulated over time, the map, by an exhaustive search over a window of (yaw, x, y) around a prior pose, every
 * candidate scored by looking the frame's hit cells up in a likelihood field of the map (Olson's real-time correlative scan
 * matching, cartographer's RealTimeCorrelativeScanMatcher). The layer is configured once behind the cost layer
 * and evaluated on request. A score is an integer sum over a set of cells: the score volume is bit for bit a function of the
 * frame, the prior, the map's info and cell, dist2 and the parameters, whatever the order of summation.
 * Input: the last frame as cm_map_integrate sees it (the raw clouds in place, the keep and ground masks); the configured map
 * with its cell, inv, height band and the info (anchor, nx, ny) of its last integration; the cost layer's fresh dist2;
 * cm_match_params given at configure time; per evaluate a prior pose P, row-major 3 x 4 fp32 as for cm_map_integrate.
 *   1. Field table, built on the host in double from three fp32 values widened to double, the map's cell, sigma and max_dist:
 *      R = (uint32_t)ceil(max_dist / cell), the table has R * R + 1 bytes. lut[0] = 255. For d2 >= 1:
 *      m = sqrt((double)d2) * cell; m > max_dist gives 0, anything else
 *      (uint8_t)floor(255.0 * cm_exp_neg((m * m) / (2.0 * sigma * sigma))), every operation rounded once ((2.0 * sigma) *
 *      sigma; cm_exp_neg is cm_ndt_math.hpp's). A d2 beyond the table, CM_MAP_DIST_NONE included, has field value 0.
 *      cm_match_table returns the table of three values, cm_map_match_table_copy the configured layer's.
 *   2. Field. L(c) = lut[dist2(c)] for every window cell c; a cell outside the window has L = 0.
 *   3. Angle candidates k = -n_a .. n_a. Candidate k uses entry e_k = (k * a_stride) & 4095 of the CM_TRAJ_HEADINGS table
 *      (cm_traj_directions), (c, s). Its linear part is the prior's rows 0 and 1 rotated about world z through the vehicle's
 *      position: for j = 0..2, Q0j = c * P0j - s * P1j, Q1j = s * P0j + c * P1j in fp32, each product and the difference or
 *      sum rounded on its own, nothing fused (P0j is P[j], P1j is P[4 + j]). The translation stays (P3, P7). For k = 0 the
 *      entry is exactly (1, 0): Q equals P in value.
 *   4. Cells of a candidate. A counted point is what the map's step 3 calls a counted point of A: in A, valid, inside the
 *      closed height band. Its world cell under Q_k is the map's step 1 (wx = ((Q00*x + Q01*y) + Q02*z) + P3, wy likewise
 *      with row 1 and P7, floorf(w * inv), the same existence test) minus the map's current anchor. D_k is the set of distinct
 *      window cells of all sensors' counted points; a point whose cell does not exist or lies outside the window under Q_k is
 *      dropped for that k only.
 *   5. Score. For i = -wx .. wx, j = -wy .. wy: S(k, i, j) = sum over c in D_k of L(c + (i, j)) as uint32_t (with
 *      nx * ny <= 2^22 and bytes it cannot overflow); shifted cells outside the window contribute 0. The entry index is
 *      ((k + n_a) * (2 wy + 1) + (j + wy)) * (2 wx + 1) + (i + wx).
 *   6. Best. The entry with the largest S; ties go to the smallest i * i + j * j, then the smallest |k|, then the lowest
 *      entry index. An empty map, or a frame without counted points, gives all zeros: the prior wins.
 *   7. Sub-cell offset, with CM_MATCH_SUBCELL only, on the host in double from the volume, per axis (x along i, y along j):
 *      S-, S+ are the scores of the best entry's two neighbours along that axis (same k, same other index), S0 its own. If
 *      both neighbours exist and den = S- - 2 * S0 + S+ < 0 (in int64), sub = 0.5 * (double)(S- - S+) / (double)den, clamped
 *      to [-0.5, 0.5]; otherwise sub = 0. Without the flag both are 0.
 *   8. Result, cm_match_result: best (the entry index), k, i, j, score; n_cells = |D_k| of the best k and
 *      max_score = 255 * n_cells; yaw = (float)((double)(k * a_stride) * (6.283185307179586 / 4096.0)); sub[2]; pose[12]: rows
 *      0 and 1 are Q_k with pose[3] = P3 + (float)(((double)i + sub_x) * (double)cell), an fp32 addition, pose[7] likewise
 *      from P7, j and sub_y; row 2 is P's. A point's cell under `pose` need not equal its shifted cell of step 5 in the last
 *      bit (adding a rounded shift to the translation is not shifting the floor of the product): the score is defined by
 *      step 5, not by `pose`.
 * cm_map_match_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured cost layer; sigma or max_dist not
 * finite and > 0; R > CM_MATCH_MAX_RADIUS_CELLS; n_a > 127, a_stride == 0 or n_a * a_stride > 1024; wx or wy above
 * CM_MATCH_MAX_SHIFT; more than 2^22 candidates (2 n_a + 1)(2 wx + 1)(2 wy + 1); unknown flag bits; a frame in flight.
 * cm_map_match_evaluate refuses: no matching layer; a stale dist2 (or none yet); a map with n_frames == 0; everything
 * cm_map_integrate refuses about the result and the pose, except that matching a frame that was already integrated is legal.
 * All memory of the layer is taken by cm_map_match_configure (the field, the candidates' bitmaps, the volume, the tables, the
 * page-locked host words): no evaluate or copy allocates. The volume and the result are stale from cm_map_match_configure
 * and from every cm_map_integrate, cm_map_cost_update and merge until the next cm_map_match_evaluate: cm_map_match_copy and
 * cm_map_match_device then refuse with CM_BAD_ARG and say since which call. cm_map_cost_configure and cm_map_configure, in
 * either form, free the layer. It reads the map and the cost layer and writes buffers of its own only: no other layer's
 * tables or staleness change. With CM_FLAG_PROFILE, cm_get_stage_times after an evaluate lists match_clear, k_match_field,
 * k_match_mark, k_match_score, k_match_best. Not modelled: branch-and-bound or multi-resolution search (the window is searched
 * exhaustively), a covariance of the match, roll, pitch and z, weighting a cell by the number of its points. */
#define CM_MATCH_MAX_RADIUS_CELLS 64
#define CM_MATCH_MAX_SHIFT 64
#define CM_MATCH_MAX_ANGLES 127
#define CM_MATCH_MAX_CANDIDATES (1u << 22)
#define CM_MATCH_SUBCELL 1u
typedef struct cm_match_params {       /* 28 bytes, no padding */
    float sigma;                       /* standard deviation of the field (m); finite, > 0 */
    float max_dist;                    /* the field is 0 beyond it (m); finite, > 0, at most CM_MATCH_MAX_RADIUS_CELLS cells */
    uint32_t n_a;                      /* angle candidates -n_a .. n_a; at most CM_MATCH_MAX_ANGLES */
    uint32_t a_stride;                 /* heading-table entries between two candidates; >= 1, n_a * a_stride <= 1024 */
    uint32_t wx, wy;                   /* shifts -wx .. wx and -wy .. wy cells; each at most CM_MATCH_MAX_SHIFT */
    uint32_t flags;                    /* CM_MATCH_SUBCELL or 0 */
} cm_match_params;
typedef struct cm_match_result {       /* 96 bytes */
    uint32_t best;                     /* entry index of step 6 */
    int32_t k, i, j;                   /* its angle candidate and shift in cells */
    uint32_t score;                    /* S of the best entry */
    uint32_t n_cells;                  /* |D_k| of the best k */
    uint32_t max_score;                /* 255 * n_cells */
    float yaw;                         /* the best candidate's rotation (rad) */
    double sub[2];                     /* step 7's offsets along x and y in cells; 0 without CM_MATCH_SUBCELL */
    float pose[12];                    /* the matched pose, step 8 */
} cm_match_result;
/* Non-NULL parameters allocate the layer (volume and result are stale until the first evaluate); NULL frees it. */
CM_API int cm_map_match_configure(cm_ctx* ctx, const cm_match_params* p);
/* Matches the last frame against the map around the prior pose. *out may be NULL. */
CM_API int cm_map_match_evaluate(cm_ctx* ctx, const float pose[12], cm_match_result* out);
/* Host copy of the (2 n_a + 1)(2 wy + 1)(2 wx + 1) scores; capacity in entries. Fewer: CM_CAPACITY (nothing is copied; *out,
 * which may be NULL, is still written). */
CM_API int cm_map_match_copy(cm_ctx* ctx, uint32_t* host_dst, uint64_t capacity, cm_match_result* out);
/* The same volume in device memory owned by the context, valid until the next cm_map_match_evaluate, cm_map_cost_update,
 * cm_map_integrate, merge or configure call of the map, the cost layer or this layer. */
CM_API int cm_map_match_device(cm_ctx* ctx, const void** scores, cm_match_result* out);
/* The configured layer's field table; capacity in bytes, *n (may be NULL) its length R * R + 1. Too small: CM_CAPACITY. */
CM_API int cm_map_match_table_copy(cm_ctx* ctx, uint8_t* host_dst, uint64_t capacity, uint64_t* n);
/* Step 1's table for a cell, sigma and max_dist. A host function: no context, no GPU. CM_BAD_ARG: a value that is not finite
 * and > 0, R above CM_MATCH_MAX_RADIUS_CELLS, a NULL dst (nothing is written). Otherwise *n (may be NULL) = R * R + 1, and a
 * capacity below it: CM_CAPACITY (dst is not written). */
CM_API int cm_match_table(float cell, float sigma, float max_dist, uint8_t* dst, uint64_t capacity, uint64_t* n);

/* ---- branch-and-bound scan matching over wide windows of the map: the search layer (an extension) ----------------------------
 * The layer above searches its window exhaustively and is capped at CM_MATCH_MAX_SHIFT cells. This one returns the best entry
 * of the same definition over shifts of up to CM_MATCH_SEARCH_MAX_SHIFT cells without computing the volume: a pyramid of
 * block maxima of the field bounds whole blocks of shifts from above, and a block whose bound lies below a score already
 * found is dropped (cartographer's FastCorrelativeScanMatcher, with integer bounds: DESIGN.md §28). The bounds are sound, so
 * the result is exactly step 6's over the whole range; the way there is specified too, so that the statistics in
 * cm_match_search_info are a function of the inputs as well. A second layer behind the cost layer with buffers of its own: it
 * may be configured beside the layer above, and neither changes the other.
 * Input: as for cm_map_match_evaluate, with cm_match_search_params in the place of cm_match_params.
 *   1-4. Field table, field L, angle candidates Q_k and cell sets D_k: steps 1 to 4 above, word for word.
 *   5. Score. S(k, i, j) as in step 5 above over i = -wx .. wx, j = -wy .. wy, with the entry index
 *      ((k + n_a) * (2 wy + 1) + (j + wy)) * (2 wx + 1) + (i + wx) (it fits uint32_t: at most 255 * 2049 * 2049). The volume
 *      is never materialised.
 *   6. Best. As step 6 above: the largest S, ties to the smallest i * i + j * j, then the smallest |k|, then the lowest entry
 *      index. How it is found:
 *      a. Pyramid. L_0 = L; L_h(x, y) = max over 0 <= a, b < 2^h of L(x + a, y + b) for all integer (x, y), L being 0
 *         outside the window. Level h is stored as (ny + 2^h - 1) rows of (nx + 2^h - 1) bytes, entry
 *         [y + 2^h - 1][x + 2^h - 1] holding L_h(x, y); outside that storage L_h is 0. cm_map_match_search_level_copy
 *         returns a level.
 *      b. A node (h, k, i0, j0) stands for the entries of k with i0 <= i < i0 + 2^h, j0 <= j < j0 + 2^h that lie in the
 *         range. Its bound is U = sum over c in D_k of L_h(c + (i0, j0)) as uint32_t: U >= S of each of its entries, and at
 *         h = 0, U = S(k, i0, j0). Node order is ascending (k + n_a, j0, i0).
 *      c. Roots: h = depth, i0 = -wx + a * 2^depth for a = 0 .. ceil((2 wx + 1) / 2^depth) - 1, j0 likewise with wy, for
 *         every k; n_roots is their number. The children of a node at h > 0 are those of the four nodes
 *         (h - 1, k, i0 + a * 2^(h-1), j0 + b * 2^(h-1)), a, b in {0, 1}, with i0' <= wx and j0' <= wy.
 *      d. Bound B. All roots are scored. From the root of the largest U (ties: the first in node order) the search descends
 *         at every level to the child of the largest U (the same tie rule) down to a leaf (h = 0);
 *         B = max(S(that leaf), S(0, 0, 0)). B is not raised afterwards. n_probe counts the children scored on the way down
 *         plus one for the prior's entry (the roots are not counted: 1 at depth 0).
 *      e. Level loop. live_depth = the roots with U >= B; for h = depth .. 1 all children of live_h are scored and
 *         live_(h-1) = those with U >= B. scored[h] and live[h] are the numbers of nodes scored and kept at level h
 *         (scored[depth] = n_roots), 0 above depth. A node is dropped only if U < B, so every entry with S = max S has all
 *         its ancestors live and is in live_0, and step 6's rule over live_0 is step 6 over the whole volume.
 *      f. Capacities. If some |D_k| exceeds max_cells the evaluate returns CM_CAPACITY with
 *         overflow_level = CM_MATCH_SEARCH_OVERFLOW_CELLS and depth and n_roots set, everything else 0. If the live nodes of
 *         level h + 1 have more than max_nodes children it returns CM_CAPACITY with overflow_level = h, scored[h] their
 *         number, live[h] and everything below 0, and bound and n_probe set. Either way the result stays stale (the info is
 *         still written to *info). overflow_level is -1 otherwise. Both conditions are functions of the inputs.
 *   7. Sub-cell offset, with CM_MATCH_SUBCELL: step 7 above; the four neighbours' scores are computed directly as leaves, a
 *      neighbour outside [-wx, wx] or [-wy, wy] does not exist.
 *   8. Result: step 8 above, the same cm_match_result.
 * cm_map_match_search_configure refuses with CM_BAD_ARG: no configured cost layer; sigma or max_dist not finite and > 0;
 * R > CM_MATCH_MAX_RADIUS_CELLS; n_a > 127, a_stride == 0 or n_a * a_stride > 1024; wx or wy above
 * CM_MATCH_SEARCH_MAX_SHIFT; depth above CM_MATCH_SEARCH_MAX_DEPTH; max_nodes or max_cells 0 or above
 * CM_MATCH_SEARCH_MAX_NODES; more roots than max_nodes; a map window with nx or ny above 65535; unknown flag bits; a frame in
 * flight. cm_map_match_search refuses what cm_map_match_evaluate refuses, with this layer in the place of that one. All
 * memory of the layer is taken by cm_map_match_search_configure (the pyramid with the table behind it, the candidates'
 * bitmaps and cell lists of max_cells words each, two node lists and one score list of max_nodes words, the roots, the
 * page-locked host words): no evaluate or copy allocates. Result, info and pyramid are stale from
 * cm_map_match_search_configure and from every cm_map_integrate, cm_map_cost_update and merge until the next successful
 * cm_map_match_search: cm_map_match_search_result and cm_map_match_search_level_copy then refuse with CM_BAD_ARG and say
 * since which call. cm_map_cost_configure and cm_map_configure, in either form, free the layer. It reads the map and the
 * cost layer and writes buffers of its own only: no other layer's tables or staleness change, the exhaustive layer's
 * included. With CM_FLAG_PROFILE, cm_get_stage_times after an evaluate lists msearch_clear, k_match_field,
 * k_msearch_pyramid, k_match_mark, k_msearch_list, k_msearch_score, k_msearch_pick, k_msearch_select, k_msearch_best, equally
 * named launches added up (the host's waits for a level's counts fall to k_msearch_select). Not modelled: raising B during
 * the level loop or a best-first order, a covariance of the match, roll, pitch and z, cell weights. */
#define CM_MATCH_SEARCH_MAX_SHIFT 1024
#define CM_MATCH_SEARCH_MAX_DEPTH 7
#define CM_MATCH_SEARCH_MAX_NODES (1u << 22)
#define CM_MATCH_SEARCH_OVERFLOW_CELLS (-2)
typedef struct cm_match_search_params { /* 40 bytes (ten words), no padding */
    float sigma;                       /* as cm_match_params */
    float max_dist;
    uint32_t n_a;
    uint32_t a_stride;
    uint32_t wx, wy;                   /* shifts -wx .. wx and -wy .. wy cells; each at most CM_MATCH_SEARCH_MAX_SHIFT */
    uint32_t depth;                    /* the roots' level; at most CM_MATCH_SEARCH_MAX_DEPTH */
    uint32_t max_nodes;                /* room of a level's node list; 1 .. CM_MATCH_SEARCH_MAX_NODES, at least n_roots */
    uint32_t max_cells;                /* room of a candidate's cell list; 1 .. CM_MATCH_SEARCH_MAX_NODES */
    uint32_t flags;                    /* CM_MATCH_SUBCELL or 0 */
} cm_match_search_params;
typedef struct cm_match_search_info {  /* 84 bytes */
    uint32_t depth;
    uint32_t n_roots;
    uint32_t bound;                    /* B */
    uint32_t scored[8];                /* nodes scored in the level loop, by level */
    uint32_t live[8];                  /* those with U >= B */
    uint32_t n_probe;                  /* nodes scored for B beyond the roots */
    int32_t overflow_level;            /* -1: none; h: the children at level h; CM_MATCH_SEARCH_OVERFLOW_CELLS */
} cm_match_search_info;
/* Non-NULL parameters allocate the layer (result, info and pyramid are stale until the first evaluate); NULL frees it. */
CM_API int cm_map_match_search_configure(cm_ctx* ctx, const cm_match_search_params* p);
/* Matches the last frame against the map around the prior pose. *out and *info may be NULL. CM_CAPACITY: step 6f (*info is
 * written, *out is not). */
CM_API int cm_map_match_search(cm_ctx* ctx, const float pose[12], cm_match_result* out, cm_match_search_info* info);
/* The last result and info again; either may be NULL. */
CM_API int cm_map_match_search_result(cm_ctx* ctx, cm_match_result* out, cm_match_search_info* info);
/* Host copy of level h <= depth of the last evaluate's pyramid; capacity in bytes; dims (may be NULL) = {columns, rows} =
 * {nx + 2^h - 1, ny + 2^h - 1}. Too small: CM_CAPACITY (nothing is copied; dims is still written). */
CM_API int cm_map_match_search_level_copy(cm_ctx* ctx, uint32_t h, uint8_t* host_dst, uint64_t capacity, uint32_t dims[2]);

/* ---- frontier layer behind the plan layer: connected frontiers of the occupancy map (an extension) ------------------------
 * Where to go when nobody gives a goal: every exploration stack over an occupancy grid (Yamauchi's frontiers,
 * frontier_exploration, explore_lite) takes the cells where known free space meets the unknown, groups them into connected
 * frontiers and ranks those by their size and the cost of getting there. The frontier layer is configured once behind the
 * plan layer and recomputed on request. Every quantity below is an integer and every reduction commutative
 * (count, sum, min, max), and a component is named by its smallest cell: labels, table and info are bit for bit a function
 * of the three input tables and the parameters, whatever the order in which the device works.
 * Input: the map's image I (int8_t, entry ix + iy * nx: -1 unknown, 0 free, 100 occupied), the cost layer's fresh cost table,
 * the plan layer's fresh pot, and the map's info. In exploration the caller sets the plan's goal to the vehicle's position
 * (cm_map_plan_update with the pose's x and y): pot(c) is then the exact cost of the cheapest walk between c and the vehicle
 * by the plan layer's steps 3 and 4, where a step charges k times the weight of the cell left behind when walking towards
 * the goal, that is, of the cell farther from the vehicle.
 *   1. Frontier cell. c is a frontier cell iff I(c) == 0, cost(c) <= max_cost, and at least one of its four edge neighbours
 *      inside the window has I == -1. A cell outside the window is not unknown: what scrolled out is forgotten.
 *   2. Components. Frontier cells are 8-connected, with no corner rule: a diagonal pair is connected. A component's
 *      first_cell is its smallest cell index ix + iy * nx.
 *   3. Frontiers. A component with n_cells >= min_cells is a frontier. Frontiers are numbered from 0 in ascending order of
 *      first_cell.
 *   4. Labels. One uint32_t per window cell (entry ix + iy * nx): the frontier's number for the cells of a frontier,
 *      CM_FRONTIER_NONE for every other cell, the frontier cells of components below min_cells among them. Numbers at or
 *      above max_frontiers still appear in the labels.
 *   5. Table. cm_frontier, entry k = frontier k, the first n_written = min(n_frontiers, max_frontiers) of them: first_cell,
 *      n_cells; sum_x, sum_y, the sums of ix and of iy over the frontier's cells (the centroid is the caller's division; 64
 *      bits, since 4 M cells times 2047 do not fit 32); min_pot, the smallest pot over the frontier's cells, and
 *      min_pot_cell, the lowest cell index that has it (every cell CM_PLAN_UNREACHABLE: CM_PLAN_UNREACHABLE and
 *      CM_FRONTIER_NONE; min_pot is then "not defined"); x0, y0, x1, y1, the closed bounding box in window cells.
 *   6. Choice. For a table entry with min_pot defined, score = pot_scale * min_pot - gain_scale * n_cells as an integer
 *      (explore_lite's cost in integers); both products fit 64 unsigned bits, the difference is exact, and a score above
 *      INT64_MAX is stored and compared as INT64_MAX: nothing wraps. best is the entry with the lowest score, ties go to
 *      the lowest number. No entry with min_pot defined: best is CM_FRONTIER_NONE and best_score 0.
 *   7. Info. cm_frontier_info: n_frontier_cells (step 1), n_components (step 2), n_frontiers (step 3), n_written (step 5),
 *      best and best_score (step 6).
 * cm_map_frontier_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured plan layer (or none of its
 * parents); min_cells 0; max_frontiers 0 or above CM_FRONTIER_MAX_TABLE; max_cost above 252; a frame in flight. All memory of
 * the layer is taken by cm_map_frontier_configure (the labels, a size word per cell, the counts of the numbering scan, the
 * table and its box scratch, the page-locked info words): no update allocates, and nothing is kept per cell but those two
 * words. The layer is stale from cm_map_frontier_configure and from every cm_map_integrate, cm_map_cost_update and
 * cm_map_plan_update until the next cm_map_frontier_update, which itself refuses a stale plan layer: the copies and
 * cm_map_frontier_device then refuse with CM_BAD_ARG and say since which call. cm_map_plan_configure, cm_map_cost_configure
 * and cm_map_configure, in either form, free the layer; like the map it survives merges, and nothing else depends on whether
 * it exists: not a frame, the map, or any other layer's bytes. With CM_FLAG_PROFILE, cm_get_stage_times after an update
 * lists k_front_local, k_front_merge, k_front_flatten, k_front_count, k_front_scan, k_front_number, k_front_table and
 * k_front_best. Not modelled: 4-connectivity, frontiers of unknown cells as explore_lite defines them (its frontier cells are
 * the unknown cells beside free ones), a blacklist of frontiers, a "middle" cell, frontiers outside the window. */
#define CM_FRONTIER_NONE 0xFFFFFFFFu
#define CM_FRONTIER_MAX_TABLE 65536u
typedef struct cm_frontier_params {    /* 20 bytes, no padding */
    uint32_t min_cells;                /* >= 1: the smallest component that is a frontier */
    uint32_t max_frontiers;            /* 1..CM_FRONTIER_MAX_TABLE: entries of the table */
    uint32_t max_cost;                 /* 0..252: the largest cost byte of a frontier cell; 252 admits every passable cell */
    uint32_t pot_scale;                /* step 6 */
    uint32_t gain_scale;
} cm_frontier_params;
typedef struct cm_frontier {           /* 40 bytes */
    uint32_t first_cell, n_cells;
    uint64_t sum_x, sum_y;
    uint32_t min_pot, min_pot_cell;
    uint16_t x0, y0, x1, y1;
} cm_frontier;
typedef struct cm_frontier_info {      /* 32 bytes */
    uint32_t n_frontier_cells;
    uint32_t n_components;
    uint32_t n_frontiers;
    uint32_t n_written;
    uint32_t best;                     /* a table entry, or CM_FRONTIER_NONE */
    uint32_t _pad;
    int64_t best_score;
} cm_frontier_info;
/* Non-NULL parameters allocate the layer (it is stale until the first update); NULL frees it. */
CM_API int cm_map_frontier_configure(cm_ctx* ctx, const cm_frontier_params* p);
/* Computes labels, table and info from the map's image and the fresh cost and plan layers. *out and *map (either may be
 * NULL) are the layer's and the map's info. */
CM_API int cm_map_frontier_update(cm_ctx* ctx, cm_frontier_info* out, cm_map_info* map);
/* Host copy of the table's n_written entries; capacity in entries. Fewer: CM_CAPACITY (nothing is copied; *info, which may
 * be NULL, is still written). */
CM_API int cm_map_frontier_copy(cm_ctx* ctx, cm_frontier* host_dst, uint64_t capacity, cm_frontier_info* info);
/* Host copy of the labels; capacity in cells. Fewer than nx * ny: CM_CAPACITY (nothing is copied; *info is still written). */
CM_API int cm_map_frontier_labels_copy(cm_ctx* ctx, uint32_t* host_dst, uint64_t capacity_cells, cm_frontier_info* info);
/* Both in device memory owned by the context (nx * ny words; n_written entries of cm_frontier), valid until the next
 * cm_map_frontier_update, cm_map_plan_update, cm_map_cost_update, cm_map_integrate or configure call of the four layers. */
CM_API int cm_map_frontier_device(cm_ctx* ctx, const void** labels, const void** table, cm_frontier_info* info);

/* ---- the localisation layer: a particle filter against the occupancy map (an extension) -----------------------------------
 * The matching layers return the single best entry of a lattice around one prior. This layer keeps a belief over poses: a set
 * of particles that carries several hypotheses from frame to frame, takes odometry between frames and can start without a
 * prior (Monte Carlo localisation against a likelihood field, amcl). It is configured once behind the cost
 * layer; its calls are init, predict and update. Scores and weights are integers, positions are fp32 with every operation
 * rounded on its own, noise is an integer sum of fields of a counter-based draw and resampling is integer systematic
 * resampling: the particles, the weight table and the info are bit for bit a function of the frame, the map's info, cell and
 * image, dist2, the parameters and the sequence of calls.
 * Constants: W1 = 65536 (weight one); K = 4294967296.0 / 6.283185307179586 (the rollout layer's); K1 = sqrt(3.0 /
 * 4294967295.0) in double; umul64hi(a, b) is the high 64 bits of the 128-bit product.
 *   1. Particle, cm_mcl_particle (24 bytes): x, y (fp32) in the map's world frame; h, a binary angle, a full turn is 2^32,
 *      whose direction (c, s) is entry ((h + 0x80000) >> 20) & 4095 of the CM_TRAJ_HEADINGS table (cm_traj_directions); parent;
 *      acc (uint64_t).
 *   2. Draws. gen counts the layer's init, predict and update calls since cm_map_mcl_configure that were not refused; the
 *      first has gen = 0 (sharpened: a refused call draws nothing and does not count). base = splitmix64(seed + gen), wrapping.
 *      draw(p, i) = splitmix64(base ^ ((uint64_t)p << 8) ^ i) for i < 256; splitmix64 is the ground stage's function
 *      (x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *      z ^ z >> 31). The noise integer n(u) of a draw u is the sum of its four 16-bit fields minus 131070, in
 *      [-131070, 131070], of mean 0 and variance (2^32 - 1) / 3. A noise value for a standard deviation sd (fp32, >= 0) is
 *      (float)n * sc with sc = (float)((double)sd * K1), computed once per call on the host: one fp32 product. cm_mcl_draws
 *      returns draw(p, i) for a range of p.
 *   3. Init around a pose (x0, y0, yaw0) with (sd_x, sd_y, sd_yaw): x_p = x0 + (float)n(draw(p, 0)) * sc_x, y_p likewise with
 *      draw 1 and sc_y, h_p = the low 32 bits of (int64_t)rint(((double)yaw0 + (double)((float)n(draw(p, 2)) * sc_yaw)) * K);
 *      acc = 0, parent = p.
 *   4. Init over the free space. The free cells are the window cells whose image byte is 0, in ascending entry order, n_free of
 *      them. Particle p takes the free cell of rank umul64hi(draw(p, 0), n_free), window cell (ix, iy). ux = (float)(draw(p, 1)
 *      >> 40) * 0x1p-24f; x_p = ((float)(ax + ix) + ux) * cell: a conversion, a sum and a product, each rounded; y_p likewise
 *      with draw 2 and ay + iy; h_p = (uint32_t)(draw(p, 3) >> 32); acc = 0, parent = p. Whether floorf(x_p * inv) lands in
 *      that very cell is not promised and not needed.
 *   5. Predict with the vehicle-frame motion since the last predict (d_fwd, d_left, d_yaw) and its standard deviations, which
 *      the caller passes as the rollout takes its dynamic window from outside. With (c, s) of h_p before the turn:
 *      a = d_fwd + (float)n(draw(p, 0)) * sc_fwd, b = d_left + (float)n(draw(p, 1)) * sc_left; x' = (x + c * a) - s * b,
 *      y' = (y + s * a) + c * b, each operation rounded (the form of the rollout's step 4); h' = h + the low 32 bits of
 *      (int64_t)rint(((double)d_yaw + (double)((float)n(draw(p, 2)) * sc_yaw)) * K), wrapping. acc and parent stay.
 *   6. Beams of an update, from the last frame as cm_map_match_evaluate sees it. A counted point is a point of A that is valid
 *      and inside the map's closed height band. Its (x, y) is taken in the common frame: no pose is applied, the body frame is
 *      taken as level. Per axis the body cell is b = floorf(x * inv) with the map's existence test; a point is dropped where
 *      either |b| > range_cells. D is the set of distinct body cells over all sensors, n_cells = |D|, ordered by (b_y, b_x)
 *      ascending. stride = max(1, ceil(n_cells / max_beams)); the beams are the cells of rank 0, stride, 2 stride, ...:
 *      n_beams = ceil(n_cells / stride). A beam's point is its cell's centre: fx = ((float)b_x + 0.5f) * cell, fy likewise.
 *   7. Score. The field L is steps 1 and 2 of the matching layer, unchanged. For particle p and every beam:
 *      wx = (x_p + c * fx) - s * fy, wy = (y_p + s * fx) + c * fy, each operation rounded; the cell of (wx, wy) is the map's
 *      step 1 minus the anchor; it contributes L if it exists and lies in the window, otherwise 0. S_p is the sum as uint32_t
 *      (at most 8192 * 255); acc_p += S_p.
 *   8. Weights. A = max acc_p, d_p = A - acc_p, W_p = (uint32_t)floor(65536.0 * cm_exp_neg((double)d_p * beta)) with
 *      beta = 1.0 / (255.0 * (double)tau) computed once on the host (cm_exp_neg is cm_ndt_math.hpp's). The best particle has
 *      W = 65536, so sum_w >= 65536. cm_mcl_weight is {S_p, W_p}, in the order of the particles the update found.
 *   9. Estimate, all sums int64 / uint64 and exact. q(v) = clamp(llrint((double)v * 1024.0), -2^30, 2^30), and 0 for a v that
 *      is not finite. ci = (int)rint(c * 32768.0f), si likewise. sum_w = sum W, sum_w2 = sum W^2, sum_wqx = sum W q(x),
 *      sum_wqy, sum_wc = sum W ci, sum_ws = sum W si. best is the particle with the largest acc, ties to the lowest index.
 *      mq_x = floor(sum_wqx / sum_w) as integers, mq_y likewise; dq = clamp(q - mq, -32768, 32767) per axis; sum_wdxx, sum_wdyy
 *      and sum_wdxy are the sums of W dq_x^2, W dq_y^2 and W dq_x dq_y. The arithmetic: W <= 2^16 and at most 2^16 particles,
 *      so sum_w <= 2^32 and sum_w2 <= 2^48; |q| <= 2^30, so |sum_wq| <= 2^62; |ci| <= 2^15, so |sum_wc| <= 2^47;
 *      |dq| <= 2^15, so the spread sums stay within 2^62: every sum is below 2^63. On the host in double:
 *      mean_x = ((double)sum_wqx / (double)sum_w) / 1024.0, mean_y likewise; mean_yaw = atan2((double)sum_ws, (double)sum_wc);
 *      var_xx = (double)sum_wdxx / ((double)sum_w * 1048576.0), var_yy and var_xy likewise (m^2, about the integer mean);
 *      n_eff = ((double)sum_w * (double)sum_w) / (double)sum_w2.
 *  10. Resampling happens iff CM_MCL_RESAMPLE_ALWAYS is set or n_eff < (double)resample_frac * (double)n_particles. T = sum_w,
 *      r = umul64hi(splitmix64(base ^ (1ull << 63)), T), C the inclusive prefix sum of W in particle order. New particle j
 *      copies (x, y, h) of the smallest p with C_p > (j * T + r) / N (integer division); its parent = p and its acc = 0.
 *      Without resampling the particles stay and parent = own index.
 *  11. cm_mcl_info: n_particles, n_cells, stride, n_beams, the gen of the update, resampled, best, the best particle's x, y, h
 *      before resampling, every sum of step 9, n_eff, the means and the three spread terms.
 * cm_map_mcl_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured cost layer; n_particles outside
 * 1..CM_MCL_MAX_PARTICLES, max_beams outside 1..CM_MCL_MAX_BEAMS, range_cells outside 1..CM_MCL_MAX_RANGE_CELLS; sigma and
 * max_dist as cm_map_match_configure refuses them; tau not finite and > 0; resample_frac not finite or outside 0..1; unknown
 * flag bits; a frame in flight. cm_map_mcl_init_pose refuses a value that is not finite, a negative sd, |yaw0| > 1024 and an sd
 * above 1024; cm_map_mcl_predict the same of its six values (|d_yaw| <= 1024), and particles that are not yet initialised.
 * cm_map_mcl_init_uniform refuses a map with n_frames == 0 and an image without a free cell. cm_map_mcl_update refuses what
 * cm_map_match_evaluate refuses (a stale dist2, a map with n_frames == 0, everything about the result), and particles that are
 * not yet initialised. All memory of the layer is taken by cm_map_mcl_configure (two particle buffers, the weight table, the
 * prefix sums, the field and its table, one bitmap and one list that serve the body cells and the free cells, the info words and
 * their page-locked copy): no other call allocates. Sharpened: the particles are the layer's state, not a table of the map; they
 * are readable (cm_map_mcl_copy) from the first init on, whatever happens to the map. The weight table and the info are stale
 * from cm_map_mcl_configure and from every cm_map_integrate, cm_map_load, cm_map_cost_update, merge, init and predict until the
 * next cm_map_mcl_update: cm_map_mcl_weights_copy and cm_map_mcl_device then refuse with CM_BAD_ARG and say since which call.
 * cm_map_cost_configure and cm_map_configure, in either form, free the layer. It reads the map and the cost layer and writes
 * buffers of its own only: no other layer's tables or staleness change. A NULL context leaves every output untouched. With
 * CM_FLAG_PROFILE, cm_get_stage_times after an update lists mcl_clear, k_match_field, k_mcl_mark, k_mcl_compact, k_mcl_score,
 * k_mcl_best, k_mcl_weights, k_mcl_spread, k_mcl_resample. The beam model's terms and occlusion are a mode of their own (the
 * next section), and so are pose hypotheses, the KLD bound and random-particle injection (the section after it). Not modelled: a
 * particle count that changes between updates, roll, pitch and z, weighting a cell by the number of its points. */
#define CM_MCL_MAX_PARTICLES 65536
#define CM_MCL_MAX_BEAMS 8192
#define CM_MCL_MAX_RANGE_CELLS 1024
#define CM_MCL_WEIGHT_ONE 65536
#define CM_MCL_RESAMPLE_ALWAYS 1u
typedef struct cm_mcl_params {         /* 40 bytes, no padding */
    uint32_t n_particles;              /* 1 .. CM_MCL_MAX_PARTICLES */
    uint32_t max_beams;                /* 1 .. CM_MCL_MAX_BEAMS */
    uint32_t range_cells;              /* body cells beyond it are dropped; 1 .. CM_MCL_MAX_RANGE_CELLS */
    float sigma, max_dist;             /* the field, exactly cm_match_params' */
    float tau;                         /* temperature of the weights, in mean field bytes; finite, > 0 */
    float resample_frac;               /* resample when n_eff < resample_frac * n_particles; finite, 0 .. 1 */
    uint32_t flags;                    /* CM_MCL_RESAMPLE_ALWAYS or 0 */
    uint64_t seed;
} cm_mcl_params;
typedef struct cm_mcl_particle {       /* 24 bytes */
    float x, y;                        /* position in the map's world frame (m) */
    uint32_t h;                        /* heading, a binary angle */
    uint32_t parent;                   /* the particle of the last update it was copied from; its own index otherwise */
    uint64_t acc;                      /* scores accumulated since it was initialised or resampled */
} cm_mcl_particle;
typedef struct cm_mcl_weight {         /* 8 bytes */
    uint32_t score;                    /* S_p of the update */
    uint32_t weight;                   /* W_p, 0 .. CM_MCL_WEIGHT_ONE */
} cm_mcl_weight;
typedef struct cm_mcl_info {           /* 176 bytes */
    uint32_t n_particles, n_cells, stride, n_beams;
    uint64_t gen;                      /* the gen of the update */
    uint32_t resampled, best;
    float best_x, best_y;              /* the best particle before resampling */
    uint32_t best_h, _pad;
    uint64_t sum_w, sum_w2;
    int64_t sum_wqx, sum_wqy, sum_wc, sum_ws;
    int64_t sum_wdxx, sum_wdyy, sum_wdxy;
    double n_eff, mean_x, mean_y, mean_yaw;
    double var_xx, var_yy, var_xy;
} cm_mcl_info;
/* Non-NULL parameters allocate the layer (no particles yet, gen = 0); NULL frees it. */
CM_API int cm_map_mcl_configure(cm_ctx* ctx, const cm_mcl_params* p);
/* Step 3. */
CM_API int cm_map_mcl_init_pose(cm_ctx* ctx, float x0, float y0, float yaw0, float sd_x, float sd_y, float sd_yaw);
/* Step 4, over the map's current image. */
CM_API int cm_map_mcl_init_uniform(cm_ctx* ctx);
/* Step 5. */
CM_API int cm_map_mcl_predict(cm_ctx* ctx, float d_fwd, float d_left, float d_yaw, float sd_fwd, float sd_left, float sd_yaw);
/* Steps 6 to 11 with the last frame. *out may be NULL. */
CM_API int cm_map_mcl_update(cm_ctx* ctx, cm_mcl_info* out);
/* Host copy of the n_particles particles after the last call; capacity in particles. Fewer: CM_CAPACITY (nothing is copied). */
CM_API int cm_map_mcl_copy(cm_ctx* ctx, cm_mcl_particle* host_dst, uint64_t capacity);
/* Host copy of the last update's weight table; capacity in entries. Fewer: CM_CAPACITY (nothing is copied; *info, which may be
 * NULL, is still written). */
CM_API int cm_map_mcl_weights_copy(cm_ctx* ctx, cm_mcl_weight* host_dst, uint64_t capacity, cm_mcl_info* info);
/* Both in device memory owned by the context, valid until the next call of this layer or configure call of the map, the cost
 * layer or this layer. Any of the three outputs may be NULL. */
CM_API int cm_map_mcl_device(cm_ctx* ctx, const void** particles, const void** weights, cm_mcl_info* info);
/* draw(p, i) of step 2 for p = first_p .. first_p + n_p - 1 into dst. A host function: no context, no GPU. CM_BAD_ARG: i >= 256,
 * a NULL dst, first_p + n_p above 2^32 (nothing is written). */
CM_API int cm_mcl_draws(uint64_t seed, uint64_t gen, uint32_t first_p, uint32_t n_p, uint32_t i, uint64_t* dst);

/* ---- the beam model of the localisation layer: rays cast per beam (an extension) -------------------------------------------
 * The field score of step 7 looks at a beam's end cell only: a pose whose beams end on a far wall after passing through a
 * near one scores like the true pose. The beam model is a second scoring mode of the same layer (amcl's beam model with its
 * hit, short and random terms). cm_map_mcl_beam_configure switches it on; it is off by default, and with it off
 * every byte of the layer is what it is without this section. With it on, step 7 above is replaced by the steps below; steps
 * 1 to 6 and 8 to 11 stay word for word. E = over_cells. Everything after the two cells is integer arithmetic: the weight
 * table, both infos and the particles stay bit for bit a function of the inputs.
 *   1. Origin cell. o is the map's step 1 of (x_p, y_p) minus the anchor. If it does not exist or lies outside the window,
 *      every beam of p is `skipped` and S_p = 0.
 *   2. End cell. (wx, wy) is computed exactly as in step 7 above, with the same rounded operations. g is its cell minus the
 *      anchor. If it does not exist, the beam is `skipped` and adds 0. g may lie outside the window.
 *   3. Line. (dx, dy) = g - o and L = max(|dx|, |dy|). The line is cm_result_grid_rays' step 5: the cell at step k is
 *      o + (rdiv(k dx, L), rdiv(k dy, L)). It is followed for k = 0 .. L + E. With L = 0 only k = 0 (the origin cell) is looked
 *      at. The bound on |dx|, |dy|: a beam's body cell has |b| <= range_cells, so |fx|, |fy| <= (range_cells + 0.5) cell; the
 *      heading table's (c, s) are fp32 roundings of a cosine and a sine, c^2 + s^2 <= 1 + 2^-22, so the exact
 *      |c fx - s fy| <= sqrt(2) (1 + 2^-23) (range_cells + 0.5) cell, 1448.87 cells at range_cells 1024, and likewise for y.
 *      Two cells whose coordinates differ by t cells have indices that differ by less than t + 1. The roundings: with M the
 *      largest |cell index| of the window, each of the two sums and each of the two products x * inv is off by at most
 *      2^-24 (M + 1450) cells (the two inner products by 2^-24 * 1024.5 cells, which 1448.87 already leaves room for), in all
 *      below 2^-22 (M + 1450). So |dx|, |dy| < 1449.87 + 2^-22 (M + 1450), which is at most 1450 = CM_MCL_BEAM_MAX_D whenever
 *      2^-22 (M + 1450) <= 1.12: every window within 2^22 cells of the world origin (200 km at a 5 cm cell). Sharpened: a beam with |dx| or |dy| above
 *      CM_MCL_BEAM_MAX_D, which only a window farther out can produce, is `skipped` and adds 0.
 *   4. Walk, in order of k. A cell outside the window ends the ray as `off`. I == 100 ends it as a hit at k*; an occupied
 *      origin cell is a hit at 0. -1 and 0 are passed through, as in the cast layer. No hit through L + E is `beyond`.
 *   5. Outcome. A hit has e = max(k* - L, -E); it counts as `early` for e < 0, `at` for e == 0 and `late` for e > 0. The table
 *      index is e + E for a hit, 2E + 1 for `beyond` and 2E + 2 for `off`. Sharpened: with L = 0 a free or unknown origin cell
 *      is `beyond`, whatever E is, and an occupied one is `at`.
 *   6. Table, 2E + 3 bytes, built once on the host in double, every operation rounded once, with cm_exp_neg of
 *      cm_ndt_math.hpp, sc = (double)sigma / (double)cell and s2 = (2.0 * sc) * sc:
 *      T[e + E] = rint(255 * min(1, (z_hit * cm_exp_neg((double)(e * e) / s2) + (e > 0 ? z_short : 0)) + z_rand)),
 *      T[2E + 1] = rint(255 * (z_short + z_rand)), T[2E + 2] = rint(255 * z_rand); ties go to even. cm_mcl_beam_table returns
 *      it.
 *   7. Score. S_p is the sum of the table bytes over the beams, at most 8192 * 255; acc_p += S_p, as in step 7 above.
 *   8. Counts, cm_mcl_beam_info: n_rays = n_particles * n_beams of the update and the six outcome counts over all
 *      (p, beam), integer sums; the host checks that they add up to n_rays.
 * CM_MCL_BEAM_PLAIN selects a device walk that does what step 4 says, cell by cell, reading the image. Without it the device
 * skips cells that dist2 proves free of an occupied cell, by the cast layer's rule; the outputs are the same bytes either way.
 * The mode does not need a configured cast layer.
 * cm_map_mcl_beam_configure refuses with CM_BAD_ARG (cm_last_error says why): a frame in flight; no localisation layer (or
 * no layer above it), in that layer's words; over_cells above CM_MCL_BEAM_MAX_OVER; sigma not finite and > 0; a z that is not
 * finite, z_hit not > 0, z_short or z_rand below 0, a sum above 1 (in double, in the order written); unknown flag bits. A
 * refused call changes nothing. An accepted call, with parameters or NULL, takes or gives back all the mode's memory (one byte
 * per window cell for the skips, the table, the count words and their page-locked copy: no other call allocates), leaves the
 * particles and gen alone (it is not one of the calls gen counts, so no draw changes) and makes the weight table and both infos
 * stale "since cm_map_mcl_beam_configure" until the next cm_map_mcl_update. cm_map_mcl_configure in either form switches the
 * mode off and frees it, and so does everything that frees the layer. cm_map_mcl_update refuses exactly what it refuses without
 * the mode. cm_map_mcl_beam_info_copy refuses what cm_map_mcl_weights_copy refuses, and a last update that ran without the
 * mode. A NULL context leaves every output untouched. With CM_FLAG_PROFILE the stage list of an update has k_mcl_beam in place
 * of k_mcl_score, and k_mcl_steps in front of it only in the first beam update after a cm_map_cost_update (or after the
 * configure call), never under CM_MCL_BEAM_PLAIN. Not modelled: a z_max term of its own (a ray without a hit takes the short
 * and random terms), sub-cell ranges, unknown cells as obstacles, a per-beam weight. */
#define CM_MCL_BEAM_MAX_OVER 64
#define CM_MCL_BEAM_MAX_D 1450
#define CM_MCL_BEAM_PLAIN 1u
typedef struct cm_mcl_beam_params {    /* 24 bytes, no padding */
    uint32_t over_cells;               /* E: how far past the measured end a ray is followed; 0 .. CM_MCL_BEAM_MAX_OVER */
    float sigma;                       /* of the hit term, metres; finite, > 0 */
    float z_hit, z_short, z_rand;      /* finite, each >= 0, z_hit > 0, their sum <= 1 */
    uint32_t flags;                    /* CM_MCL_BEAM_PLAIN or 0 */
} cm_mcl_beam_params;
typedef struct cm_mcl_beam_info {      /* 56 bytes */
    uint64_t n_rays;                   /* n_particles * n_beams of the update */
    uint64_t n_early, n_at, n_late, n_beyond, n_off, n_skipped;   /* their sum is n_rays */
} cm_mcl_beam_info;
/* Non-NULL parameters switch the beam model on (or replace its parameters); NULL goes back to the field score. */
CM_API int cm_map_mcl_beam_configure(cm_ctx* ctx, const cm_mcl_beam_params* p);
/* The counts of the last update, which must have run the beam model. */
CM_API int cm_map_mcl_beam_info_copy(cm_ctx* ctx, cm_mcl_beam_info* out);
/* The table of step 6 for a map of this cell: 2 * over_cells + 3 bytes. A host function: no context, no GPU. CM_BAD_ARG: NULL
 * p or dst, parameters cm_map_mcl_beam_configure refuses, a cell that is not finite and > 0; a smaller capacity: CM_CAPACITY
 * (nothing is written). */
CM_API int cm_mcl_beam_table(const cm_mcl_beam_params* p, float cell, uint8_t* dst, uint64_t capacity);

/* ---- pose hypotheses and random-particle recovery of the localisation layer (an extension) ----------------------------------
 * cm_mcl_info reports one weighted mean over all particles. While the belief has two modes that mean lies between them, and
 * after a kidnapping every particle scores equally badly, n_eff stays high and nothing is ever drawn elsewhere. This mode adds
 * what amcl adds: the clusters of the belief (pf_cluster_stats), the KLD bound on the particle count, and the injection of
 * random particles steered by a slow and a fast average of the score (recovery_alpha_slow / _fast).
 * cm_map_mcl_hyp_configure switches it on; it is off by default, and with it off every byte, stage name and refusal of the
 * layer is what it is without this section. With inject_max = 0 the particles, the weight table and cm_mcl_info are byte for
 * byte those of the mode off. "Steps" are those of the localisation layer above. Everything is integer arithmetic on keys and
 * sums except the few doubles named below, whose every operation is written out: the hypotheses and the info are bit for bit
 * a function of the inputs.
 * The hypotheses are computed in every update while the mode is on, over the particles as the update found them: acc after
 * the score of step 7, W of step 8, before the resampling of step 10: the particles cm_mcl_info's estimate is defined over.
 *   H1. Bins. With q of step 9 and floor division of integers (q = -1 lies in bin -1): bx = floor(q(x) / bin_q),
 *       by = floor(q(y) / bin_q); bh = h >> (32 - heading_bits), and 0 when heading_bits = 0. |q| <= 2^30 and bin_q >= 64, so
 *       |bx|, |by| <= 2^24. key = ((uint64_t)(by + 2^24) << 34) | ((uint64_t)(bx + 2^24) << 8) | bh: keys order bins by
 *       (by, bx, bh).
 *   H2. Occupied bins. n_bins is the number of distinct keys.
 *   H3. Neighbours and components. Two occupied bins are neighbours when |by - by'| <= 1, |bx - bx'| <= 1 and bh - bh' is -1, 0
 *       or 1 modulo 2^heading_bits: headings wrap (amcl's do not). With heading_bits = 0 or 1 every two heading bins are
 *       neighbours. A component is a connected set of occupied bins; its label is its smallest key. n_components counts all
 *       of them.
 *   H4. Per component, over its particles, exact integers within the bounds of step 9 (a component is a subset of the
 *       particles): n; sum_w, sum_wqx, sum_wqy, sum_wc, sum_ws with ci, si of step 9; top, the particle with the largest W,
 *       ties to the lowest index. mq_x = floor(sum_wqx / sum_w), mq_y likewise; dq = clamp(q - mq, -32768, 32767) per axis;
 *       sum_wdxx, sum_wdyy, sum_wdxy are the sums of W dq_x^2, W dq_y^2, W dq_x dq_y. A component with sum_w = 0 has mq = 0,
 *       zero spread sums and 0.0 in every double of H5.
 *   H5. Order and output. Components are ordered by sum_w descending, ties by label ascending. The first
 *       n_hyp = min(n_components, max_hyp) become cm_mcl_hyp records. Their doubles are computed on the host from the
 *       component's sums exactly as step 9 computes the global ones: mean_x = ((double)sum_wqx / (double)sum_w) / 1024.0,
 *       mean_y likewise, mean_yaw = atan2((double)sum_ws, (double)sum_wc), var_xx = (double)sum_wdxx / ((double)sum_w *
 *       1048576.0), var_yy and var_xy likewise. share = (double)sum_w / (double)(step 9's sum_w over all particles).
 *   H6. KLD bound. n_kld = cm_mcl_kld_bound(n_bins, kld_err, kld_z), on the host in double, every operation rounded once: 1
 *       for k <= 1; otherwise a = 2.0 / (9.0 * (double)(k - 1)), b = (1.0 - a) + sqrt(a) * (double)z,
 *       n = ceil(((double)(k - 1) / (2.0 * (double)err)) * ((b * b) * b)), clamped to 1 .. 2^32 - 1 (a value that is not a
 *       number gives 2^32 - 1). It is reported only.
 * The recovery, in every update while the mode is on; inject_max bounds what it may do.
 *   R1. Average score. sum_s = the sum of S_p over the particles, exact and below 2^38. With n_beams of cm_mcl_info: if
 *       n_beams = 0 the two averages stay as they are, n_inject = 0 and w_avg and p_inject are reported as 0.0. Otherwise
 *       w_avg = (double)sum_s / (((double)n_particles * (double)n_beams) * 255.0): both products are exact, the division is
 *       rounded once.
 *   R2. Slow and fast average. w_slow becomes w_avg when it is 0.0, otherwise w_slow + a_slow * (w_avg - w_slow): a
 *       difference, a product and a sum, each rounded, nothing fused; a_slow = (double)alpha_slow. w_fast likewise with
 *       alpha_fast. Both are 0.0 after cm_map_mcl_hyp_configure and after every cm_map_mcl_init_pose / _init_uniform that was
 *       not refused.
 *   R3. Injection count. p_inject = 1.0 - w_fast / w_slow when w_slow > 0 and w_fast < w_slow (the new values), else 0.0.
 *       n_inject = min(inject_max, (uint32_t)floor(p_inject * (double)n_particles)), and 0 when the map's image has no free
 *       cell. The averages are not reset after an injection (amcl's reset stops the injection after one round).
 *       n_free is the number of free cells of the map's current image (step 4), and 0 when inject_max = 0: no list is built.
 *   R4. Resampling happens iff step 10's condition holds or n_inject > 0. m = n_particles - n_inject (>= 1). New particle
 *       j < m copies (x, y, h) of the smallest p with C_p > (j * T + r) / m, with T, r and C of step 10, parent = p, acc = 0:
 *       with n_inject = 0 this is step 10 word for word. New particle j >= m is step 4 over the free cells of the map's
 *       current image with draw(j, 0 .. 3) of this update's base (an update uses no draw(p, i) otherwise); its parent is
 *       CM_MCL_NO_PARENT and its acc is 0. cm_mcl_info's resampled is 1 whenever resampling happened.
 * cm_mcl_hyp_info: the gen of the update, n_bins, n_components, n_hyp, n_kld, n_inject, n_free, sum_s, w_avg, w_slow and
 * w_fast after R2, p_inject.
 * cm_map_mcl_hyp_configure refuses with CM_BAD_ARG (cm_last_error says why): a frame in flight; no localisation layer (or no
 * layer above it), in that layer's words; bin_q outside 64 .. 1048576; heading_bits above 8; max_hyp outside
 * 1 .. CM_MCL_HYP_MAX; inject_max above n_particles - 1; an alpha that is not finite or not 0 <= alpha_slow <= alpha_fast <= 1;
 * kld_err not finite or outside 0 < kld_err <= 1; kld_z not finite and > 0; flags or _pad not 0. A refused call changes
 * nothing. An accepted call, with parameters or NULL, takes or gives back all the mode's memory (the table of bins of
 * a power of two >= 4 n_particles slots with a parent and a component word per slot, a slot word and a record per particle,
 * the chosen records, the mode's words, a bitmap and a list of the free cells, and a page-locked copy of what an update reads
 * back: no other call allocates), leaves the particles and gen alone (it is not one of the calls gen counts) and makes the
 * weight table, the infos and the hypotheses stale "since cm_map_mcl_hyp_configure" until the next cm_map_mcl_update.
 * cm_map_mcl_configure in either form switches the mode off and frees it, and so does everything that frees the layer. The
 * mode and the beam model do not know of each other. cm_map_mcl_update refuses exactly what it refuses without the mode.
 * cm_map_mcl_hyp_copy refuses what cm_map_mcl_weights_copy refuses, and a last update that ran without the mode; a capacity
 * below n_hyp is CM_CAPACITY (nothing is copied; *info, which may be NULL, is still written). A NULL context leaves every
 * output untouched. With CM_FLAG_PROFILE the stage list of an update has, between k_mcl_spread and k_mcl_resample:
 * mcl_hyp_clear, k_mcl_hyp_bins, k_mcl_hyp_link, k_mcl_hyp_flatten, k_mcl_hyp_sums, k_mcl_hyp_spread, k_mcl_hyp_pick, then
 * k_mcl_free_bits and k_mcl_compact only where inject_max > 0, then k_mcl_hyp_recover. Not modelled: a particle count that
 * follows n_kld, amcl's reset of the averages, a cluster's heading spread. */
#define CM_MCL_HYP_MAX 64
#define CM_MCL_NO_PARENT 0xFFFFFFFFu
typedef struct cm_mcl_hyp_params {     /* 40 bytes, no padding */
    uint32_t bin_q;                    /* bin width in 1/1024 m; 64 .. 1048576 */
    uint32_t heading_bits;             /* 2^heading_bits heading bins; 0 .. 8 */
    uint32_t max_hyp;                  /* 1 .. CM_MCL_HYP_MAX */
    uint32_t inject_max;               /* most particles one update may inject; 0: no injection; <= n_particles - 1 */
    float alpha_slow, alpha_fast;      /* finite, 0 <= alpha_slow <= alpha_fast <= 1 */
    float kld_err, kld_z;              /* finite, 0 < kld_err <= 1, kld_z > 0 */
    uint32_t flags, _pad;              /* 0 */
} cm_mcl_hyp_params;
typedef struct cm_mcl_hyp {            /* 136 bytes */
    uint64_t label;                    /* the smallest key of the component */
    uint32_t n, top;                   /* its particles; the heaviest of them */
    uint64_t sum_w;
    int64_t sum_wqx, sum_wqy, sum_wc, sum_ws;
    int64_t sum_wdxx, sum_wdyy, sum_wdxy;
    double share, mean_x, mean_y, mean_yaw;
    double var_xx, var_yy, var_xy;
} cm_mcl_hyp;
typedef struct cm_mcl_hyp_info {       /* 72 bytes */
    uint64_t gen;                      /* the gen of the update */
    uint32_t n_bins, n_components, n_hyp, n_kld, n_inject, n_free;
    uint64_t sum_s;
    double w_avg, w_slow, w_fast, p_inject;
} cm_mcl_hyp_info;
/* Non-NULL parameters switch the mode on (or replace its parameters; the averages start at 0.0); NULL switches it off and
 * frees it. */
CM_API int cm_map_mcl_hyp_configure(cm_ctx* ctx, const cm_mcl_hyp_params* p);
/* The hypotheses of the last update, which must have run the mode, in the order of H5; capacity in records. */
CM_API int cm_map_mcl_hyp_copy(cm_ctx* ctx, cm_mcl_hyp* host_dst, uint64_t capacity, cm_mcl_hyp_info* info);
/* H6 for k bins. A host function: no context, no GPU. CM_BAD_ARG: a NULL out, err not finite or outside 0 < err <= 1, z not
 * finite and > 0 (nothing is written). */
CM_API int cm_mcl_kld_bound(uint32_t k, float err, float z, uint32_t* out);

/* ---- the cast layer: expected ranges from many poses in the occupancy map (an extension) ----------------------------------
 * Every other layer looks single cells up. This one answers what the map was built by ray casting to answer: from this pose,
 * in this direction, how far is the first occupied cell? It serves a beam model, a virtual LaserScan of the map, visibility
 * from a candidate pose and simulated scans. It is configured once behind the cost layer and evaluated on
 * request for n poses x n_bearings rays. Everything after the origin cell is integer arithmetic: the rays and the info are bit
 * for bit a function of the map's image, info and cell, the parameters, the bearings and the poses.
 * Input: the map's image I as cm_map_occupancy_copy returns it, the map's info (anchor, nx, ny) and cell, the cost layer's
 * fresh dist2 (it only lets the device skip: no output depends on it), the parameters, the bearings and per evaluation n poses.
 *   1. Pose, cm_cast_pose (12 bytes): x, y (fp32) in the map's world frame and h, a binary angle, a full turn is 2^32. The
 *      origin cell is step 1 of the map's semantics per axis (floorf(x * inv), the same existence test) minus the map's
 *      anchor. An origin whose cell does not exist (NaN, +-inf, beyond +-2^30) or lies outside the window gives every ray of
 *      that pose {status CM_CAST_NO_ORIGIN, k 0, jx 0, jy 0}.
 *   2. Bearings. n_bearings binary angles b_a, taken at configure time; a NULL list means evenly spaced,
 *      b_a = (uint32_t)(((uint64_t)a << 32) / n_bearings). Ray (p, a) has the heading H = h_p + b_a, wrapping; its direction
 *      entry is e = ((H + 0x80000) >> 20) & 4095, the rollout layer's rule.
 *   3. Direction table. 4096 pairs of int16_t, built once on the host from the CM_TRAJ_HEADINGS table (c_e, s_e) of
 *      cm_traj_directions: E_e = (rint((double)c_e * (double)range_cells), rint((double)s_e * (double)range_cells)), ties to
 *      even. cm_cast_directions returns it. With (dx, dy) = E_e, L = max(|dx|, |dy|). L >= 1 for every entry and every
 *      range_cells >= 1: the table's angle th lies within pi / 4 of an axis, so the larger of |cos th| and |sin th| is at least
 *      cos(pi / 4) = 0.7071..., its fp32 rounding is at least 0.70710677, the product with range_cells >= 1 is at least that
 *      and rint of a value >= 0.5000...1 is at least 1. |c_e|, |s_e| <= 1 gives |dx|, |dy| <= range_cells: int16_t holds them.
 *   4. Line: cm_result_grid_rays' step 5, unchanged. At step k the ray's cell is o + (rdiv(k * dx, L), rdiv(k * dy, L)) for
 *      k = 0 .. L; unlike the map's rays the end cell (k = L) is included.
 *   5. Walk. For k = 0, 1, .., L in order: a cell outside the window ends the ray with status CM_CAST_OFF_MAP, and step
 *      k - 1 is reported (k >= 1 here: the origin is inside); else I(cell) == 100 ends it with status CM_CAST_HIT at step k;
 *      I == -1 and I == 0 are both passed through. After step L without either the status is CM_CAST_MAX at step L. An
 *      occupied origin cell is a HIT at k = 0.
 *   6. Record, cm_cast_ray (8 bytes): k, the reported step; status; a zero byte; jx, jy, the reported step's cell minus the
 *      origin cell. Ray (p, a) is entry p * n_bearings + a. The metric range is not part of the table
 *      (cell * sqrt(jx^2 + jy^2)).
 *   7. cm_cast_info: n_poses, n_bearings and the four status counts over all rays (integer sums).
 * CM_CAST_PLAIN selects a device walk that does what steps 4 and 5 say, cell by cell, reading the image. Without it the
 * device skips cells that dist2 proves free of an occupied cell (DESIGN.md §30 has the rule and its proof); the outputs are
 * the same bytes either way.
 * cm_map_cast_configure refuses with CM_BAD_ARG (cm_last_error says why): no configured cost layer; max_poses outside
 * 1..CM_CAST_MAX_POSES, n_bearings outside 1..CM_CAST_MAX_BEARINGS, range_cells outside 1..CM_CAST_MAX_RANGE_CELLS;
 * max_poses * n_bearings above CM_CAST_MAX_RAYS; unknown flag bits; a frame in flight. cm_map_cast_evaluate refuses: no layer; a
 * stale or absent dist2 (no cm_map_cost_update since the last cm_map_integrate, cm_map_load or cm_map_cost_configure); n of 0
 * or above max_poses; NULL poses; a frame in flight. cm_map_cast_evaluate_mcl casts from the localisation layer's current
 * particles (x, y, h read from the 24-byte records in place; n = n_particles, refused above max_poses) and is refused without
 * initialised particles; it changes nothing of that layer. A map with n_frames == 0 is allowed: every ray then ends MAX or
 * OFF_MAP. All memory of the layer is taken by cm_map_cast_configure (the rays, the poses, the bearings, the direction table,
 * one byte per window cell for the skips, the count words and their page-locked copy): no other call allocates. The rays and
 * the info are stale from cm_map_cast_configure and from every cm_map_integrate, cm_map_load and cm_map_cost_update until the
 * next evaluate: cm_map_cast_copy and cm_map_cast_device then refuse with CM_BAD_ARG and say since which call.
 * cm_map_cost_configure and cm_map_configure, in either form, free the layer. It reads the map, the cost layer and the
 * particles and writes buffers of its own only: no other layer's tables, staleness or timing change. A NULL context leaves
 * every output untouched. With CM_FLAG_PROFILE, cm_get_stage_times after an evaluate lists cast_upload, k_cast_steps (only in
 * the first evaluate after a cm_map_cost_update, and never under CM_CAST_PLAIN) and k_cast_rays. Not modelled: stopping at or
 * counting unknown cells, sub-cell origins (a ray starts at its origin cell's centre, as the map's own rays do), 3-D casting.
 * cm_map_mcl_update does not read this layer's table: its beam model (cm_map_mcl_beam_configure) casts its own rays, from
 * each particle towards each beam's end cell, with the same line and the same skip rule. */
#define CM_CAST_MAX_POSES 65536
#define CM_CAST_MAX_BEARINGS 4096
#define CM_CAST_MAX_RANGE_CELLS 1024
#define CM_CAST_MAX_RAYS 16777216
#define CM_CAST_PLAIN 1u
#define CM_CAST_MAX 0                  /* status values, not bits */
#define CM_CAST_HIT 1
#define CM_CAST_OFF_MAP 2
#define CM_CAST_NO_ORIGIN 3
typedef struct cm_cast_params {        /* 16 bytes, no padding */
    uint32_t max_poses;                /* 1 .. CM_CAST_MAX_POSES; max_poses * n_bearings <= CM_CAST_MAX_RAYS */
    uint32_t n_bearings;               /* 1 .. CM_CAST_MAX_BEARINGS */
    uint32_t range_cells;              /* the reach of a ray in cells; 1 .. CM_CAST_MAX_RANGE_CELLS */
    uint32_t flags;                    /* CM_CAST_PLAIN or 0 */
} cm_cast_params;
typedef struct cm_cast_pose {          /* 12 bytes */
    float x, y;                        /* position in the map's world frame (m) */
    uint32_t h;                        /* heading, a binary angle */
} cm_cast_pose;
typedef struct cm_cast_ray {           /* 8 bytes, ray (p, a) is entry p * n_bearings + a */
    uint16_t k;                        /* the reported step */
    uint8_t status;                    /* CM_CAST_MAX, _HIT, _OFF_MAP or _NO_ORIGIN */
    uint8_t _pad;                      /* zero */
    int16_t jx, jy;                    /* the reported step's cell minus the origin cell */
} cm_cast_ray;
typedef struct cm_cast_info {          /* 24 bytes */
    uint32_t n_poses, n_bearings;
    uint32_t n_max, n_hit, n_off_map, n_no_origin;   /* rays by status; their sum is n_poses * n_bearings */
} cm_cast_info;
/* Non-NULL parameters allocate the layer and take the bearings (n_bearings of them, or NULL: evenly spaced); NULL parameters
 * free it. */
CM_API int cm_map_cast_configure(cm_ctx* ctx, const cm_cast_params* p, const uint32_t* bearings);
/* Steps 1 to 7 for n poses. *out may be NULL. */
CM_API int cm_map_cast_evaluate(cm_ctx* ctx, const cm_cast_pose* host_poses, uint32_t n, cm_cast_info* out);
/* The same from the localisation layer's current particles. */
CM_API int cm_map_cast_evaluate_mcl(cm_ctx* ctx, cm_cast_info* out);
/* Host copy of the n_poses * n_bearings rays of the last evaluate; capacity in rays. Fewer: CM_CAPACITY (nothing is copied;
 * *info, which may be NULL, is still written). */
CM_API int cm_map_cast_copy(cm_ctx* ctx, cm_cast_ray* host_dst, uint64_t capacity, cm_cast_info* info);
/* The same table in device memory owned by the context, valid until the next evaluate or configure call of the map, the cost
 * layer or this layer. Either output may be NULL. */
CM_API int cm_map_cast_device(cm_ctx* ctx, const void** rays, cm_cast_info* info);
/* The direction table of step 3 for range_cells: 2 * 4096 int16_t. A host function: no context, no GPU. CM_BAD_ARG: a NULL
 * dst, range_cells outside 1..CM_CAST_MAX_RANGE_CELLS; a capacity below 4096 pairs: CM_CAPACITY (nothing is written). */
CM_API int cm_cast_directions(uint32_t range_cells, int16_t* dst, uint64_t capacity_pairs);

/* ---- surface normals and curvature of the result (pcl::NormalEstimation, setKSearch; an extension) --------------------
 * One unit normal and one curvature per published point, estimated from its k nearest neighbours in the published cloud,
 * computed on request after a frame. Input: the n = n_out records of the last result, c_0 .. c_{n-1} in the
 * order of cm_result_copy, their x, y, z as fp32.
 *   1. Distance. d2(i, j) = (dx*dx + dy*dy) + dz*dz, dx = c_i.x - c_j.x ..., fp32, round-to-nearest, no contraction: the
 *      distance of the radius, statistical-outlier and cluster stages. It may be +inf; it is never NaN.
 *   2. Neighbourhood. N_i is i itself plus the m - 1 other indices j with the smallest (d2(i, j), j) in lexicographic order,
 *      m = min(k, n): ties in distance go to the smaller result index, exact duplicates count (at distance 0). r2_k and
 *      last are the d2 and the index of the last of them. The table is therefore a function of the result alone.
 *   3. Moments, in fp64, every operation rounded on its own, no contraction. Offsets e_j = double(c_j) - double(c_i) per
 *      axis; s_a = sum e_a and S_ab = sum e_a e_b, added one neighbour after the other from 0 in the ascending (d2, j) order
 *      of step 2 (the point itself contributes zeros); mu = s / m; C_ab = S_ab / m - mu_a mu_b for a >= b, mirrored.
 *      (The deviation from PCL 1.8, which accumulates raw coordinates in fp32 and so cancels away from the origin — §12
 *      records the effect; offsets about the query point are what later PCL versions use.)
 *   4. Plane. The eigenvalues l0 <= l1 <= l2 of C by cyclic Jacobi rotations in fp64. normal: the eigenvector of l0,
 *      normalised in fp64; curvature |l0 / (l0 + l1 + l2)|; orientation by PCL's flipNormalTowardsViewpoint: with
 *      v = double(viewpoint) - double(c_i) a normal with n.v < 0 is negated (at n.v == 0 the sign is unspecified). The
 *      outputs are rounded to fp32.
 *   5. Validity. An entry is valid (CM_NORMAL_VALID) when m >= 3, l2 > 0 and every figure is finite; otherwise flags is 0
 *      and normal and curvature are NaN. n_neighbors, r2_k and last are written in either case.
 * Entry i belongs to result record i. The table is owned by the context and valid until the next merge or the next call.
 * search_cell sets the cells of the search grid and with them the speed of the call, never its result. CM_FLAG_OCCUPANCY is
 * not required. Refused with CM_BAD_ARG (cm_last_error says why): a frame in flight, no result, a result of cm_merge_partial
 * / cm_merge_tables, a last status other than CM_OK (no voxel grid), k outside 3..CM_NORMAL_MAX_K, a viewpoint that is not
 * finite, a search_cell that is negative or not finite. No later frame depends on whether the table was asked for; with
 * CM_FLAG_PROFILE, cm_get_stage_times afterwards lists the stages of this call. */
#define CM_NORMAL_MAX_K 64
#define CM_NORMAL_VALID 1u
typedef struct cm_normal_params {
    uint32_t k;                        /* setKSearch: the point itself plus its k-1 nearest others; 3..CM_NORMAL_MAX_K */
    float viewpoint[3];                /* setViewPoint, common frame; finite. PCL's default is (0,0,0) */
    float search_cell;                 /* edge (m) of the search grid's cells: speed only, never the result; 0 = library's choice */
    uint32_t _pad;
} cm_normal_params;
typedef struct cm_voxel_normal {       /* 32 bytes */
    float normal[3];                   /* unit; NaN unless valid */
    float curvature;                   /* lambda_0 / (lambda_0 + lambda_1 + lambda_2); NaN unless valid */
    float r2_k;                        /* fp32 squared distance to the farthest neighbour used (0 when there is none) */
    uint32_t n_neighbors;              /* m = min(k, n_out): points in the neighbourhood, the point itself included */
    uint32_t last;                     /* result index of that farthest neighbour (the entry's own index when m == 1) */
    uint32_t flags;                    /* CM_NORMAL_* */
} cm_voxel_normal;
/* Host copy; capacity in entries, fewer than n_out: CM_CAPACITY (nothing is computed or copied). */
CM_API int cm_result_normals(cm_ctx* ctx, const cm_normal_params* p, cm_voxel_normal* host_dst, uint64_t capacity);
/* The same table left in device memory owned by the context (*n entries of 32 bytes; NULL when the result is empty). */
CM_API int cm_result_normals_device(cm_ctx* ctx, const cm_normal_params* p, const void** dev_ptr, uint64_t* n);

/* ---- point-to-plane ICP registration of a cloud against the result (an extension) --------------------------------------
 * Aligns a source cloud to the last result with its normals (Chen & Medioni's point-to-plane error, linearised about a
 * pivot), computed on request after a frame. Source: n_src 16-byte records (x, y, z as fp32, the fourth word
 * ignored: the format of cm_result_copy, so a previous result feeds straight in), n_src < 2^30. Target: the n = n_out records
 * c_0 .. c_{n-1} of the last result and their normals at normals_k (cm_result_normals). A pose T = [R|t] is 12 doubles,
 * row-major 3x4; it is never rounded to fp32. One evaluation E(T):
 *   1. Transform. q64 = ((r00*x + r01*y) + r02*z) + t0 and likewise for the other rows, x = double(src.x) ..., fp64, every
 *      operation rounded on its own, no contraction. qf = float(q64) per axis.
 *   2. Match. j(i) is the result index with the smallest (d2(qf_i, c_j), j) in lexicographic order among those with
 *      d2 < float(max_corr_dist * max_corr_dist); d2 = (dx*dx + dy*dy) + dz*dz in fp32, the distance of the cluster and
 *      normals stages; strict <; ties go to the smaller result index. No such j, or a qf that is not finite: the
 *      correspondence is idx = CM_ALIGN_NONE, d2 = 0.
 *   3. Terms, for every matched i whose target normal is CM_NORMAL_VALID (every other i contributes +0.0), in fp64, every
 *      operation rounded on its own. p0 = pivot = double(mn) + (double(mx) - double(mn)) * 0.5 per axis, mn / mx the fp32
 *      bounds of the result's records. a = q64 - p0, b = double(c_j) - p0, n = double(normal_j);
 *      res = (n0*(a0-b0) + n1*(a1-b1)) + n2*(a2-b2); J = [a x n, n] (6 entries). The 28 terms: J_u J_v for u >= v (the lower
 *      triangle of H, row by row), J_u res (g), res*res (sse); and the integer count n_corr of the i that have terms.
 *   4. Sums in a defined order, so that the result is a function of the inputs alone. Terms sit at their source index in
 *      aligned blocks of 256. Inside 64 consecutive indices v[l] += v[l + s] for s = 32, 16, 8, 4, 2, 1 and v[0] is their
 *      sum; a block is ((w0 + w1) + w2) + w3; the block sums are added one after the other in ascending order from 0.0.
 *      The sign of a normal cancels exactly in every term: the viewpoint the normals were turned to never matters.
 * The loop, on the host, for it = 0 .. max_iterations - 1: E(T_it); n_corr < min_correspondences: stop. Solve H x = -g by
 * LDL^T without pivoting in fp64; a pivot <= CM_ALIGN_PIVOT_MIN * max_i H_ii (or NaN): CM_ALIGN_SINGULAR, stop, pose
 * unchanged. x = (w, v) is a twist about the pivot: R' = Rodrigues(w) R, t' = Rodrigues(w)(t - p0) + p0 + v; iterations
 * counts these updates. Converged (CM_ALIGN_CONVERGED, stop) when |w| < rot_eps and |v| < trans_eps. All max_iterations
 * updates applied without that: CM_ALIGN_MAX_ITER_HIT. After the loop one more E(T_final) fills H, g, sse, n_corr,
 * rms = sqrt(sse / n_corr) (0 without terms) and the correspondence table; CM_ALIGN_FEW is set iff that n_corr is below
 * min_correspondences. max_iterations 0 is that evaluation alone at the guess: a nearest-neighbour and fitness query.
 * The normals are those of cm_result_normals at normals_k: a table the context already holds for this result at that k is
 * used as it is, otherwise the call computes it (viewpoint 0, search_cell 0) — the outcome is the same bytes either way.
 * Refused with CM_BAD_ARG (cm_last_error says why): what cm_result_normals refuses about the result, a max_corr_dist that is
 * not finite and > 0 or whose fp32 square is 0 or not finite, normals_k outside 3..CM_NORMAL_MAX_K, max_iterations above
 * CM_ALIGN_MAX_ITER, min_correspondences below 6, an eps that is negative or NaN, a guess that is not finite, a NULL source
 * with n_src > 0, n_src >= 2^30. n_src 0 is CM_OK with CM_ALIGN_FEW. The call reads the result and the normals table and
 * writes only buffers of its own; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists one entry per kernel of the call,
 * its milliseconds summed over the evaluations. */
#define CM_ALIGN_MAX_ITER 64
#define CM_ALIGN_NONE 0xFFFFFFFFu
#define CM_ALIGN_PIVOT_MIN 1e-9
#define CM_ALIGN_CONVERGED 1u
#define CM_ALIGN_MAX_ITER_HIT 2u
#define CM_ALIGN_FEW 4u
#define CM_ALIGN_SINGULAR 8u
typedef struct cm_align_params {       /* 128 bytes */
    float max_corr_dist;               /* matching radius r, metres */
    uint32_t max_iterations;           /* 0..CM_ALIGN_MAX_ITER */
    uint32_t normals_k;                /* 3..CM_NORMAL_MAX_K */
    uint32_t min_correspondences;      /* >= 6 */
    double trans_eps, rot_eps;         /* >= 0; 0: never converged by that criterion */
    double guess[12];                  /* row-major 3x4 [R|t], used verbatim as T_0 */
} cm_align_params;
typedef struct cm_align_result {       /* 368 bytes */
    double pose[12];                   /* final pose, row-major 3x4 */
    double H[21];                      /* lower triangle, row by row, at the final pose */
    double g[6];
    double sse, rms;
    double pivot[3];
    uint64_t n_corr;
    uint32_t iterations;               /* updates applied */
    uint32_t flags;                    /* CM_ALIGN_* */
} cm_align_result;
typedef struct cm_align_corr {         /* 8 bytes */
    uint32_t idx;                      /* result index, or CM_ALIGN_NONE */
    float d2;                          /* fp32 squared distance to it (0 without a match) */
} cm_align_corr;
CM_API int cm_result_align(cm_ctx* ctx, const cm_align_params* p, const void* src_host, uint64_t n_src, cm_align_result* out);
/* The same with the source already in device memory, read in place. */
CM_API int cm_result_align_device(cm_ctx* ctx, const cm_align_params* p, const void* src_dev, uint64_t n_src,
                                  cm_align_result* out);
/* The correspondences of the last call's final evaluation, entry i for source record i. *n: the entries (written whenever
 * there was such a call); more than capacity: CM_CAPACITY (nothing is copied). No call since the last merge: CM_BAD_ARG. */
CM_API int cm_align_correspondences_copy(cm_ctx* ctx, cm_align_corr* host_dst, uint64_t capacity, uint64_t* n);

/* ---- NDT registration of a cloud against the per-voxel covariance table (an extension) ----------------------------------
 * Aligns a source cloud to the last result's voxel statistics (cm_result_voxel_cov at `cov`; Biber & Strasser's normal
 * distributions transform with Magnusson's score), computed on request after a frame. It needs no
 * nearest-neighbour search and no normals: the result's voxel keys are sorted, and a voxel is found by one binary search.
 * Source, pose and pivot are cm_result_align's: n_src 16-byte records, 12 doubles row-major 3x4 never rounded to fp32, the
 * midpoint of the result's fp32 bounds. All fp64 work is rounded per operation, no contraction. One evaluation E(T):
 *   0. Constants, on the host with std::log / std::exp: res3 = (double(leaf0) * double(leaf1)) * double(leaf2) of the frame,
 *      p = double(outlier_ratio), c1 = 10 (1 - p), c2 = p / res3, d3 = -log(c2), d1 = -log(c1 + c2) - d3,
 *      d2 = -2 log((-log(c1 exp(-0.5) + c2) - d3) / d1) (PCL's gauss_d1 / gauss_d2; returned). d2h = d2 * 0.5.
 *   1. Transform: cm_result_align's step 1, q64 and qf = float(q64).
 *   2. Voxels of a point, in the grid of the result's keys (inv = the frame's fp32 1 / leaf, min_b / div_b the grid's origin
 *      cell and extent): per axis v_a = fsub(floorf(fmul(qf_a, inv_a)), float(min_b_a)) in fp32. A qf that is not finite, or
 *      a v_a outside [-1, float(div_a)] on any axis (tested in float), has no voxel. Otherwise c_a = (int)v_a and the
 *      candidates are c, c - e0, c + e0, c - e1, c + e1, c - e2, c + e2 in this order (neighborhood 1: the first alone). A
 *      candidate counts only if every coordinate lies in [0, div_a) as an integer, per axis — never on the linear key, so a
 *      neighbour across the x border does not alias into the next row. It is USED iff its key c0 + c1 div0 + c2 div0 div1 is
 *      among the result's keys, its table entry is CM_COV_VALID, and m below is finite and >= 0.
 *   3. Terms per used voxel j: a = q64 - p0, b = double(mean_j) - p0, r = a - b, B = double(icov_j);
 *      u_i = (B_i0 r_0 + B_i1 r_1) + B_i2 r_2; m = (r_0 u_0 + r_1 u_1) + r_2 u_2; w = cm_exp_neg(d2h * m) (cm_ndt_math.hpp:
 *      the exponential spelled out, 0 for an argument >= 700). The Jacobian columns of a twist about the pivot:
 *      c_0 = (0, -a2, a1), c_1 = (a2, 0, -a0), c_2 = (-a1, a0, 0), c_3..5 = e_0..2; y_v = B c_v and z_u = c_u . u in the same
 *      three-term form (exact zeros and ones may be skipped: values are compared, the sign of a zero is free). The 28 terms:
 *      w (c_u . y_v) for u >= v row by row (H), w z_u (g), w (score). A point's terms are added over its used voxels in
 *      candidate order from 0.0; n_corr counts the points with at least one used voxel.
 *   4. Sums: cm_result_align's step 4 unchanged.
 * The loop is cm_result_align's: solve H x = -g by LDL^T without pivoting, x a twist about the pivot, the same stops, flags
 * and final evaluation; CM_NDT_FEW iff the final n_corr is below min_correspondences. This is iteratively reweighted
 * Gauss-Newton on NDT's score: each step minimises the quadratic that majorises -sum exp(-d2h m) at the current weights. It
 * is the one deviation from pcl::NormalDistributionsTransform, which takes Newton steps with the full Hessian and a
 * More-Thuente line search over Euler angles; H here is positive semi-definite by construction, which is why LDL^T without
 * pivoting suffices.
 * The table is cm_result_voxel_cov's at `cov`: one the context already holds for this result at these parameters is used as
 * it is, otherwise the call computes it — the outcome is the same bytes either way.
 * Refused with CM_BAD_ARG (cm_last_error says why): everything cm_result_voxel_cov refuses (a context without
 * CM_FLAG_OCCUPANCY among it), an outlier_ratio that is not finite or outside (0, 1), a d2 that is not finite and > 0, a
 * neighborhood other than 1 or 7, max_iterations above CM_NDT_MAX_ITER, min_correspondences below 6, an eps that is negative
 * or NaN, a guess that is not finite, a NULL source with n_src > 0, n_src >= 2^30. A refused call leaves
 * *out as it was. (d2 fails only where c1 vanishes beside c2: an outlier_ratio next to 1 at a leaf volume below about 1e-10.)
 * n_src 0 is CM_OK with CM_NDT_FEW. The call reads the result, its keys and the covariance table and writes only buffers of
 * its own; with CM_FLAG_PROFILE, cm_get_stage_times afterwards lists one entry per kernel of the call, its milliseconds summed
 * over the evaluations, and before them an entry "voxel_cov" iff the call computed the table itself. */
#define CM_NDT_MAX_ITER 64
#define CM_NDT_NONE 0xFFFFFFFFu
#define CM_NDT_CONVERGED 1u            /* the same four meanings as CM_ALIGN_* */
#define CM_NDT_MAX_ITER_HIT 2u
#define CM_NDT_FEW 4u
#define CM_NDT_SINGULAR 8u
typedef struct cm_ndt_params {         /* 136 bytes, no padding */
    float outlier_ratio;               /* PCL's 0.55; finite, in (0, 1) */
    uint32_t neighborhood;             /* 1: the voxel that holds the point; 7: it and its six face neighbours */
    uint32_t max_iterations;           /* 0..CM_NDT_MAX_ITER */
    uint32_t min_correspondences;      /* >= 6 */
    cm_cov_params cov;                 /* the table used; {0, 0}: the default {6, 0.01f} */
    double trans_eps, rot_eps;         /* >= 0; 0: never converged by that criterion */
    double guess[12];                  /* row-major 3x4 [R|t], used verbatim as T_0 */
} cm_ndt_params;
typedef struct cm_ndt_result {         /* 376 bytes */
    double pose[12];                   /* final pose, row-major 3x4 */
    double H[21];                      /* lower triangle, row by row, at the final pose */
    double g[6];
    double score;                      /* sum of the weights w at the final pose */
    double gauss_d1, gauss_d2;         /* the constants the call used */
    double pivot[3];
    uint64_t n_corr;                   /* source points with at least one voxel used */
    uint32_t iterations;               /* updates applied */
    uint32_t flags;                    /* CM_NDT_* */
} cm_ndt_result;
typedef struct cm_ndt_corr {           /* 16 bytes */
    uint32_t idx;                      /* result index of the voxel holding the point if it was used, else CM_NDT_NONE */
    uint32_t n_used;                   /* voxels used for this point, 0..7 */
    double score;                      /* this point's sum of w */
} cm_ndt_corr;
CM_API int cm_result_ndt_align(cm_ctx* ctx, const cm_ndt_params* p, const void* src_host, uint64_t n_src, cm_ndt_result* out);
/* The same with the source already in device memory, read in place. */
CM_API int cm_result_ndt_align_device(cm_ctx* ctx, const cm_ndt_params* p, const void* src_dev, uint64_t n_src,
                                      cm_ndt_result* out);
/* The correspondences of the last call's final evaluation, entry i for source record i. *n: the entries (written whenever
 * there was such a call); more than capacity: CM_CAPACITY (nothing is copied). No call since the last merge: CM_BAD_ARG. */
CM_API int cm_ndt_correspondences_copy(cm_ctx* ctx, cm_ndt_corr* host_dst, uint64_t capacity, uint64_t* n);

/* ---- host memory helpers (pinned staging for PointCloud2 payloads) --------------------------- */
CM_API int cm_host_alloc(void** ptr, size_t bytes);
CM_API int cm_host_free(void* ptr);
/* Makes memory the caller already owns (a message's payload vector) DMA-able for the asynchronous copies, and undoes it. */
CM_API int cm_host_register(void* ptr, size_t bytes);
CM_API int cm_host_unregister(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDMERGE_H */
