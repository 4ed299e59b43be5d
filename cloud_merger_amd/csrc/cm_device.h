// cm_device.h — structures shared by the host-side C-ABI (cm_api.cpp) and the gfx950 kernels.
#pragma once
#include <stdint.h>

#define CM_DEV_MAX_SENSORS 16

// Tiling of the padded point index space: every sensor starts at a multiple of CM_TILE, so a tile
// never straddles two sensors (wave-uniform transform) and the key kernel can emit the first radix
// histogram per tile.
#define CM_TILE 4096          // points per workgroup in the streaming and radix kernels
#define CM_BLOCK 256          // threads per workgroup (4 wave64)
#define CM_ITEMS 16           // CM_TILE / CM_BLOCK
#define CM_WAVES 4
#define CM_RADIX_BITS 8
#define CM_RADIX 256
#define CM_MAX_PASSES 4
#define CM_INVALID_KEY 0xFFFFFFFFu

#define CM_GROUP 32           // tiles per group total in the radix passes
#define CM_DIRECT_GROUPS 64   // up to this many groups (8 M slots) k_scatter sums the group totals itself

#define CM_SEG_TILE 2048      // sorted items per workgroup in the centroid kernel
#define CM_SEG_ITEMS 8
#define CM_MINMAX_BLOCKS 1024 // workgroups (= partial records) of the min/max pass
#define CM_SEG_GROUP 256      // sorted tiles per kept-voxel group total (== CM_BLOCK)
#define CM_SEG_DIRECT_TILES 4096  // up to this many sorted tiles the per-tile counts are summed directly

// Bucket path (cm_kernels_v2.hip): G global 8-bit passes over 16-byte point records on the HIGH key
// bits, then one workgroup-local finish (LDS sort of the low bits + centroids) per bucket-aligned tile.
#define CM2_BLOCK 512         // threads per workgroup in the record passes (8 wave64, 8 points each)
#define CM2_WAVES 8
#define CM2_ITEMS 8
// (the local finish's geometry — 2048-record tiles, room for 4032 (k3_local) / 4096 (k2_local), 512 threads — is fixed where it is launched)
#define CM2_MAX_LOW_BITS 14   // key bits left to the local finish when the global passes allow it

// Quantile passes (cm_kernels_v4.hip): ONE global pass into up to CM4_BINS buckets cut at the quantiles of the previous
// frame's sorted records (about CM4_TARGET records each), one finish workgroup per bucket (room for CM4_CAP records).
#define CM4_BINS 2048         // bins of the wide pass
#define CM4_MAX_BUCKETS 8192  // buckets of a frame: above CM4_BINS two or four neighbouring buckets share a bin of the pass
                              // (cm_quant_sub_shift below; frames of up to 15 M records)
#define CM4_TARGET 1920u
#define CM4_CAP 4032u          // records a finish workgroup of the usual shape holds (k3_local: 512 threads, four per CU)
#define CM4_CAP_BIG 8064u      // ... and of the large shape (1024 threads, one per CU) that takes the few buckets beyond that
#define CM4_MAX_BIG 64u        // at most this many such buckets per frame (more: the frame is handed back); the large launch has this many workgroups
#define CM4_MAX_AVG 2600u     // the host takes the path only while records / buckets stays below this
#define CM4_MAX_TILES 4096u   // ... and the frame has at most this many 4096-slot tiles (k4_colscan's register tile)
// Buckets the NEXT frame uses when this one sorted n records (the finish writes that many splitters; the host sizes the grids).
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t cm_quant_buckets(uint32_t n) {
    if (n == 0) return 0;
    uint32_t b = (n + CM4_TARGET - 1u) / CM4_TARGET;
    // one pass for as long as CM4_BINS buckets of at most CM4_MAX_AVG records hold the frame (cfg2: 2048 x 1953)
    if (b > CM4_BINS && (n + CM4_BINS - 1u) / CM4_BINS <= CM4_MAX_AVG) b = CM4_BINS;
    return b > CM4_MAX_BUCKETS ? CM4_MAX_BUCKETS : b;
}
// More than CM4_BINS buckets, still one global pass ("shared bins"): the pass scatters by bucket >> shift — 2^shift
// neighbouring buckets share a bin — and the finish workgroup of a bucket picks its records out of its bin by their
// index (k3_local<SUB>: the 2^shift workgroups of a bin run on the same XCD and read it through that XCD's L2).
static inline uint32_t cm_quant_sub_shift(uint32_t n_buckets) {
    return n_buckets <= CM4_BINS ? 0u : n_buckets <= 2u * CM4_BINS ? 1u : 2u;
}

// Point layouts the loaders special-case.
#define CM_LAYOUT_XYZI16 0    // x,y,z,intensity @0,4,8,12, step 16, 16-B aligned: one dwordx4 load
#define CM_LAYOUT_PCL32 1     // pcl::PointXYZI image, step 32, intensity @16: dwordx4 + dword
#define CM_LAYOUT_GENERIC 2   // any step/offsets, possibly unaligned: four dword loads

struct CmSensorDev {
    const unsigned char* data;
    uint32_t n;               // points in the cloud
    uint32_t base;            // first padded global index (multiple of CM_TILE)
    uint32_t point_step;
    uint32_t off_x, off_y, off_z, off_i;   // off_i == 0xFFFFFFFF: no intensity
    uint32_t layout;
    float m[12];              // row-major 3x4 [R|t]
    uint32_t slot;            // the caller's sensor number (slots without a cloud are skipped in s[]): what per-sensor
                              // settings — the ground stage's slab tables — are indexed by
    uint32_t _pad;
};

// One entry per 4096-slot tile of the padded index space, written by k_setup with the frame descriptor: where the
// tile's first point lies and how many points of its cloud are left from there, so that the streaming kernels reach
// their points through ONE dependent load instead of descriptor -> sensor -> payload.
struct CmTileDev {
    const unsigned char* data;   // address of the tile's first point
    uint32_t n_left;             // points of the cloud from there to its end (>= 1)
    uint32_t info;               // index into CmFrameDev::s | layout << 8
};

struct CmFrameDev {
    CmSensorDev s[CM_DEV_MAX_SENSORS];
    uint32_t n_sensors;
    uint32_t n_padded;        // size of the padded index space (multiple of CM_TILE)
    uint32_t n_tiles;         // n_padded / CM_TILE
    uint32_t crop_enable;
    float crop_min[3];
    float crop_max[3];
    float inv_leaf[3];        // 1.0f / leaf, computed once on the host in fp32
    uint32_t min_pts;
    uint32_t downsample_all;
    float inv_cell[3];        // outlier stage: 1 / (1.01 * radius) — candidate grid a little wider than the radius
    float outlier_r2;         // float(double(r) * double(r)): FLANN compares squared distances
    uint32_t outlier_min_nb;
    float ext_min[3];         // grid bounds handed in by the host (fused cloud across GPUs: the
    float ext_max[3];         // min/max of the WHOLE merged cloud, all-reduced over the ranks)
    // Bucket path: the grid of the box the frame is sorted in (crop box or predicted box), set up on the
    // host with the arithmetic of compute_grid (cm_common.hpp): cell of the box minimum, cells per axis.
    int32_t box_min_b[3];
    int32_t box_div_b[3];
    uint32_t box_key_bits;
    uint32_t box_predicted;   // 1: the box is a prediction (check every point against it)
    // ... and of the radius grid of the outlier stage over the crop box (cells 1.01 r wide), same set-up
    int32_t cell_min_b[3];
    int32_t cell_div_b[3];
    uint32_t cell_key_bits;
    uint32_t _pad_cell;
};

// Zone-wise ground removal (cm_kernels_ground.hip): per sensor up to 8 x-slabs, each with a z band.
#define CM_DEV_MAX_ZONES 8
#define CM_GROUND_BATCH 32        // RANSAC hypotheses scored per round (PCL's loop usually stops within the first)
#define CM_GROUND_CHUNK 8192      // band points per workgroup of the least-squares sums (fixed: it defines their order)
#define CM_GROUND_SPARE 24        // hypotheses beyond max_iterations, for collinear samples that are skipped
struct CmGroundDev {
    uint32_t n_zones[CM_DEV_MAX_SENSORS];
    float x0[CM_DEV_MAX_SENSORS][CM_DEV_MAX_ZONES], x1[CM_DEV_MAX_SENSORS][CM_DEV_MAX_ZONES];
    float zmax[CM_DEV_MAX_SENSORS][CM_DEV_MAX_ZONES];      // < 0: keep the slab whole
    float zlo[CM_DEV_MAX_SENSORS][CM_DEV_MAX_ZONES];       // float(double(zmax) + 0.01): where the part above the band starts
    float z_keep_max;
    float threshold;
    float probability;
    uint32_t max_iterations;
    uint32_t optimize;
    uint32_t _pad;
    unsigned long long seed;
};
struct CmGroundPlaneDev {                 // == cm_ground_plane
    float plane[4];
    uint32_t band_points, inliers, iterations;
    int32_t found;
};

// Per-frame device state, zeroed before the first kernel of a frame.
struct CmFrameState {
    uint32_t outside;         // bucket path: a point fell outside the predicted box (frame must be redone)
    uint32_t quant_abort;     // quantile passes (cm_kernels_v4.hip): a bucket beyond the finish's capacity — every later kernel leaves
    uint32_t spl_incomplete;  // the finish could not leave every quantile (a voxel reached beyond what a tile holds in LDS): no splitters
    uint32_t quant_big;       // quantile passes: buckets this frame handed to the large finish shape (k4_colscan's list)
    uint32_t _unused[2];
    uint32_t n_valid_k0;      // valid points counted by the min/max pass
    int32_t status;           // cm_status of the frame (0 OK, 1 EMPTY, 2 OVERFLOW)
    int32_t min_b[3], max_b[3], div_b[3];
    float min_p[3], max_p[3];
    uint32_t key_bits;
    uint32_t n_passes;
    uint32_t n_valid;         // points that entered the sort (after pass 0)
    uint32_t n_out;
    uint32_t n_seg_tiles;
    uint32_t err;
};

// Device status codes mirror cm_status.
#define CM_DEV_OK 0
#define CM_DEV_EMPTY 1
#define CM_DEV_OVERFLOW 2
#define CM_DEV_ERR_UNSORTED 2u   // CmFrameState.err: the radix sort's output was not sorted
#define CM_DEV_ERR_LOOKBACK 3u   // ... a workgroup waited too long for its predecessors' counts
#define CM_DEV_ERR_BUCKET 4u     // ... a bucket did not fit the local finish's LDS capacity
#define CM_DEV_ERR_BUCKET_PRE 5u // ... the same in the outlier stage's sort (a radius cell with thousands of points)
#define CM_DEV_ERR_GRID 6u       // ... the kernels behind pass 0 were launched with fewer workgroups than the kept records need
#define CM_DEV_ERR_QUANT 7u      // ... a quantile bucket (cm_kernels_v4.hip) grew beyond the finish's capacity: the splitters are stale
#define CM_DEV_OUTLIER_GRID 3   // the radius grid of the outlier stage does not fit (rows or 32-bit index)
#define CM_DEV_ABORTED 4        // a stage gave up (CmFrameState.err says why): every later kernel of the frame leaves at once —
                                // what the stage left behind (half-sorted keys, unwritten records) must not be indexed with

#define CM_ROW_TABLE_CAP (1u << 22)   // rows (y,z cell pairs) of the outlier stage's candidate grid

// Ego-motion compensation (cm_kernels_motion.hip): the raw sensor descriptors of the frame plus, per sensor, its time field
// and the offset of its header stamp from the reference instant; the twist. Passed by value to k_motion.
#define CM_MOTION_ITEMS 8         // points per thread of k_motion: CM_BLOCK * 8 = 2048 per workgroup, two to a tile
#define CM_DEV_TIME_NONE 0u       // == CM_TIME_NONE / CM_TIME_F32_S / CM_TIME_U32_NS
#define CM_DEV_TIME_F32_S 1u
#define CM_DEV_TIME_U32_NS 2u
struct CmMotionDev {
    CmSensorDev s[CM_DEV_MAX_SENSORS];
    uint32_t time_off[CM_DEV_MAX_SENSORS];
    uint32_t time_type[CM_DEV_MAX_SENSORS];
    float dt0[CM_DEV_MAX_SENSORS];   // (float)((double)(stamp - t_ref) * 1e-9), seconds
    float v[3], w[3];
    float k[3];                      // w x v, fp32 on the host
    uint32_t n_sensors;
};

// Per-voxel covariance (cm_kernels_cov.hip): the grid the result's keys (out_key) are linear indices in — cm_ctx's cell grid
// and the frame's fp32 1 / leaf — passed by value to k_cov_keys; and one table entry (== cm_voxel_cov, 80 bytes).
struct CmCovGridDev {
    float inv[3];
    int32_t min_b[3];
    uint32_t div_b[3];
};
#define CM_COV_VALID_DEV 1u       // == CM_COV_VALID / CM_COV_INFLATED
#define CM_COV_INFLATED_DEV 2u
struct CmVoxelCovDev {
    float mean[3];
    uint32_t count;
    float cov[6];
    float icov[6];
    float evals[3];
    uint32_t flags;
};

// Statistical outlier removal (cm_kernels_sor.hip): the stage's word array (u64): per-exponent bins of d_i and of
// fp32(d_i * d_i), the count of the second launch's list, then the stats record (== cm_sor_stats).
#define CM_SOR_KMAX 64
#define CM_SOR_WORD_LIST 512
#define CM_SOR_WORD_STATS 514
#define CM_SOR_WORDS 520
struct CmSorStatsDev {
    unsigned long long n_valid, n_removed;
    double mean, stddev, threshold;
};

// Euclidean cluster extraction (cm_kernels_cluster.hip): the search grid of the result's centroids — cell c = floor((p - min)
// * inv) per axis, clamped to [0, dims - 1], key = c0 + dims0 * (c1 + dims1 * c2) — passed by value to k_cl_keys; and one
// table entry (== cm_cluster, 40 bytes; the AABB as order-preserving integer images until k_cl_decode).
struct CmClusterGridDev {
    float min[3];
    float inv;
    uint32_t dims[3];
};
struct CmClusterDev {
    uint32_t first, n_voxels, n_points, _pad;
    uint32_t lo[3], hi[3];
};

// Normals of the result (cm_kernels_normals.hip): the search grid is a CmClusterGridDev; an entry (== cm_voxel_normal, 32
// bytes) is written as two 16-byte words; the flag == CM_NORMAL_VALID.
#define CM_NORMAL_VALID_DEV 1u

// Registration against the result (cm_kernels_align.hip): the search grid is a CmClusterGridDev; a correspondence
// (== cm_align_corr, 8 bytes) is one uint2. The pose and the pivot go to k_aln_eval by value, in fp64. A block's partials:
// CM_ALIGN_TERMS sums (the lower triangle of H row by row, g, sse) and the count as a 64-bit integer, CM_ALIGN_STRIDE
// doubles apart.
#define CM_ALIGN_NONE_DEV 0xFFFFFFFFu
#define CM_ALIGN_TERMS 28
#define CM_ALIGN_SUMS 29
#define CM_ALIGN_STRIDE 32
struct CmAlignPoseDev {
    double m[12];          // row-major 3x4 [R|t]
    double p0[3];          // the pivot
};

// NDT registration against the covariance table (cm_kernels_ndt.hip): the grid is k_cov_keys' CmCovGridDev, the pose a
// CmAlignPoseDev, the block partials k_aln_eval's (the 28th sum is the score); a correspondence (== cm_ndt_corr, 16 bytes:
// idx, n_used, the score's 8 bytes) is one uint4.
#define CM_NDT_NONE_DEV 0xFFFFFFFFu

// Oriented boxes of the clusters (cm_kernels_box.hip): the constants of include/cloudmerge.h the kernels need (cm_api.cpp
// asserts that they agree) and one table entry (== cm_cluster_box, 48 bytes). CM_BOX_SPLIT: a cluster of more members is
// not walked by one workgroup but chunk by chunk across workgroups (DESIGN.md §19 says why 1024).
#define CM_BOX_CHUNK_DEV 256
#define CM_BOX_MAX_ANGLES_DEV 180
#define CM_BOX_MAX_EXTENT_DEV 1.0e6f
#define CM_BOX_CLOSENESS_DEV 1u
#define CM_BOX_VALID_DEV 1u
#define CM_BOX_SPLIT 1024u
struct CmBoxDev {
    float center[3], size[3], yaw;
    uint32_t angle;
    double score;
    uint32_t flags, _pad;
};

// 2-D grid map of the frame (cm_kernels_grid.hip): what the kernels take of cm_grid_params (inv = 1.0f / cell, formed on the
// host) and the states of include/cloudmerge.h (cm_api.cpp asserts that they agree). A cell's record is 8 words, kept as
// images whose zero means "nothing yet" until k_grid_finish: n, n_ground, ~ord(z_lo), ord(z_hi), ~ord(g_lo), ord(g_hi),
// ord(i_max), 0 — ord the order-preserving image of a float, never 0 and never 0xFFFFFFFF for a number that is not NaN, so
// that every field grows by an add or a max from a table cleared to zero bytes.
#define CM_GRID_UNKNOWN_DEV 0u
#define CM_GRID_FREE_DEV 1u
#define CM_GRID_OCCUPIED_DEV 2u
#define CM_GRID_WORDS 8
#define CM_GRID_HASH 1024         // slots of k_grid_bin's LDS table of a tile's distinct cells (a power of two)
#define CM_GRID_PROBES 8          // slots a point tries before it goes to the table in HBM itself
struct CmGridDev {
    float origin[2];
    float inv;
    uint32_t nx, ny;
    float z_min, z_max;
    float obstacle_height;
    uint32_t min_points;
};

// Free-space ray casting over the grid map (cm_kernels_rays.hip): per descriptor sensor the origin cell the host computed
// with the grid's step 1 (has: 0 where the origin is outside the grid or not finite — the sensor casts nothing), the grid's
// width and the range limit (0: none). A ray cell's record is (n_pass, n_end), two words.
#define CM_RAY_RUN 32             // bitmap words (1024 end cells) of one sensor a k_ray_cast workgroup takes
#define CM_RAY_HASH_BITS 12
#define CM_RAY_HASH (1u << CM_RAY_HASH_BITS)   // slots of its LDS table of crossed cells: 32 KiB of (cell, count), four workgroups per CU
#define CM_RAY_PROBES 8           // slots a step tries before it goes to the table in HBM itself
struct CmRayDev {
    int32_t ox[CM_DEV_MAX_SENSORS], oy[CM_DEV_MAX_SENSORS];
    uint32_t has[CM_DEV_MAX_SENSORS];
    uint32_t nx;
    uint32_t max_range;
};

// Rolling log-odds occupancy map (cm_kernels_map.hip). What k_map_mark takes: rows x and y of the pose, inv = 1.0f / cell, the
// window's anchor (the absolute cell of window cell (0, 0)) and size, the height band. What k_map_update takes: the window,
// the shift anchor_new - anchor_old per axis (carry 0: the old window shares no cell with the new one, or there is none), the
// frame's sensors and the eight log-odds parameters. A state record is (logodds, n_obs), two words.
struct CmMapDev {
    float p[8];
    float inv;
    int32_t ax, ay;
    uint32_t nx, ny;
    float z_min, z_max;
};
struct CmMapUpdateDev {
    uint32_t nx, ny;
    int32_t sx, sy;
    uint32_t carry;
    uint32_t n_sensors;
    int32_t l_hit, l_miss, l_min, l_max, l_free, l_occ;
};

// Cost layer over the occupancy map (cm_kernels_cost.hip). The column pass works on blocks of CM_COST_ROWS rows: one bit per
// row says whether the cell is an obstacle, so a block of one column is one 32-bit word. The row pass gives a workgroup of
// CM_COST_BLOCK threads one row, which it walks in strips of CM_COST_BLOCK cells, with the row's squared vertical distances in
// LDS: CM_COST_MAX_AXIS words, the widest window a cost layer takes. CM_COST_FAR stands for "no obstacle in this column" in
// LDS: adding any dx * dx of a window to it neither overflows nor comes below it.
#define CM_COST_ROWS 32
#define CM_COST_BLOCK 256
#define CM_COST_MAX_AXIS_DEV 2048
#define CM_COST_FAR 0xF0000000u
#define CM_COST_NO_ROW 0xFFFFu
struct CmCostDev {
    uint32_t nx, ny;
    uint32_t r2;                       // R * R: the table has r2 + 1 entries
    uint32_t inflate_unknown;
};

// Plan layer behind the cost layer (cm_kernels_plan.hip). A sweep gives a workgroup of CM_PLAN_BLOCK threads one tile of
// CM_PLAN_TILE x CM_PLAN_TILE cells, one thread per cell, with the tile and one ring of cells around it in LDS. The host
// launches CM_PLAN_BATCH sweeps between two reads of their changed-tile counters, and a thread relaxes its cell CM_PLAN_INNER
// times between two barriers of its workgroup (both measured). k_plan_path's output begins with
// CM_PLAN_PATH_HEAD words (n_cells, status, pot(start), 0); the status values are cm_path_info's, BROKEN is the kernel's own.
#define CM_PLAN_TILE 32
#define CM_PLAN_BLOCK 1024
#define CM_PLAN_BATCH 8
#define CM_PLAN_INNER 4
#define CM_PLAN_PATH_HEAD 4
#define CM_PLAN_PATH_FOUND_DEV 0u
#define CM_PLAN_PATH_UNREACHABLE_DEV 1u
#define CM_PLAN_PATH_TRUNCATED_DEV 2u
#define CM_PLAN_PATH_BROKEN_DEV 0xFFFFFFFFu
struct CmPlanDev {
    uint32_t nx, ny;
    uint32_t tiles_x, tiles_y;
    uint32_t goal;                     // window cell ix + iy * nx
    uint32_t neutral, factor_q8;
    uint32_t allow_unknown;
};

// Rollout layer behind the plan layer (cm_kernels_traj.hip). k_traj_roll gives one wave one trajectory, CM_TRAJ_WAVES of them
// to a workgroup; the wave issues the cost-byte loads of CM_TRAJ_STEP_BATCH poses before it reduces any of them, and reads the
// heading table through the caches (CM_TRAJ_DIRS_LDS 1: every workgroup stages it in LDS first; both batch sizes and both
// table routes were measured). k_traj_best reduces the records in one workgroup of CM_TRAJ_BEST_BLOCK threads
// and writes CM_TRAJ_INFO_WORDS words (best, n_valid). The status values are cm_traj_score's.
#ifndef CM_TRAJ_STEP_BATCH
#define CM_TRAJ_STEP_BATCH 4
#endif
#ifndef CM_TRAJ_DIRS_LDS
#define CM_TRAJ_DIRS_LDS 0
#endif
#define CM_TRAJ_WAVES 4
#define CM_TRAJ_BEST_BLOCK 1024
#define CM_TRAJ_INFO_WORDS 2
#define CM_TRAJ_HEADINGS_DEV 4096
#define CM_TRAJ_MAX_SAMPLES_DEV 16384
#define CM_TRAJ_MAX_STEPS_DEV 256
#define CM_TRAJ_MAX_FOOT_DEV 256
#define CM_TRAJ_VALID_DEV 0u
#define CM_TRAJ_COLLISION_DEV 1u
#define CM_TRAJ_OFF_MAP_DEV 2u
#define CM_TRAJ_NO_POTENTIAL_DEV 3u
struct CmTrajDev {
    float x, y;                        // the start
    float inv;                         // 1.0f / cell
    int32_t ax, ay;                    // the map's anchor
    uint32_t nx, ny;
    uint32_t h0;                       // the start heading, a binary angle
    uint32_t nv, nw;
    uint32_t n_steps, n_foot;
    uint32_t occ_scale, goal_scale;
    uint32_t allow_unknown;
};
struct CmTrajScoreDev {                // cm_traj_score
    uint32_t status, bad_step, occ, pot_end;
    unsigned long long total;
    float end_x, end_y;
};

// Scan matching layer behind the cost layer (cm_kernels_match.hip). k_match_score gives a workgroup of CM_MATCH_BLOCK threads
// one angle candidate and one tile of CM_MATCH_TILE x CM_MATCH_TILE window cells: the tile's field bytes with a halo of
// (wx, wy) cells and the tile's marked cells are staged in LDS, every thread sums the bytes of its translations over the cell
// list and adds the sums into the volume (integer atomicAdd: the order cannot show). k_match_best reduces the volume in one
// workgroup of CM_MATCH_BEST_BLOCK threads and writes CM_MATCH_INFO_WORDS words: best, n_cells, score, then the scores of the
// best entry's neighbours at i - 1, i + 1, j - 1, j + 1 (0 where there is none), one spare.
#define CM_MATCH_TILE 32
#define CM_MATCH_BLOCK 256
#define CM_MATCH_BEST_BLOCK 1024
#define CM_MATCH_INFO_WORDS 8
#define CM_MATCH_MAX_SHIFT_DEV 64
#define CM_MATCH_MAX_ANGLES_DEV 255
struct CmMatchDev {
    float tx, ty;                      // the prior's translation (P3, P7)
    float inv;                         // 1.0f / cell
    int32_t ax, ay;                    // the map's anchor
    uint32_t nx, ny;
    float z_min, z_max;
    uint32_t n_k;                      // 2 * n_a + 1 candidates
    uint32_t n_a;
    uint32_t wx, wy;
    uint32_t words;                    // bitmap words of one candidate
    uint32_t r2;                       // the field table has r2 + 1 entries
};

// Frontier layer behind the plan layer (cm_kernels_front.hip). k_front_local gives a workgroup of CM_FRONT_BLOCK threads one
// tile of CM_FRONT_TILE x CM_FRONT_TILE cells, one thread per cell, with the image bytes of the tile and one ring of cells
// around it in LDS. The cell passes (merge, flatten, count, number, table) run CM_FRONT_BLOCK cells per workgroup, and the
// scan of their counts and k_front_best are one workgroup each. The info words the host reads back: the frontier cells, the
// components, the frontiers, the entries written, best, one spare, then the score's low and high word. A table entry on the
// device is cm_frontier with min_pot and min_pot_cell as one 64-bit key (pot << 32 | cell: an atomicMin keeps the smallest
// pot and the lowest cell that has it) and the box in a scratch table of four words per entry, since there is no 16-bit
// atomic; k_front_best puts both into cm_frontier's form.
#define CM_FRONT_TILE 32
#define CM_FRONT_BLOCK 1024
#define CM_FRONT_INFO_WORDS 8
#define CM_FRONT_SLOTS 32              // per workgroup of k_front_flatten and k_front_table: keys whose waves combine in LDS first
#define CM_FRONT_NONE_DEV 0xFFFFFFFFu
#define CM_FRONT_MAX_TABLE_DEV 65536u
struct CmFrontDev {
    uint32_t nx, ny;
    uint32_t tiles_x, tiles_y;
    uint32_t n_blocks;                 // (nx * ny + CM_FRONT_BLOCK - 1) / CM_FRONT_BLOCK
    uint32_t min_cells, max_frontiers, max_cost;
    uint32_t pot_scale, gain_scale;
};
struct CmFrontEntryDev {               // cm_frontier
    uint32_t first_cell, n_cells;
    unsigned long long sum_x, sum_y;
    unsigned long long key;            // until k_front_best: pot << 32 | cell; then min_pot (low word) and min_pot_cell
    uint32_t box01, box23;             // x0 | y0 << 16, x1 | y1 << 16 (written by k_front_best)
};

// Search layer behind the cost layer (cm_kernels_msearch.hip): branch-and-bound scan matching over wide windows. A node is one
// word, (k + n_a) << 24 | (j0 + wy) << 12 | (i0 + wx); a cell of a candidate's list is x | y << 16. k_msearch_score gives a
// workgroup of CM_MSEARCH_BLOCK threads one node; k_msearch_pick and k_msearch_best are one workgroup of CM_MSEARCH_ONE_BLOCK
// threads. The layer's CM_MSEARCH_WORDS info words on the device: the bound B, the nodes scored for it, the best leaf with
// its score and cell count, the live leaves, the length of the tiny list of the descent, the score of the prior's leaf, the
// four neighbours of step 7 and their scores, per level h the live nodes and their children at CM_MSEARCH_W_LEVEL + 2 h, the
// tiny list and its scores, the prior's leaf, and three list lengths the host writes (1, 4, the number of roots).
#define CM_MSEARCH_BLOCK 256
#define CM_MSEARCH_ONE_BLOCK 1024
#define CM_MSEARCH_MAX_SHIFT_DEV 1024
#define CM_MSEARCH_MAX_DEPTH_DEV 7
#define CM_MSEARCH_W_B 0
#define CM_MSEARCH_W_PROBE 1
#define CM_MSEARCH_W_BEST 2
#define CM_MSEARCH_W_SCORE 3
#define CM_MSEARCH_W_NCELLS 4
#define CM_MSEARCH_W_LIVE0 5
#define CM_MSEARCH_W_TN 6
#define CM_MSEARCH_W_PRIOR_U 7
#define CM_MSEARCH_W_NEIGH 8
#define CM_MSEARCH_W_NEIGH_U 12
#define CM_MSEARCH_W_LEVEL 16
#define CM_MSEARCH_W_TINY 32
#define CM_MSEARCH_W_TINY_U 36
#define CM_MSEARCH_W_PRIOR 40
#define CM_MSEARCH_W_ONE 41
#define CM_MSEARCH_W_FOUR 42
#define CM_MSEARCH_W_NROOTS 43
#define CM_MSEARCH_WORDS 48
struct CmMSearchDev {
    uint32_t nx, ny;
    uint32_t n_k;                      // 2 * n_a + 1 candidates
    uint32_t n_a;
    uint32_t wx, wy;
    uint32_t max_cells;                // room of one candidate's cell list
};

// Localisation layer behind the cost layer (cm_kernels_mcl.hip): a particle filter against the matching layer's likelihood
// field. k_mcl_score gives one wave one particle at a time, CM_MCL_WAVES waves to a workgroup, the grid sized to the device
// with a stride over the particles; the beams are staged once per workgroup in LDS as float2, and a lane issues the field
// loads of CM_MCL_BEAM_BATCH beams before it adds any. The cell passes and the particle passes run CM_MCL_BLOCK threads per
// workgroup, the scans of block counts, the best particle and the prefix sum of the weights are one workgroup of
// CM_MCL_ONE_BLOCK threads. The layer's CM_MCL_WORDS 64-bit info words on the device, zero before an update: the distinct
// body cells, the stride and the beams of the ordered compaction (the free cells of cm_map_mcl_init_uniform land in the same
// three), the largest acc, the best particle with its x, y (bit patterns) and h, the nine sums of step 9 and the resampling
// decision.
#ifndef CM_MCL_BEAM_BATCH
#define CM_MCL_BEAM_BATCH 4
#endif
#define CM_MCL_WAVES 4
#define CM_MCL_BLOCK 256
#define CM_MCL_ONE_BLOCK 1024
#define CM_MCL_MAX_PARTICLES_DEV 65536u
#define CM_MCL_MAX_BEAMS_DEV 8192u
#define CM_MCL_MAX_RANGE_DEV 1024u
#define CM_MCL_W_NCELLS 0
#define CM_MCL_W_STRIDE 1
#define CM_MCL_W_NBEAMS 2
#define CM_MCL_W_AMAX 3
#define CM_MCL_W_BEST 4
#define CM_MCL_W_BEST_X 5
#define CM_MCL_W_BEST_Y 6
#define CM_MCL_W_BEST_H 7
#define CM_MCL_W_SW 8
#define CM_MCL_W_SW2 9
#define CM_MCL_W_SWQX 10
#define CM_MCL_W_SWQY 11
#define CM_MCL_W_SWC 12
#define CM_MCL_W_SWS 13
#define CM_MCL_W_SWDXX 14
#define CM_MCL_W_SWDYY 15
#define CM_MCL_W_SWDXY 16
#define CM_MCL_W_RESAMPLED 17
#define CM_MCL_WORDS 24
struct CmMclDev {
    float inv, cell;                   // 1.0f / cell, and the map's cell
    int32_t ax, ay;                    // the map's anchor
    uint32_t nx, ny;
    float z_min, z_max;
    uint32_t n;                        // particles
    uint32_t max_beams;
    uint32_t range;                    // range_cells: the body bitmap is side x side bits, side = 2 * range + 1
    uint32_t side;
};
struct CmMclParticleDev {              // cm_mcl_particle
    float x, y;
    uint32_t h, parent;
    unsigned long long acc;
};
struct CmMclWeightDev {                // cm_mcl_weight
    uint32_t score, weight;
};
// The beam model of the localisation layer (k_mcl_beam): a lane keeps CM_MCL_BEAM_WALKS rays in flight (1 and 4
// are compiled too and chosen by the environment's CM_MCL_BEAM_WALKS, a measurement's switch: the same bytes at every value);
// the CM_MCL_BEAM_COUNTS 64-bit outcome counts on the device, zero before an update, in cm_mcl_beam_info's order.
#define CM_MCL_BEAM_WALKS 2
#define CM_MCL_BEAM_COUNTS 6
#define CM_MCL_BEAM_MAX_OVER_DEV 64u
struct CmMclBeamDev {
    uint32_t over;                     // over_cells
    uint32_t plain;                    // CM_MCL_BEAM_PLAIN
    uint32_t walks;                    // rays a lane keeps in flight: 1, 2 or 4
};
// What one init or predict call adds to a particle: the centre (init) or the motion (predict), the three noise scales sc and
// the base of the call's draws.
struct CmMclMoveDev {
    float a, b;                        // x0, y0 or d_fwd, d_left
    double yaw;                        // yaw0 or d_yaw, widened
    float sc_a, sc_b, sc_yaw;
    unsigned long long base;
};
// The hypotheses and the recovery of the localisation layer (k_mcl_hyp_*). The bins of the particles live in an
// open-addressing table of `cap` 64-bit keys (a power of two >= 4 n_particles, CM_MCL_HYP_EMPTY where free), with one parent
// word and one component word per slot; a component's record is CmMclHypRecDev, n_particles of them at most. The mode's
// CM_MCL_HYP_WORDS 64-bit words on the device: the first three are those of the ordered compaction of the free cells (where
// cmk_mcl_compact and k_mcl_init_uniform expect them), then the counts, sum_s and the four doubles of the recovery as bit
// patterns, all zero before an update; the last two are the slow and the fast average, which live from update to update.
#define CM_MCL_HYP_MAX_DEV 64u
#define CM_MCL_HYP_EMPTY 0xFFFFFFFFFFFFFFFFull
#define CM_MCL_HW_NFREE 0
#define CM_MCL_HW_NBINS 3
#define CM_MCL_HW_NCOMP 4
#define CM_MCL_HW_NHYP 5
#define CM_MCL_HW_SUMS 6
#define CM_MCL_HW_WAVG 7
#define CM_MCL_HW_WSLOW 8
#define CM_MCL_HW_WFAST 9
#define CM_MCL_HW_PINJECT 10
#define CM_MCL_HW_NINJECT 11
#define CM_MCL_HW_CLEARED 12           // words [0, 12) are zero before an update
#define CM_MCL_HW_STATE_SLOW 12
#define CM_MCL_HW_STATE_FAST 13
#define CM_MCL_HYP_WORDS 16
struct CmMclHypRecDev {                // the integer part of cm_mcl_hyp
    unsigned long long label;
    unsigned long long n;
    unsigned long long sum_w, sum_wqx, sum_wqy, sum_wc, sum_ws;
    unsigned long long top;            // W << 32 | ~p of the heaviest particle
    unsigned long long sum_wdxx, sum_wdyy, sum_wdxy;
};
struct CmMclHypDev {
    uint32_t on;                       // 0: the mode is off, nothing below is read
    uint32_t n;                        // particles
    uint32_t cap_bits;                 // the table has 1 << cap_bits slots
    uint32_t bin_q, heading_bits, max_hyp, inject_max;
    uint32_t agg;                      // lanes of a wave that share a component combine before the atomics (0: a measurement's switch)
    double a_slow, a_fast;
    unsigned long long* keys;          // cap keys
    uint32_t* parent;                  // cap parent words
    uint32_t* comp;                    // cap component numbers
    uint32_t* slot;                    // n: the slot of every particle
    CmMclHypRecDev* rec;               // n records
    CmMclHypRecDev* out;               // CM_MCL_HYP_MAX_DEV records: the chosen ones in order
    unsigned long long* words;         // CM_MCL_HYP_WORDS
    const uint32_t* free_list;         // the free cells of the map's image in entry order (inject_max > 0)
};

// Cast layer behind the cost layer (cm_kernels_cast.hip): expected ranges from many poses in the map. k_cast_rays gives one
// lane one ray, CM_CAST_BLOCK threads per workgroup, the grid sized to the device with a stride over the rays, so that a wave
// holds consecutive bearings of one pose; the direction table (CM_CAST_DIRS pairs of int16_t, 16 KiB) is staged in LDS.
// k_cast_steps writes the skip table, one byte per window cell: 0 on an occupied cell, otherwise the number of steps a ray
// may take from there, capped at CM_CAST_STEP_CAP. The layer's four count words on the device are indexed by status.
#define CM_CAST_BLOCK 256
#define CM_CAST_DIRS 4096
#define CM_CAST_STEP_CAP 255u
#define CM_CAST_MAX_POSES_DEV 65536u
#define CM_CAST_MAX_BEARINGS_DEV 4096u
#define CM_CAST_MAX_RANGE_DEV 1024u
#define CM_CAST_MAX_RAYS_DEV (1u << 24)
#define CM_CAST_WORDS 4
struct CmCastDev {
    float inv;                         // 1.0f / cell
    int32_t ax, ay;                    // the map's anchor
    uint32_t nx, ny;
    uint32_t n_poses, n_bearings;
    uint32_t pose_words;               // 32-bit words from one pose to the next: 3 (cm_cast_pose) or 6 (cm_mcl_particle)
    uint32_t plain;                    // CM_CAST_PLAIN
};
struct CmCastRayDev {                  // cm_cast_ray
    uint16_t k;
    uint8_t status, pad;
    int16_t jx, jy;
};
