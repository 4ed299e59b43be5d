// cm_route.hpp — route policy of a frame: which launch sequence it runs, the sizes it takes from the frame before it, and
// the adaptive counters a hand-back moves. Host arithmetic only (no HIP): tests/test_route_policy.py builds it on the CPU.
#pragma once
#include <stdint.h>

#include "../../include/cloudmerge.h"
#include "cm_device.h"

// Host copy of the kernels' grid guard for a box (the crop box, or bounds handed in): true when the box itself fits PCL's
// int32 index, in which case the data min/max pass can be skipped (box-relative indices give the same occupancy and the same
// order). Also returns the key width.
bool box_grid(const float bmin[3], const float bmax[3], const float inv[3], uint32_t* key_bits,
              int32_t* min_b = nullptr, int32_t* div_b = nullptr);

// Bits of a linear index over `cells` cells (1 ... 32).
uint32_t key_width(unsigned long long cells);

// Global passes for keys of kb bits over about `est` points: enough that at most CM2_MAX_LOW_BITS index bits are
// left to the local finish, and enough that an average bucket (points / 2^(8 g)) stays well inside its LDS
// capacity. 0: the bucket kernels do not fit this grid.
uint32_t bucket_passes(uint32_t kb, uint64_t est, uint32_t extra);

// Statistical outlier removal: the edge of the search grid's cells. requested > 0 is taken as it is; 0: the last
// frame's mean distance (last_mean, NaN or <= 0: none) clamped to [0.05, 5] m, 0.5 m without one.
float sor_cell(float requested, double last_mean);
// The cell doubled until the grid over [bmin, bmax] fits: 32-bit keys, at most row_cap (y,z) rows, fewer than 2^24 cells per
// axis (the bucket kernels' multiplier). Returns the cell and its grid's key width. The result never depends on the cell.
// 0: no finite cell fits (an extent beyond FLT_MAX on some axis); *key_bits is then left unwritten.
float sor_fit_cell(float cell, const float bmin[3], const float bmax[3], uint32_t row_cap, uint32_t* key_bits);
// Euclidean cluster extraction (cm_result_clusters): the search grid over the bounds [mn, mx] of the result's centroids. A
// centroid's cell is floor((p - mn) * inv) per axis, in fp32. The cell starts a little above the tolerance (1 + 2^-8: with
// at most CM_CLUSTER_AXIS_CAP cells per axis the fp32 rounding of that expression moves a centroid by less than 2^-10 of a
// cell, so two centroids the fp32 predicate joins never lie two cells apart) and doubles until the grid fits: at most
// CM_CLUSTER_AXIS_CAP cells per axis, at most row_cap (y,z) rows, keys below 0xFFFFFFFF. An extent that overflows fp32 on
// some axis (or a cell that does) is searched as one cell: cell +inf, inverse 0. The partition never depends on the cell.
#define CM_CLUSTER_AXIS_CAP 4096u
struct ClusterGrid {
    float cell, inv;
    uint32_t dims[3];
    uint32_t key_bits;
    uint32_t doublings;
};
ClusterGrid cluster_grid(float tolerance, const float mn[3], const float mx[3], uint32_t row_cap);
// Normals of the result (cm_result_normals): the same kind of grid for the k-nearest-neighbour search. The cell starts at
// search_cell, or for 0 at max(leaf) * cbrt(k): the result holds at most one centroid per voxel, so such a cell holds at most
// about k of them and the 27 cells around a centroid on a surface (about 9 k^(2/3) voxels of it) usually hold its k nearest.
// It doubles until the grid fits, exactly as cluster_grid's does, and an extent that overflows fp32 is one cell. The search is
// exact for every cell: the cell sets the cost of the call, never its result.
ClusterGrid normals_grid(float search_cell, const float leaf[3], uint32_t k, const float mn[3], const float mx[3], uint32_t row_cap);
// The search grid of a frame (cm_launch.cpp enqueue). sor_crop_grid: over the crop box when one is on and some finite cell
// fits it (half the row table): returns 1 (the stage's grid mode) with that cell in *cell and its key width; else 0 with
// *cell unchanged, and the grid is over the cloud's own bounds. sor_bounds_cell: the cell over the measured bounds [mn, mx],
// widened by the cell on every side (a quarter of the row table); +inf — one cell, inverse 0 — when the cloud's extent
// overflows fp32 and no finite cell fits.
int sor_crop_grid(const cm_params& p, float* cell, uint32_t* key_bits);
float sor_bounds_cell(float cell, const float mn[3], const float mx[3], uint32_t* key_bits);

// What the frame in flight runs. Set by RouteState::plan at enqueue, rewritten for a replay inside cm_wait; the launch
// functions read it and decide nothing. Fields marked (prev) are sized from the frame before this one (DESIGN.md names the
// device check that catches each of them being wrong).
struct FramePlan {
    // the call
    cm_params params;
    int mode = 0;                  // 0 centroids, 1 partial table
    int grid_mode = 0;             // general path: 0 data min/max (k_minmax), 1 crop box, 2 bounds handed in
    uint32_t key_bits = 0;         // ... with a box: its key width
    bool outl = false;             // radius outlier removal (cm_params.outlier_enable)
    bool sor = false;              // statistical outlier removal (cm_set_statistical_outlier); shares the outlier stage's grid
    cm_sor_params sor_p = {};      // ... its parameters as the frame was enqueued (a redo inside cm_wait reads these)
    bool pre = false;              // pre-stages (ground / outlier removal) leave a keep-mask for the voxel stage
    int gm_o = 0;                  // grid of the outlier stage: 0 data min/max, 1 crop box
    uint32_t kb_o = 0;             // ... its key width
    uint32_t g_o = 0;              // outlier stage on the bucket kernels: its global passes (0: general sort)
    bool pack_o = false;           // ... pass 0 packs the survivors' records (prev)
    // the voxel stage
    bool bucket = false;           // bucket path (else general path)
    bool post_bucket = false;      // ... behind the pre-stages, which run on the general kernels first
    bool quant = false;            // ... quantile passes (cm_kernels_v4.hip)
    bool measured = false;         // ... redone in the box the hand-back measured
    bool redone = false;           // cm_wait launched the frame a second time (CM_PATH_REDONE)
    int b_grid_mode = 0;           // the bucket launch's box: 1 crop box, 2 predicted box or bounds handed in
    bool predicted = false;        // ... the box predicted from the last frame's bounds (checked on the device: `outside`)
    uint32_t g = 0, low = 0;       // ... its global passes (prev: sized for the last frame's points) and the key bits left
    uint32_t nb = 0, sub = 0;      // quantile buckets and shared-bin shift (prev: the last frame's splitters)
    uint32_t n_tile_state = 0;     // words k4_hist clears of tile_info + group totals (prev: nb)
    bool big_armed = false;        // the large finish shape is launched
    bool pack = false;             // k2_hist0 packs the crop survivors' records (prev)
    bool sparse = false;           // ... and the first scatter takes them eight tiles per workgroup (prev)
    uint32_t nt_later = 0;         // tiles of the grids behind pass 0 (prev)
    bool k3 = false;               // finish by k3_local + k3_compact (else k2_local)

    bool writes_splitters() const { return bucket && (quant || (k3 && mode == 0)); }
};

enum class Replay { none, fixed_grid, measured_box, general };

// A box and whether it holds.
struct Box {
    bool ok = false;
    float min[3] = {0, 0, 0}, max[3] = {0, 0, 0};
};

// The adaptive policy of one context: switches read at cm_create, what the last frames left (predicted box, splitters,
// size) and how long each route rests after a hand-back.
struct RouteState {
    // switches (cm_create)
    bool classic_only = false;     // CM_PATH=classic: the general path only
    bool finish_v2 = false;        // CM_FINISH=v2: k2_local with its look-back instead of k3_local + k3_compact
    bool quant_never = false;      // CM_QUANT=0: fixed-grid passes only
    bool quant_sub = true;         // CM_QUANT_SUB=0: frames above 2048 buckets take the fixed-grid passes
    bool verbose = false;          // CM_VERBOSE: say so on stderr when a quantile frame is handed back
    bool lds_rank = false;         // lane-ordered LDS adds (probe at cm_create, CM_LDS_RANK); cleared by a mis-ranked pass
    int debug_misrank = 0;         // test build + CM_DEBUG_MISRANK=1: the last global pass swaps two records of tile 0 (once)

    // what the last frames left
    Box pred;                      // the last frame's bounds plus a margin
    uint64_t last_n_merged = 0;    // points that entered the voxel grid in the last finished frame (0: none yet)
    int spl_cur = 0;               // splitters: a frame reads spl[spl_cur]; its finish writes spl[spl_cur ^ 1]
    bool spl_valid = false;        // spl[spl_cur] holds the quantiles of the last finished frame
    uint32_t spl_n = 0;            // ... which sorted this many records
    int32_t spl_min_b[3] = {0, 0, 0}, spl_div_b[3] = {0, 0, 0};   // ... as indices of this grid
    float spl_inv_leaf[3] = {0, 0, 0};

    // rests and back-offs
    uint32_t v2_extra_passes = 0;  // buckets overflowed LDS: sort more bits globally
    uint32_t v2_good_frames = 0;   // frames since the last overflow (on whichever path they ran)
    uint32_t v2_retry_after = 256; // ... after this many, try one global pass fewer again (doubles on failure)
    uint32_t v2_off_frames = 0;    // ... or give the path a rest
    uint32_t pre_bucket_off = 0;   // frames for which the outlier stage sorts with the general kernels (a bucket overflowed)
    uint32_t pre_bucket_backoff = 16;
    uint32_t grid_shrink_off = 0;  // frames for which the kernels behind pass 0 get whole grids again (after CM_DEV_ERR_GRID)
    uint32_t quant_big_arm = 0;    // quantile frames for which the large finish shape is still launched
    uint32_t quant_off_frames = 0; // frames for which the fixed-grid passes run although splitters are at hand
    uint32_t quant_hist = 0;       // the last eight attempts, newest in bit 0: 1 = handed back
    uint32_t quant_rest = 8;       // how long the next rest is (doubles while rests keep being needed, back to 8 after 16 good)
    uint32_t quant_good = 0;       // good attempts in a row

    // The bucket path applies and does not rest, but has no box yet: the caller measures the cloud's bounds
    // (set_predicted_box) before plan().
    bool needs_box(const FramePlan& pl) const;
    // The route of a new frame. pl holds the call (params ... kb_o); f is its descriptor, which gets the box.
    // spl_ok: the last frame left splitters. cap_padded: the context's padded capacity.
    void plan(FramePlan& pl, CmFrameDev& f, const float* bounds, const float inv_cell[3], bool spl_ok, uint64_t n_in,
              uint32_t cap_padded);
    // The sizes of a fixed-grid bucket launch (pl.b_grid_mode, g, low set): packing, the later passes' grids, the finish.
    void size_fixed_grid(FramePlan& pl, const CmFrameDev& f, uint64_t n_in);
    // The bookkeeping of a finished attempt (h: its host record; UNSORTED clears h.err) and what to replay.
    Replay settle(const FramePlan& pl, CmFrameState& h);
    // A box miss: the frame in a box around the bounds it measured, on the bucket path again. false: refused (pred as it
    // was, except a box that does not fit the index: pred.ok cleared), the frame goes to the general path. f: a copy of
    // the descriptor, given the box.
    bool measured_box(FramePlan& pl, CmFrameDev& f, const CmFrameState& h, uint64_t n_in);
    // A frame that finished: its bounds move the predicted box, its size sizes the next frame, its splitters serve it.
    void adopt(const FramePlan& pl, const CmFrameState& h, const CmFrameDev& f, bool masked);

    void set_predicted_box(const float mn[3], const float mx[3], const float leaf[3]);
    void update_predicted_box(const float mn[3], const float mx[3], const float leaf[3]);

  private:
    bool bucket_applies(const FramePlan& pl) const;
    bool pack_survivors(const CmFrameDev& f, uint64_t n_in) const;
};
