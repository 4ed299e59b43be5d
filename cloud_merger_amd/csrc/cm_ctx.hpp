// cm_ctx.hpp — the context behind the C-ABI handle, shared by the host translation units (cm_api.cpp: entry points and
// their argument checks; cm_launch.cpp: frame assembly and the frame's launch sequences; cm_byproducts.cpp: the tables computed
// from a result on request; cm_route.cpp: the route policy).
//
// Owns the HBM layout and the launch sequence; no arithmetic on points happens on the host. There is no
// CPU fallback of any kind: without a gfx950 device cm_create fails.
//
// HBM layout per context (N = padded point capacity, multiples of CM_TILE per sensor):
//   sensor slots      raw PointCloud2 payloads as submitted (or caller-owned device pointers)
//   keys_a/b, vals_a/b  4 x N x u32   radix ping-pong: voxel index, padded point index
//   hist              (N/4096) x 256 u32   digit counts per tile (one coalesced row each)
//   grp               5 x (N/4096/32) x 256 u32   digit counts per group of 32 tiles, per pass
//   seg_tile_counts   N/2048 u32      kept voxels per sorted tile (+ totals per 256 tiles)
//   out               N x 16 B        centroids x,y,z,intensity (ascending voxel index = PCL order)
//   out_key/out_cnt   N x u32 each    only with CM_FLAG_OCCUPANCY
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/cloudmerge.h"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_route.hpp"

// A cloud as a frame sees it: where its payload lies in HBM and how its points are laid out.
struct SlotCloud {
    const void* dptr = nullptr;      // an owned buffer of the slot or a caller-owned device pointer
    uint32_t n = 0, step = 0, ox = 0, oy = 0, oz = 0, oi = 0;
};

// One sensor. Two owned HBM buffers: the frame that was enqueued last reads `active` (and so do its by-products:
// cm_merged_copy, cm_ground_copy, the overflow fallback, a hand-back's redo) until the NEXT frame is enqueued;
// a submit meanwhile always goes to the other buffer and becomes `staged`. Nothing a subscriber thread does can
// therefore touch what a frame in flight — or its by-products afterwards — read, and cm_submit_cloud never waits for a
// merge (the reference's callbacks run beside its 10 Hz loop: pc_preprocessing_main.cpp:513, :318-337, :549-584).
struct Slot {
    std::mutex mu;
    void* buf[2] = {nullptr, nullptr};   // owned HBM buffers (host submits)
    size_t cap[2] = {0, 0};
    int active_buf = -1;                 // which of them `active` lives in (-1: none / a caller-owned pointer)
    SlotCloud active, staged;
    bool has_data = false;               // `active` (or, while fresh, `staged`) holds a cloud
    bool fresh = false;                  // `staged` holds a cloud no frame has consumed yet
    bool copy_pending = false;           // its H2D copy was enqueued without waiting (cm_submit_cloud_async): ev_copy tells
    float m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy = nullptr;
    uint64_t bytes_h2d = 0;              // payload bytes of the staged cloud that crossed PCIe (0: device submit)
    uint64_t active_bytes_h2d = 0;
    uint64_t gen = 0, active_gen = 0;    // accepted submits so far; the one `active` came from
    uint32_t time_off = 0, time_type = CM_TIME_NONE;   // per-point time field (cm_set_sensor_time_field)
};

struct cm_ctx;

// Buffers of an LSD radix sort of (key, value) pairs over nt tiles: ping-pong a -> b -> a ...; pass 0 reads the group totals
// in grp0 (filled by the launch that made the keys), pass p > 0 those at grp_rest + (p - 1) * gw.
struct SortPairs {
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b, *hist, *totals, *grp0, *grp_rest;
};

// The HBM of one by-product's radix sort, grown with what it sorts (cm_byproducts.cpp).
struct PairSort {
    uint32_t cap_slots = 0;              // words of each keys / vals buffer (a multiple of CM_TILE)
    uint32_t *keys_a = nullptr, *keys_b = nullptr, *vals_a = nullptr, *vals_b = nullptr;
    uint32_t *hist = nullptr, *grp = nullptr;    // (cap_slots / CM_TILE) rows; CM_MAX_PASSES x groups rows
    uint32_t* totals = nullptr;          // CM_RADIX digit totals (k_gscan)
    // Room for n_slots pairs: beyond cap_slots everything is freed and allocated anew (`what`: the error text of a failure).
    int reserve(cm_ctx* c, uint32_t n_slots, const char* what);
    void release();
    // gw: words of one pass's group totals in the sort at hand.
    SortPairs pairs(uint32_t gw) const { return {keys_a, keys_b, vals_a, vals_b, hist, totals, grp, grp + gw}; }
};

// A result's centroids in the order of a search grid over their own bounds (k_cl_bounds, k_cl_keys, the radix passes,
// k_cl_gather, cmk_sorted_rows): what the cluster extraction, the normals and the registration search in. The sorted keys lie
// in sort.keys_a / keys_b (state says which), the grid is the caller's choice (cm_byproducts.cpp build_search_index).
struct SearchIndex {
    PairSort sort;
    CmFrameState* state = nullptr;       // the sort's state record (the cluster call keeps a second one behind it)
    uint32_t* bounds = nullptr;          // six order-images: min x, y, z, max x, y, z of the centroids
    void* pts = nullptr;                 // the centroids in search-grid order (x, y, z, result index)
    uint32_t* aux = nullptr;             // room for 3 x sort.cap_slots words: the three arrays k_cl_gather initialises for the
                                         // cluster call, laid out at the n_slots of the build at hand (aux, aux + n_slots,
                                         // aux + 2 n_slots), not at cap_slots
    void* rows = nullptr;                // (y,z)-row ranges of the search grid
    uint64_t cap_rows = 0;
    CmClusterGridDev grid{};             // the grid of the last build, as the search kernels take it
    void release();
};

// The state of a registration's Gauss-Newton loop (cm_byproducts.cpp fit_pose): align's and ndt's.
struct PoseFit {
    uint64_t cap_src = 0;                // source records corr and part are sized for
    void* corr = nullptr;                // one correspondence per source record: the last evaluation's
    double* part = nullptr;              // CM_ALIGN_STRIDE doubles per block of 256 source records
    double* sums = nullptr;              // CM_ALIGN_SUMS doubles: what the host reads back per evaluation
    void* src = nullptr;                 // the device copy of a host source (cap_src_host records of 16 bytes)
    uint64_t cap_src_host = 0;
    bool have = false;                   // corr holds the table of a call since the last merge, n_src entries
    uint64_t n_src = 0;
    // Room for n_src records of corr_bytes each (what_state, what_table: the error texts of a failure).
    int reserve(cm_ctx* c, uint64_t n_src, size_t corr_bytes, const char* what_state, const char* what_table);
    void release();
};

struct cm_ctx {
    int device = 0;
    uint32_t flags = 0, max_sensors = 0;
    uint64_t max_points = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    Slot slots[CM_MAX_SENSORS];

    uint32_t cap_padded = 0, cap_tiles = 0, cap_seg_tiles = 0;
    uint32_t *keys_a = nullptr, *keys_b = nullptr, *vals_a = nullptr, *vals_b = nullptr;
    uint32_t *hist = nullptr, *grp = nullptr, *totals = nullptr, *seg_counts = nullptr, *seg_tile_counts = nullptr, *seg_groups = nullptr;
    uint32_t cap_groups = 0, frame_seq = 0;
    void* stage32 = nullptr;             // k3_local's staging for partial tables (32-byte entries)
    void* out32 = nullptr;               // the result as pcl::PointXYZI images (cm_result_copy with point_step_out 32)
    float* partials = nullptr;
    uint32_t *out_key = nullptr, *out_cnt = nullptr, *merged_total = nullptr;
    void* out = nullptr;
    void* merged = nullptr;
    unsigned char* mask = nullptr;       // outlier stage: keep-mask over the padded point indices
    void* sorted_pts = nullptr;          // outlier stage: points in radius-grid order
    void* rows = nullptr;                // outlier stage: (y,z)-row ranges
    CmFrameState* d_state_o = nullptr;   // outlier stage: its grid and counts
    const unsigned char* frame_mask = nullptr;   // mask of the last frame (nullptr: stage off)
    void* partial = nullptr;             // cm_partial_entry table of the last cm_merge_partial
    void* table_entries = nullptr;       // merged entries inside cm_merge_tables
    int last_mode = 0;                   // what the last result is: 0 centroids, 1 partial table, 2 merged tables
    CmFrameDev* d_frame = nullptr;
    CmTileDev* d_tiles = nullptr;        // per-tile entries of the uploaded descriptor (k_setup)
    CmFrameDev frame_uploaded;
    bool frame_uploaded_valid = false;
    CmFrameState* d_state[2] = {nullptr, nullptr};
    int cur = 0;
    CmFrameState* h_state = nullptr;     // pinned, written by the last kernel of a frame
    uint32_t* h_state_dev = nullptr;     // device view of h_state
    hipEvent_t ev_done = nullptr;

    std::mutex merge_mu;
    bool pending = false;                // an enqueued frame has not been waited for
    bool pending_trivial = false;        // ... and it had no kernels (nothing submitted)
    bool trivial_grid = false;           // ... but, as an empty share of a fused cloud, it has the shared grid
    float trivial_box[6] = {0, 0, 0, 0, 0, 0};
    CmFrameDev frame;                    // descriptor of the last enqueued frame
    FramePlan plan;                      // ... and what it runs
    RouteState route;
    bool from_crop = false;
    uint64_t n_in = 0;
    uint32_t n_sensors_used = 0;
    cm_result result;
    bool have_result = false;

    // zone-wise ground removal (cm_kernels_ground.hip)
    bool ground_on = false;
    CmGroundDev ground;                  // host copy of the slab table
    bool ground_uploaded = false;
    CmGroundDev* d_ground = nullptr;
    CmFrameState* d_state_g = nullptr;   // state of the slab sort
    unsigned char* gmask = nullptr;      // ground points of the last frame (padded index space)
    uint32_t* zone_off = nullptr;
    CmGroundPlaneDev* d_planes = nullptr;
    void* hyp0 = nullptr;                // first round of hypotheses of every slab: planes, validity, inlier counts
    uint32_t *valid0 = nullptr, *counts0 = nullptr;
    double* chunk_sums = nullptr;        // least-squares sums per chunk of band points
    bool frame_had_ground = false;
    float ground_outlier_radius = 0.f;   // > 0: radius filter on every slab's band points that are not ground (:119)
    uint32_t ground_outlier_min_nb = 0;
    unsigned char* bmask = nullptr;      // those points (input of that filter)
    unsigned char* zcode = nullptr;      // slab of every band point

    // bucket path (cm_kernels_v2.hip)
    void *rec_a = nullptr, *rec_b = nullptr;      // 16-byte point records, ping-pong
    unsigned char* dig = nullptr;        // next digit of every record
    unsigned long long* tile_state = nullptr;     // published kept-voxel counts of the local finish
    uint32_t* wave_cnt = nullptr;                 // records k2_hist0 packed per wave (frames whose crop box drops most points)
    float* records = nullptr;            // min/max/count per tile
    int cell_min_b[3] = {0, 0, 0}, cell_div_b[3] = {1, 1, 1};   // grid the cells in out_key are relative to

    // pipelined publish (cm_result_publish_async): the result buffers exist twice, so that the copy-out of frame n runs on
    // its own stream beside the kernels of frame n + 1
    void* out_other = nullptr;           // the result buffer the frame in flight does NOT write
    void* out32_other = nullptr;
    hipStream_t pub_stream = nullptr;
    hipEvent_t ev_pub[2] = {nullptr, nullptr};   // [0]: the last copy-out that read `out`, [1]: ... `out_other`
    bool pub_pending[2] = {false, false};

    // quantile passes (cm_kernels_v4.hip): one global pass into buckets cut at the last frame's quantiles
    uint32_t* spl[2] = {nullptr, nullptr};   // splitters: route.spl_cur says which one the next frame reads
    uint32_t *qcnt = nullptr, *qtot = nullptr, *qbofs = nullptr;  // per-tile bucket counts / prefixes, bucket totals, bucket starts
    uint32_t* qbig = nullptr;                                     // buckets beyond CM4_CAP records: count, then their numbers
    uint16_t* qbid = nullptr;            // the bucket of every padded slot
    uint32_t hist_resident[3] = {0, 0, 0};   // workgroups of k4_hist<11 .. 13> resident at once on this device (0: not asked yet)

    // per-sensor figures of the last enqueued frame (cm_frame_stats)
    uint32_t stats_n_sensors = 0;
    uint32_t stats_sensor[CM_MAX_SENSORS] = {0}, stats_n[CM_MAX_SENSORS] = {0}, stats_fresh[CM_MAX_SENSORS] = {0};
    uint64_t stats_bytes[CM_MAX_SENSORS] = {0}, stats_gen[CM_MAX_SENSORS] = {0};
    uint32_t* d_tile_kept = nullptr;     // per 4096-slot tile: points that passed crop / masks and entered the sort — the first scatter
    uint32_t* h_tile_kept = nullptr;     // writes them straight into pinned host memory (d_tile_kept is its device view)
    uint64_t bytes_d2h = 0;              // result / merged / ground bytes copied to the host since the frame was enqueued

    // ego-motion compensation (cm_kernels_motion.hip): k_motion writes the frame's compensated points here, at their padded
    // indices, and the descriptor points at them; they live as long as the frame's by-products (until the next enqueue)
    bool motion_on = false;
    cm_motion motion;
    void* motion_buf = nullptr;          // cap_padded x 16 B, allocated by the first cm_set_ego_motion
    bool last_motion = false;            // the frame enqueued last was compensated (CM_PATH_MOTION)

    // per-voxel covariance of the result (cm_kernels_cov.hip), on request after a frame: buffers of its own — no frame reads
    // them — allocated by the first request and grown with the frames. (The merged records go to `merged`, which
    // cm_merged_copy fills with the same bytes and which no frame reads either.)
    PairSort cov;                        // (voxel number, record index), cap_slots = the frame's padded points
    uint32_t* cov_tile_counts = nullptr; // cap_tiles words: cmk_merged's per-tile offsets
    uint32_t* cov_words = nullptr;       // [0] merged records, [1] error word of k_cov_reduce
    CmFrameState* cov_state = nullptr;   // the sort's state record
    void* cov_entries = nullptr;         // the table: cm_voxel_cov per voxel
    uint64_t cov_cap_entries = 0;
    bool cov_have = false;               // cov_entries holds the table of the result at rest, computed with these parameters:
    uint32_t cov_min_points = 0;         // what ndt() reuses
    float cov_eig_mult = 0.0f;

    // Euclidean cluster extraction on the result (cm_kernels_cluster.hip), on request after a frame: buffers of its own — no
    // frame reads them — allocated by the first request and grown with the results. It reads `out` (and out_cnt).
    SearchIndex cl;                      // two state records: the sort by cell, the sort by cluster number; its aux words are
                                         // the union-find's parent, size and point count per voxel
    uint32_t cl_cap_tables = 0;          // voxels the four tables below are sized for (a multiple of CM_TILE)
    uint32_t *cl_root = nullptr, *cl_num = nullptr;
    uint32_t* cl_labels = nullptr;       // the label table
    void* cl_tile_sums = nullptr;        // per tile: kept roots and their voxels, then their exclusive prefixes
    uint32_t* cl_words = nullptr;        // [0] clusters, [1] clustered voxels
    void* cl_clusters = nullptr;         // the cluster table: cm_cluster per cluster
    uint64_t cl_cap_clusters = 0;
    const uint32_t* cl_indices = nullptr;   // the member lists of the last call (one of cl.sort.vals_a / vals_b)
    uint64_t cl_n_clusters = 0, cl_n_clustered = 0;

    // Oriented boxes of the clusters (cm_kernels_box.hip), on request after a frame: the cluster call, then the fit. Buffers of
    // its own — no frame reads them — allocated by the first request and grown with the results.
    void* box_entries = nullptr;         // the table: cm_cluster_box per cluster
    uint64_t box_cap_entries = 0;
    uint64_t box_n = 0;                  // its entries: the clusters of the last box call (0 after a cluster call)
    void* box_dirs = nullptr;            // CM_BOX_MAX_ANGLES (cos, sin) pairs: the direction table at box_dirs_n headings
    uint32_t box_dirs_n = 0;
    float box_dirs_host[2 * CM_BOX_MAX_ANGLES];   // what the upload reads
    uint32_t* box_words = nullptr;       // [0] listed (large) clusters, [1] their chunks
    void *box_list = nullptr, *box_ext = nullptr;    // per listed cluster: (cluster, first chunk row); the extremes' images
    uint64_t box_cap_large = 0;
    void* box_work = nullptr;            // per listed chunk: (slot, chunk)
    double* box_sums = nullptr;          // per listed chunk: CM_BOX_MAX_ANGLES sums
    uint64_t box_cap_chunks = 0;
    uint32_t box_split = CM_BOX_SPLIT;   // (CM_BOX_SPLIT in the environment: the measurement of scripts/box_cost.py)

    // 2-D grid map of the frame (cm_kernels_grid.hip), on request after a frame: it reads the frame's clouds in place (d_frame,
    // frame_mask, gmask) and writes a table and an image of its own — no frame reads them — allocated by the first request and
    // grown with the grids asked for.
    void* grid_cells = nullptr;          // the table: cm_grid_cell per cell
    void* grid_image = nullptr;          // the occupancy image: one byte per cell
    uint64_t grid_cap_cells = 0;         // cells both are sized for
    uint64_t grid_n = 0;                 // cells of the last grid call
    bool grid_have = false;              // the two hold the grid of the result at rest (cleared where a merge replaces it)

    // Free-space ray casting over the grid map (cm_kernels_rays.hip), on request after a frame, behind the grid map of the
    // same call: the per-sensor bitmaps of end cells, the table and the cleared image — no frame reads them — allocated by the
    // first request and grown together.
    float frame_origin[CM_MAX_SENSORS][2] = {};   // per descriptor sensor the (x, y) translation of the matrix the last frame
                                                  // was built with (build_frame; under deskew the descriptor's own is the
                                                  // identity). Read by grid_rays and by nothing else.
    uint32_t* ray_bits = nullptr;        // max_sensors bitmaps of ceil(ray_cap_cells / 32) words
    void* ray_cells = nullptr;           // the table: cm_grid_ray_cell per cell
    void* ray_image = nullptr;           // the cleared occupancy image: one byte per cell
    uint64_t ray_cap_cells = 0;          // cells all three are sized for
    uint64_t ray_n = 0;                  // cells of the last ray call
    bool ray_have = false;               // they hold the rays of the result at rest (cleared by a merge and by a grid call)

    // Normals and curvature of the result (cm_kernels_normals.hip), on request after a frame: buffers of its own, as the
    // cluster extraction's — no frame reads them — allocated by the first request and grown with the results. It reads `out`.
    SearchIndex nrm;
    uint32_t nrm_cap_tables = 0;         // voxels the list and the table are sized for (a multiple of CM_TILE)
    void* nrm_list = nullptr;            // 8 B per voxel: the centroids the first search launch could not finish
    uint32_t* nrm_words = nullptr;       // [0] list count, [1] unused
    void* nrm_entries = nullptr;         // the table: cm_voxel_normal per voxel
    uint32_t nrm_n_listed = 0;           // centroids the last call's second launch took
    bool nrm_have = false;               // nrm_entries holds the table of the result at rest, computed with k = nrm_k:
    uint32_t nrm_k = 0;                  // set by normals(), cleared where a merge invalidates the result

    // Registration of a source cloud against the result (cm_kernels_align.hip), on request after a frame: the cluster call's
    // front end on an index of its own — no frame reads it — allocated by the first request and grown with the results and
    // the sources. It reads `out` and nrm_entries.
    SearchIndex aln;
    PoseFit aln_fit;                     // cm_align_corr per source record

    // NDT registration of a source cloud against the covariance table (cm_kernels_ndt.hip), on request after a frame: reads
    // out, out_key and cov_entries; these buffers are the call's own.
    PoseFit ndt_fit;                     // cm_ndt_corr per source record
    uint32_t* ndt_bounds = nullptr;      // six bounds images (k_cl_bounds)

    // statistical outlier removal (cm_kernels_sor.hip): sorts by the outlier stage's grid (sorted_pts, rows, d_state_o) and
    // leaves its keep-mask in `mask`; its own buffers are allocated by the first cm_set_statistical_outlier
    bool sor_on = false;
    cm_sor_params sor;
    float* sor_d = nullptr;              // cap_padded floats: d_i per padded index (0xFFFFFFFF: not in the stage's input)
    void* sor_list = nullptr;            // cap_padded x 8 B: the points the first search launch could not finish, and their bound
    unsigned long long* sor_words = nullptr;   // CM_SOR_WORDS: bins, list count, stats record
    bool last_sor = false;               // the frame enqueued last ran the stage
    cm_sor_stats sor_stats;              // ... its figures, read back by cm_wait
    double sor_last_mean = 0.0;          // mean distance of the last frame that had one (search_cell 0)

    std::vector<hipEvent_t> prof_ev;
    std::vector<std::string> prof_names;
    size_t prof_used = 0;
    cm_stage_times stage_times;

    std::mutex err_mu;
    std::string err;
};

// (subscriber threads and the loop thread may fail at the same time — an oversize cloud beside a refused merge — and a third
// thread may be reading the text: the string is only touched under its own lock, and cm_last_error hands out a copy)
inline int fail(cm_ctx* c, int code, const std::string& what) {
    if (c) { std::lock_guard<std::mutex> lk(c->err_mu); c->err = what; }
    return code;
}

#define HIP_TRY(c, call)                                                                        \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail((c), CM_HIP_ERROR, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// cm_launch.cpp. Every one of them is called with merge_mu held.
// Builds the frame descriptor in c->frame (consume: the frame takes the sensors' fresh clouds; false: a peek).
int build_frame(cm_ctx* c, const cm_params* p, bool consume, std::vector<std::unique_lock<std::mutex>>& locks);
// The frame's points that `mask` keeps (nullptr: every valid one) as 16-byte records in (sensor, point) order into `out`,
// and their number (a host round trip). tile_counts: cap_tiles words.
int fuse_points(cm_ctx* c, uint32_t* tile_counts, void* out, const unsigned char* mask, uint32_t* total);
// k_minmax over the uploaded descriptor and a host round trip: the bounds of the frame's valid points and their count.
int measure_bounds(cm_ctx* c, float mn[3], float mx[3], uint64_t* n_valid);
// mode 0: the path (centroids). mode 1: partial table of per-voxel sums (fused cloud across GPUs); `bounds` (min xyz,
// max xyz of the whole fused cloud) then fixes the grid unless the crop box does.
int enqueue(cm_ctx* c, const cm_params* p, int mode = 0, const float* bounds = nullptr);
int wait_frame(cm_ctx* c, cm_result* res);
int merge_tables(cm_ctx* c, const void* const* dev_tables, const uint64_t* n_entries, uint32_t n_tables, const cm_params* p,
                 cm_result* res);
void prof_mark(cm_ctx* c, const char* name);
// scatter_mark: the prof_mark name of the scatter (the histogram and scan passes get theirs); nullptr: no marks.
void radix_sort_pairs(cm_ctx* c, CmFrameState* st, const SortPairs& b, uint32_t n_pass, uint32_t nt, uint32_t n_slots,
                      bool lds_rank, uint32_t* tile_kept, const char* scatter_mark);

// cm_byproducts.cpp: the tables computed from the last result on request. Called with merge_mu held.
// The tables of the last result go with it (where a merge replaces the result).
inline void invalidate_result_tables(cm_ctx* c) { c->cov_have = c->nrm_have = c->aln_fit.have = c->ndt_fit.have = c->grid_have = c->ray_have = false; }
// The covariance table of the last result (cov_entries, n_out entries).
int voxel_cov(cm_ctx* c, const cm_cov_params& q);
// The cluster tables of the last result (cl_labels, cl_clusters, cl_indices, cl_n_clusters, cl_n_clustered).
// more_stages: the caller goes on launching and closes the stage list itself.
int clusters(cm_ctx* c, const cm_cluster_params& q, bool more_stages = false);
// The box table of the last result's clusters at q.cluster (box_entries, box_n entries), behind the cluster tables.
int cluster_boxes(cm_ctx* c, const cm_box_params& q);
// The direction table of n_angles headings (1..CM_BOX_MAX_ANGLES): 2 * n_angles floats.
void box_direction_table(uint32_t n_angles, float* cos_sin);
// The grid map of the last frame at q (grid_cells and grid_image, grid_n = q.nx * q.ny cells).
// more_stages: the caller goes on launching and closes the stage list itself.
int grid_map(cm_ctx* c, const cm_grid_params& q, bool more_stages = false);
// The grid map at q and behind it the rays of the last frame at r (ray_cells and ray_image, ray_n = q.nx * q.ny cells).
int grid_rays(cm_ctx* c, const cm_grid_params& q, const cm_ray_params& r);
// The normal table of the last result (nrm_entries, n_out entries).
int normals(cm_ctx* c, const cm_normal_params& q);
// Registration of the n_src source records at src_dev against the last result: *out, and the correspondences in aln_fit.corr.
int align(cm_ctx* c, const cm_align_params& q, const void* src_dev, uint64_t n_src, cm_align_result* out);
// NDT registration of the n_src source records at src_dev against the last result's covariance table at cov (resolved, never
// {0, 0}): *out, and the correspondences in ndt_fit.corr.
int ndt(cm_ctx* c, const cm_ndt_params& q, const cm_cov_params& cov, const void* src_dev, uint64_t n_src, cm_ndt_result* out);
