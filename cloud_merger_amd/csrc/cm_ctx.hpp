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
//
// Every allocation the context owns is a DevBuf or a PinnedBuf (cm_devbuf.hpp): it is freed with the context, and where it
// grows its own capacity says how far. A plain pointer in these structs is a view of memory owned elsewhere.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/cloudmerge.h"
#include "cm_devbuf.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_map_layers.hpp"
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
    DevBuf<void> buf[2];                 // owned HBM buffers (host submits)
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
    DevBuf<uint32_t> keys_a, keys_b, vals_a, vals_b; // n_slots words each (a multiple of CM_TILE)
    DevBuf<uint32_t> hist, grp;          // (n_slots / CM_TILE) rows; CM_MAX_PASSES x groups rows
    DevBuf<uint32_t> totals;             // CM_RADIX digit totals (k_gscan)
    // Room for n_slots pairs: a buffer that is too small is freed and allocated anew (`what`: the error text of a failure).
    int reserve(cm_ctx* c, uint32_t n_slots, const char* what);
    // gw: words of one pass's group totals in the sort at hand.
    SortPairs pairs(uint32_t gw) const { return {keys_a, keys_b, vals_a, vals_b, hist, totals, grp, grp + gw}; }
};

// A result's centroids in the order of a search grid over their own bounds (k_cl_bounds, k_cl_keys, the radix passes,
// k_cl_gather, cmk_sorted_rows): what the cluster extraction, the normals and the registration search in. The sorted keys lie
// in sort.keys_a / keys_b (state says which), the grid is the caller's choice (cm_byproducts.cpp build_search_index).
struct SearchIndex {
    PairSort sort;
    DevBuf<CmFrameState> state;          // the sort's state record (the cluster call keeps a second one behind it)
    DevBuf<uint32_t> bounds;             // six order-images: min x, y, z, max x, y, z of the centroids
    DevBuf<void> pts;                    // the centroids in search-grid order (x, y, z, result index)
    DevBuf<uint32_t> aux;                // 3 x n_slots words: the three arrays k_cl_gather initialises for the cluster call,
                                         // laid out at the n_slots of the build at hand (aux, aux + n_slots, aux + 2 n_slots),
                                         // not at the capacity
    DevBuf<void> rows;                   // (y,z)-row ranges of the search grid
    CmClusterGridDev grid{};             // the grid of the last build, as the search kernels take it
};

// The state of a registration's Gauss-Newton loop (cm_byproducts.cpp fit_pose): align's and ndt's.
struct PoseFit {
    DevBuf<void> corr;                   // one correspondence per source record: the last evaluation's
    DevBuf<double> part;                 // CM_ALIGN_STRIDE doubles per block of 256 source records
    DevBuf<double> sums;                 // CM_ALIGN_SUMS doubles: what the host reads back per evaluation
    DevBuf<void> src;                    // the device copy of a host source (records of 16 bytes)
    bool have = false;                   // corr holds the table of a call since the last merge, n_src entries
    uint64_t n_src = 0;
    // Room for n_src records of corr_bytes each (what_state, what_table: the error texts of a failure).
    int reserve(cm_ctx* c, uint64_t n_src, size_t corr_bytes, const char* what_state, const char* what_table);
};

// Rolling log-odds occupancy map (cm_kernels_map.hip), configured by cm_map_configure and fed by cm_map_integrate after a
// frame: the one by-product that survives merges (invalidate_result_tables leaves it alone). Buffers of its own — no frame
// and no other by-product reads them —, all allocated by the configure call, so an integrate call allocates nothing.
struct MapLayer {
    cm_map_params params{};
    DevBuf<void> state[2];           // cm_map_cell per window cell, twice: k_map_update reads one and writes the other
    int cur = 0;                     // which of the two holds the map
    DevBuf<void> image;              // the three-valued image: one byte per cell
    DevBuf<uint32_t> bits;           // 2 * max_sensors bitmaps of ceil(cells / 32) words: the E bitmaps, then the H bitmaps
    DevBuf<void> rays;               // k_ray_cast's scratch table: (n_pass, n_end) per cell
    cm_map_info info{};              // anchor, size, integrations since the configure call, who cast in the last one
    uint64_t serial = 0;             // the frame integrated last (0: none since the configure call)
};

// Cost layer over the occupancy map (cm_kernels_cost.hip), configured by cm_map_cost_configure behind the map and
// recomputed by cm_map_cost_update from map.image. Buffers of its own, all allocated by the configure call; it lives and
// goes with the map (map_configure frees it).
struct CostLayer {
    cm_cost_params params{};
    uint32_t radius = 0;            // R: the table has R * R + 1 entries
    DevBuf<unsigned char> cells;    // the inflated cost: one byte per cell
    DevBuf<uint32_t> dist2;         // the squared distance: one word per cell
    DevBuf<uint32_t> masks;         // the column pass: ceil(ny / CM_COST_ROWS) * nx obstacle words, then as many carry words
    DevBuf<unsigned char> lut;      // the table in HBM
    std::vector<unsigned char> lut_host;   // and as it was built
};

// Plan layer behind the cost layer (cm_kernels_plan.hip), configured by cm_map_plan_configure and recomputed by
// cm_map_plan_update from cost.cells. Buffers of its own, all allocated by the configure call; it lives and goes with the
// cost layer (map_cost_configure frees it).
struct PlanLayer {
    cm_plan_params params{};
    cm_plan_info info{};
    DevBuf<uint32_t> pot;           // the potential: one word per cell
    DevBuf<uint32_t> words;         // CM_PLAN_BATCH sweep counters, then two tables of tile flags
    DevBuf<uint32_t> path;          // CM_PLAN_PATH_HEAD words, then max_path_cells cells
    PinnedBuf<uint32_t> host;       // what the host reads back: the counters of a batch, a path's head
};

// Rollout layer behind the plan layer (cm_kernels_traj.hip), configured by cm_map_traj_configure and evaluated by
// cm_map_traj_evaluate from cost.cells and plan_layer.pot. Buffers of its own, all allocated by the configure call; it lives and
// goes with the plan layer (map_plan_configure frees it).
struct TrajLayer {
    cm_traj_params params{};
    uint32_t n_foot = 0;
    cm_traj_info info{};
    DevBuf<CmTrajScoreDev> scores;  // nv * nw records
    DevBuf<uint32_t> words;         // CM_TRAJ_INFO_WORDS info words, then nv step lengths (fp32) and nw heading increments
    DevBuf<float> consts;           // the heading table (2 * CM_TRAJ_HEADINGS floats), then the footprint (2 * n_foot)
    PinnedBuf<uint32_t> host;       // CM_TRAJ_INFO_WORDS words read back, then the nv + nw words an evaluate uploads
    std::vector<float> v, w;   // the samples of the last evaluate (nv and nw entries from the configure call on)
};

// Frontier layer behind the plan layer (cm_kernels_front.hip), configured by cm_map_frontier_configure and recomputed by
// cm_map_frontier_update from map.image, cost.cells and plan_layer.pot. Buffers of its own, all allocated by the configure call;
// it lives and goes with the plan layer (map_plan_configure frees it).
struct FrontLayer {
    cm_frontier_params params{};
    cm_frontier_info info{};
    DevBuf<uint32_t> labels;       // a word per cell: parents, then roots, then the frontier numbers
    DevBuf<uint32_t> words;        // a size word per cell, the counts of the scan (one per CM_FRONT_BLOCK cells), CM_FRONT_INFO_WORDS info words
    DevBuf<CmFrontEntryDev> table; // max_frontiers entries
    DevBuf<uint32_t> box;          // four words per entry: the box while it is reduced
    PinnedBuf<uint32_t> host;      // CM_FRONT_INFO_WORDS words read back
};

// Scan matching layer behind the cost layer (cm_kernels_match.hip), configured by cm_map_match_configure and evaluated by
// cm_map_match_evaluate from the frame at rest, map.info and cost.dist2. Buffers of its own, all allocated by the
// configure call; it lives and goes with the cost layer (map_cost_configure frees it).
struct MatchLayer {
    cm_match_params params{};
    uint32_t radius = 0;           // R: the field table has R * R + 1 entries
    cm_match_result result{};
    DevBuf<unsigned char> field;   // nx * ny bytes L, then the field table
    DevBuf<uint32_t> bits;         // 2 * n_a + 1 bitmaps of (nx * ny + 31) / 32 words
    DevBuf<uint32_t> vol;          // the volume, then CM_MATCH_INFO_WORDS info words
    DevBuf<float> q;               // six floats per candidate
    PinnedBuf<uint32_t> host;      // CM_MATCH_INFO_WORDS words read back, then the candidates' floats an evaluate uploads
    std::vector<unsigned char> lut_host;
};

// Search layer behind the cost layer (cm_kernels_msearch.hip): branch-and-bound scan matching over wide windows,
// configured by cm_map_match_search_configure and evaluated by cm_map_match_search from the same inputs as the layer
// above. Buffers of its own, all allocated by the configure call; it lives and goes with the cost layer too.
struct SearchLayer {
    cm_match_search_params params{};
    uint32_t radius = 0;         // R: the field table has R * R + 1 entries
    uint32_t n_roots = 0;
    cm_match_result result{};
    cm_match_search_info info{};
    DevBuf<unsigned char> pyr;   // levels 0 .. depth (level_offset), then the field table
    DevBuf<uint32_t> bits;       // 2 * n_a + 1 bitmaps of (nx * ny + 31) / 32 words
    DevBuf<uint32_t> cells;      // 2 * n_a + 1 cell lists of max_cells words, then as many counts
    DevBuf<uint32_t> nodes;      // the roots, two node lists of max_nodes words, the scores of max_nodes words, CM_MSEARCH_WORDS info words
    DevBuf<float> q;             // six floats per candidate
    PinnedBuf<uint32_t> host;    // CM_MSEARCH_WORDS words read back, 256 counts, CM_MSEARCH_WORDS words an evaluate uploads, then the candidates' floats
};

// Localisation layer behind the cost layer (cm_kernels_mcl.hip): a particle filter against the matching layer's field,
// configured by cm_map_mcl_configure and driven by cm_map_mcl_init_* / _predict / _update from the frame at rest, map.info,
// map.image and cost.dist2. Buffers of its own, all allocated by the configure call; it lives and goes with the cost layer.
struct MclLayer {
    bool init = false;               // the particles are initialised (an init call since the configure call)
    uint64_t gen = 0;                // init, predict and update calls since the configure call
    cm_mcl_params params{};
    uint32_t radius = 0;             // R: the field table has R * R + 1 entries
    cm_mcl_info info{};
    DevBuf<CmMclParticleDev> parts[2];      // n_particles each: the resampling gathers from one into the other
    int cur = 0;                     // which of the two holds the particles
    DevBuf<CmMclWeightDev> wts;      // n_particles records
    DevBuf<unsigned long long> cum;  // n_particles prefix sums, then CM_MCL_WORDS info words
    DevBuf<unsigned char> field;     // nx * ny bytes L, then the field table
    DevBuf<uint32_t> bits;           // one bitmap: the body cells ((2 range_cells + 1)^2 bits) or the free cells (nx * ny bits)
    DevBuf<uint32_t> list;           // CM_MCL_ONE_BLOCK block counts, then max(max_beams, nx * ny) list entries
    DevBuf<float> dirs;              // the heading table (2 * CM_TRAJ_HEADINGS floats)
    PinnedBuf<unsigned long long> host;     // CM_MCL_WORDS words read back
    // The beam model (cm_map_mcl_beam_configure, k_mcl_beam): a second scoring mode, off by default. All of it allocated by
    // that call; cm_map_mcl_configure and whatever frees the layer assign the struct afresh, which frees the mode with it.
    bool beam_on = false;
    bool beam_steps_fresh = false;   // beam_steps is that of the current dist2
    bool beam_info_have = false;     // the last update ran the beam model: beam_info is its
    cm_mcl_beam_params beam_params{};
    cm_mcl_beam_info beam_info{};
    DevBuf<unsigned char> beam_steps;       // nx * ny bytes: the skip table (cmk_cast_steps)
    DevBuf<unsigned char> beam_table;       // 2 * over_cells + 3 bytes
    DevBuf<unsigned long long> beam_counts; // CM_MCL_BEAM_COUNTS words
    PinnedBuf<unsigned long long> beam_host;        // the counts read back
    // The hypotheses and the recovery (cm_map_mcl_hyp_configure, k_mcl_hyp_*): a second mode, off by default, allocated and
    // freed like the beam model.
    bool hyp_on = false;
    bool hyp_have = false;           // the last update ran the mode: hyp_info and hyp_out are its
    cm_mcl_hyp_params hyp_params{};
    cm_mcl_hyp_info hyp_info{};
    uint32_t hyp_cap_bits = 0;       // the table of bins has 1 << hyp_cap_bits slots
    std::vector<cm_mcl_hyp> hyp_out; // the hypotheses of the last update (reserved by the configure call)
    DevBuf<unsigned long long> hyp_keys;    // cap keys
    DevBuf<uint32_t> hyp_slots;      // cap parent words, cap component words, then n_particles slot words
    DevBuf<CmMclHypRecDev> hyp_rec;  // n_particles records, then CM_MCL_HYP_MAX chosen ones
    DevBuf<unsigned long long> hyp_words;   // CM_MCL_HYP_WORDS
    DevBuf<uint32_t> hyp_bits;       // the free cells' bitmap (nx * ny bits)
    DevBuf<uint32_t> hyp_list;       // CM_MCL_ONE_BLOCK block counts, then nx * ny list entries
    PinnedBuf<unsigned long long> hyp_host; // CM_MCL_HYP_WORDS words, then the chosen records read back
};

// Cast layer behind the cost layer (cm_kernels_cast.hip): expected ranges from many poses, configured by cm_map_cast_configure
// and evaluated by cm_map_cast_evaluate / _evaluate_mcl from map.info, map.image, cost.dist2 and, for the latter, mcl.parts.
// Buffers of its own, all allocated by the configure call; it lives and goes with the cost layer.
struct CastLayer {
    bool steps_fresh = false;       // steps is that of the current dist2
    cm_cast_params params{};
    cm_cast_info info{};
    DevBuf<CmCastRayDev> rays;      // max_poses * n_bearings records
    DevBuf<uint32_t> poses;         // max_poses poses of three words, as an evaluate uploads them
    DevBuf<uint32_t> bearings;      // n_bearings binary angles
    DevBuf<uint32_t> dirs;          // CM_CAST_DIRS pairs of int16_t
    DevBuf<unsigned char> steps;    // nx * ny bytes: the skip table
    DevBuf<uint32_t> words;         // CM_CAST_WORDS status counts
    PinnedBuf<uint32_t> host;       // the counts read back
};

struct cm_ctx {
    ~cm_ctx();                           // the streams and events it created (cm_api.cpp); the buffers go by themselves
    int device = 0;
    uint32_t flags = 0, max_sensors = 0;
    uint64_t max_points = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    Slot slots[CM_MAX_SENSORS];

    uint32_t cap_padded = 0, cap_tiles = 0, cap_seg_tiles = 0;
    DevBuf<uint32_t> keys_a, keys_b, vals_a, vals_b;
    DevBuf<uint32_t> hist, grp, totals, seg_counts, seg_tile_counts, seg_groups;
    uint32_t cap_groups = 0, frame_seq = 0;
    DevBuf<void> stage32;                // k3_local's staging for partial tables (32-byte entries)
    DevBuf<void> out32;                  // the result as pcl::PointXYZI images (cm_result_copy with point_step_out 32)
    DevBuf<float> partials;
    DevBuf<uint32_t> out_key, out_cnt, merged_total;
    DevBuf<void> out;
    DevBuf<void> merged;
    DevBuf<unsigned char> mask;          // outlier stage: keep-mask over the padded point indices
    DevBuf<void> sorted_pts;             // outlier stage: points in radius-grid order
    DevBuf<void> rows;                   // outlier stage: (y,z)-row ranges
    DevBuf<CmFrameState> d_state_o;      // outlier stage: its grid and counts
    const unsigned char* frame_mask = nullptr;   // mask of the last frame (nullptr: stage off)
    DevBuf<void> partial;                // cm_partial_entry table of the last cm_merge_partial
    DevBuf<void> table_entries;          // merged entries inside cm_merge_tables
    int last_mode = 0;                   // what the last result is: 0 centroids, 1 partial table, 2 merged tables
    DevBuf<CmFrameDev> d_frame;
    DevBuf<CmTileDev> d_tiles;           // per-tile entries of the uploaded descriptor (k_setup)
    CmFrameDev frame_uploaded;
    bool frame_uploaded_valid = false;
    DevBuf<CmFrameState> d_state[2];
    int cur = 0;
    PinnedBuf<CmFrameState> h_state;     // pinned, written by the last kernel of a frame
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
    DevBuf<CmGroundDev> d_ground;
    DevBuf<CmFrameState> d_state_g;      // state of the slab sort
    DevBuf<unsigned char> gmask;         // ground points of the last frame (padded index space)
    DevBuf<uint32_t> zone_off;
    DevBuf<CmGroundPlaneDev> d_planes;
    DevBuf<void> hyp0;                   // first round of hypotheses of every slab: planes, validity, inlier counts
    DevBuf<uint32_t> valid0, counts0;
    DevBuf<double> chunk_sums;           // least-squares sums per chunk of band points
    bool frame_had_ground = false;
    float ground_outlier_radius = 0.f;   // > 0: radius filter on every slab's band points that are not ground (:119)
    uint32_t ground_outlier_min_nb = 0;
    DevBuf<unsigned char> bmask;         // those points (input of that filter)
    DevBuf<unsigned char> zcode;         // slab of every band point

    // bucket path (cm_kernels_v2.hip)
    DevBuf<void> rec_a, rec_b;           // 16-byte point records, ping-pong
    DevBuf<unsigned char> dig;           // next digit of every record
    DevBuf<unsigned long long> tile_state; // published kept-voxel counts of the local finish
    DevBuf<uint32_t> wave_cnt;           // records k2_hist0 packed per wave (frames whose crop box drops most points)
    DevBuf<float> records;               // min/max/count per tile
    int cell_min_b[3] = {0, 0, 0}, cell_div_b[3] = {1, 1, 1};   // grid the cells in out_key are relative to

    // pipelined publish (cm_result_publish_async): the result buffers exist twice, so that the copy-out of frame n runs on
    // its own stream beside the kernels of frame n + 1
    DevBuf<void> out_other;              // the result buffer the frame in flight does NOT write
    DevBuf<void> out32_other;
    hipStream_t pub_stream = nullptr;
    hipEvent_t ev_pub[2] = {nullptr, nullptr};   // [0]: the last copy-out that read `out`, [1]: ... `out_other`
    bool pub_pending[2] = {false, false};

    // quantile passes (cm_kernels_v4.hip): one global pass into buckets cut at the last frame's quantiles
    DevBuf<uint32_t> spl[2];             // splitters: route.spl_cur says which one the next frame reads
    DevBuf<uint32_t> qcnt, qtot, qbofs;  // per-tile bucket counts / prefixes, bucket totals, bucket starts
    DevBuf<uint32_t> qbig;               // buckets beyond CM4_CAP records: count, then their numbers
    DevBuf<uint16_t> qbid;               // the bucket of every padded slot
    uint32_t hist_resident[3] = {0, 0, 0};   // workgroups of k4_hist<11 .. 13> resident at once on this device (0: not asked yet)

    // per-sensor figures of the last enqueued frame (cm_frame_stats)
    uint32_t stats_n_sensors = 0;
    uint32_t stats_sensor[CM_MAX_SENSORS] = {0}, stats_n[CM_MAX_SENSORS] = {0}, stats_fresh[CM_MAX_SENSORS] = {0};
    uint64_t stats_bytes[CM_MAX_SENSORS] = {0}, stats_gen[CM_MAX_SENSORS] = {0};
    uint32_t* d_tile_kept = nullptr;     // per 4096-slot tile: points that passed crop / masks and entered the sort — the first scatter
    PinnedBuf<uint32_t> h_tile_kept;     // writes them straight into pinned host memory (d_tile_kept is its device view)
    uint64_t bytes_d2h = 0;              // result / merged / ground bytes copied to the host since the frame was enqueued

    // ego-motion compensation (cm_kernels_motion.hip): k_motion writes the frame's compensated points here, at their padded
    // indices, and the descriptor points at them; they live as long as the frame's by-products (until the next enqueue)
    bool motion_on = false;
    cm_motion motion;
    DevBuf<unsigned char> motion_buf;    // cap_padded x 16 B, allocated by the first cm_set_ego_motion
    bool last_motion = false;            // the frame enqueued last was compensated (CM_PATH_MOTION)

    // per-voxel covariance of the result (cm_kernels_cov.hip), on request after a frame: buffers of its own — no frame reads
    // them — allocated by the first request and grown with the frames. (The merged records go to `merged`, which
    // cm_merged_copy fills with the same bytes and which no frame reads either.)
    PairSort cov;                        // (voxel number, record index), sized for the frame's padded points
    DevBuf<uint32_t> cov_tile_counts;    // cap_tiles words: cmk_merged's per-tile offsets
    DevBuf<uint32_t> cov_words;          // [0] merged records, [1] error word of k_cov_reduce
    DevBuf<CmFrameState> cov_state;      // the sort's state record
    DevBuf<void> cov_entries;            // the table: cm_voxel_cov per voxel
    bool cov_have = false;               // cov_entries holds the table of the result at rest, computed with these parameters:
    uint32_t cov_min_points = 0;         // what ndt() reuses
    float cov_eig_mult = 0.0f;

    // Euclidean cluster extraction on the result (cm_kernels_cluster.hip), on request after a frame: buffers of its own — no
    // frame reads them — allocated by the first request and grown with the results. It reads `out` (and out_cnt).
    SearchIndex cl;                      // two state records: the sort by cell, the sort by cluster number; its aux words are
                                         // the union-find's parent, size and point count per voxel
    DevBuf<uint32_t> cl_root, cl_num;
    DevBuf<uint32_t> cl_labels;          // the label table
    DevBuf<void> cl_tile_sums;           // per tile: kept roots and their voxels, then their exclusive prefixes
    DevBuf<uint32_t> cl_words;           // [0] clusters, [1] clustered voxels
    DevBuf<void> cl_clusters;            // the cluster table: cm_cluster per cluster
    const uint32_t* cl_indices = nullptr;   // the member lists of the last call (one of cl.sort.vals_a / vals_b)
    uint64_t cl_n_clusters = 0, cl_n_clustered = 0;

    // Oriented boxes of the clusters (cm_kernels_box.hip), on request after a frame: the cluster call, then the fit. Buffers of
    // its own — no frame reads them — allocated by the first request and grown with the results.
    DevBuf<void> box_entries;            // the table: cm_cluster_box per cluster
    uint64_t box_n = 0;                  // its entries: the clusters of the last box call (0 after a cluster call)
    DevBuf<void> box_dirs;               // CM_BOX_MAX_ANGLES (cos, sin) pairs: the direction table at box_dirs_n headings
    uint32_t box_dirs_n = 0;
    float box_dirs_host[2 * CM_BOX_MAX_ANGLES];   // what the upload reads
    DevBuf<uint32_t> box_words;          // [0] listed (large) clusters, [1] their chunks
    DevBuf<void> box_list, box_ext;      // per listed cluster: (cluster, first chunk row); the extremes' images
    DevBuf<void> box_work;               // per listed chunk: (slot, chunk)
    DevBuf<double> box_sums;             // per listed chunk: CM_BOX_MAX_ANGLES sums
    uint32_t box_split = CM_BOX_SPLIT;   // (CM_BOX_SPLIT in the environment: the measurement of scripts/box_cost.py)
    uint32_t mcl_beam_walks = CM_MCL_BEAM_WALKS;     // (CM_MCL_BEAM_WALKS in the environment: scripts/map_mcl_beam_cost.py)
    uint32_t mcl_hyp_agg = 1;        // (CM_MCL_HYP_NO_AGG=1 in the environment sets 0: scripts/map_mcl_hyp_cost.py)

    // 2-D grid map of the frame (cm_kernels_grid.hip), on request after a frame: it reads the frame's clouds in place (d_frame,
    // frame_mask, gmask) and writes a table and an image of its own — no frame reads them — allocated by the first request and
    // grown with the grids asked for.
    DevBuf<void> grid_cells;             // the table: cm_grid_cell per cell
    DevBuf<void> grid_image;             // the occupancy image: one byte per cell
    uint64_t grid_n = 0;                 // cells of the last grid call
    bool grid_have = false;              // the two hold the grid of the result at rest (cleared where a merge replaces it)

    // Free-space ray casting over the grid map (cm_kernels_rays.hip), on request after a frame, behind the grid map of the
    // same call: the per-sensor bitmaps of end cells, the table and the cleared image — no frame reads them — allocated by the
    // first request and grown together.
    float frame_origin[CM_MAX_SENSORS][3] = {};   // per descriptor sensor the (x, y, z) translation of the matrix the last frame
                                                  // was built with (build_frame; under deskew the descriptor's own is the
                                                  // identity). Read by grid_rays (x, y) and map_integrate, by nothing else.
    DevBuf<uint32_t> ray_bits;           // max_sensors bitmaps of ceil(cells / 32) words
    DevBuf<void> ray_cells;              // the table: cm_grid_ray_cell per cell
    DevBuf<void> ray_image;              // the cleared occupancy image: one byte per cell
    uint64_t ray_n = 0;                  // cells of the last ray call
    bool ray_have = false;               // they hold the rays of the result at rest (cleared by a merge and by a grid call)

    // The occupancy map and the layers behind it (cm_map_layers.hpp has the tree): the one family of by-products that survives
    // merges (invalidate_result_tables leaves it alone). `layers` says which of them are configured and whose result is stale;
    // each struct holds one layer's parameters, result and buffers, so that giving a layer back is assigning a fresh struct.
    uint64_t frame_serial = 0;           // counts the frames enqueued (enqueue, merge_tables): the frame at rest is this one
    MapLayers layers;
    MapLayer map;
    CostLayer cost;
    PlanLayer plan_layer;                // (`plan` is the frame's)
    TrajLayer traj;
    FrontLayer front;
    MatchLayer match;
    SearchLayer msearch;
    MclLayer mcl;
    CastLayer cast;

    // Normals and curvature of the result (cm_kernels_normals.hip), on request after a frame: buffers of its own, as the
    // cluster extraction's — no frame reads them — allocated by the first request and grown with the results. It reads `out`.
    SearchIndex nrm;
    DevBuf<void> nrm_list;               // 8 B per voxel: the centroids the first search launch could not finish
    DevBuf<uint32_t> nrm_words;          // [0] list count, [1] unused
    DevBuf<void> nrm_entries;            // the table: cm_voxel_normal per voxel
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
    DevBuf<uint32_t> ndt_bounds;         // six bounds images (k_cl_bounds)

    // statistical outlier removal (cm_kernels_sor.hip): sorts by the outlier stage's grid (sorted_pts, rows, d_state_o) and
    // leaves its keep-mask in `mask`; its own buffers are allocated by the first cm_set_statistical_outlier
    bool sor_on = false;
    cm_sor_params sor;
    DevBuf<float> sor_d;                 // cap_padded floats: d_i per padded index (0xFFFFFFFF: not in the stage's input)
    DevBuf<void> sor_list;               // cap_padded x 8 B: the points the first search launch could not finish, and their bound
    DevBuf<unsigned long long> sor_words; // CM_SOR_WORDS: bins, list count, stats record
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

// The buffers that more than one place allocates on first use, each with its size stated here once. false: out of memory.
inline bool ensure_merged(cm_ctx* c) { return c->merged.once(static_cast<size_t>(c->cap_padded) * 16); }
inline bool ensure_partial(cm_ctx* c) { return c->partial.once(static_cast<size_t>(c->cap_padded) * 32); }
inline bool ensure_out32(cm_ctx* c) { return c->out32.once(static_cast<size_t>(c->cap_padded) * 32); }
inline bool ensure_mask(cm_ctx* c) { return c->mask.once(c->cap_padded); }
inline bool ensure_sorted_pts(cm_ctx* c) { return c->sorted_pts.once(static_cast<size_t>(c->cap_padded) * 16); }
// (what the outlier stages' sort writes: cell_sort, and cm_set_statistical_outlier ahead of the first frame that runs it)
inline bool ensure_cell_sort(cm_ctx* c) {
    return ensure_sorted_pts(c) && c->rows.once(static_cast<size_t>(CM_ROW_TABLE_CAP) * 8) && c->d_state_o.once(1);
}

// cm_launch.cpp. Every one of them is called with merge_mu held.
// Builds the frame descriptor. peek == nullptr: in c->frame, and the frame takes the sensors' fresh clouds. Otherwise in *peek,
// from the clouds the next frame would read, and nothing of the last frame changes. A refusal changes nothing either.
int build_frame(cm_ctx* c, const cm_params* p, CmFrameDev* peek, std::vector<std::unique_lock<std::mutex>>& locks);
// Uploads c->frame unless HBM holds it already (a peek leaves its own descriptor there). Every call that reads the last
// frame's clouds through d_frame after the frame has finished starts with it; behind a frame it costs one memcmp.
void frame_on_device(cm_ctx* c);
// The frame's points that `mask` keeps (nullptr: every valid one) as 16-byte records in (sensor, point) order into `out`,
// and their number (a host round trip). tile_counts: cap_tiles words.
int fuse_points(cm_ctx* c, uint32_t* tile_counts, void* out, const unsigned char* mask, uint32_t* total);
// k_minmax over the uploaded descriptor, which has n_tiles tiles, and a host round trip: the bounds of its valid points and
// their count.
int measure_bounds(cm_ctx* c, uint32_t n_tiles, float mn[3], float mx[3], uint64_t* n_valid);
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
// The tables of the last result go with it (where a merge replaces the result). The occupancy map is not one of them: it
// accumulates over the frames and stays.
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
// The occupancy map and its layers (cm_map_layers.hpp has the tree, the refusals and the staleness rule; each layer's state is
// one struct above). Every *_configure below works alike: the layers below the one at hand are given back (their structs
// assigned afresh, which frees their buffers), then nullptr gives back the layer itself, and anything else reserves its
// buffers — which allocates nothing where they fit —, uploads its tables and leaves the layer on and stale since this call.
// Every producer marks its layer failed before it launches and fresh once its result is read back, and marks the layers
// below stale where it changes what they read.
// The occupancy map. map_configure: room for q's window, cleared (nullptr: the buffers go). map_vehicle_cell: the absolute
// cell of the pose's translation at the configured cell size, false where it does not exist. map_integrate: the last frame
// under `pose` into the map, whose window is then anchored around the vehicle cell v.
int map_configure(cm_ctx* c, const cm_map_params* q);
bool map_vehicle_cell(const cm_ctx* c, const float pose[12], int v[2]);
// The window cell of a world position (step 1 per axis, minus the anchor); false: not finite, no such cell, or outside the window.
bool map_window_cell(const cm_ctx* c, float x, float y, uint32_t cell[2]);
int map_integrate(cm_ctx* c, const float pose[12], const int v[2]);
// The cost layer over the occupancy map. map_cost_configure: room for the map's window and the table of q at radius R cells
// (nullptr: the buffers go). map_cost_update: dist2 and cost of the map's current image.
int map_cost_configure(cm_ctx* c, const cm_cost_params* q, uint32_t R);
int map_cost_update(cm_ctx* c);
// The plan layer behind the cost layer. map_plan_configure: room for the map's window and q's longest path (nullptr: the
// buffers go). map_plan_update: pot for the goal's window cell. map_plan_path: the walk from the start's window cell into
// plan_layer.path; head receives its CM_PLAN_PATH_HEAD words.
int map_plan_configure(cm_ctx* c, const cm_plan_params* q);
int map_plan_update(cm_ctx* c, const uint32_t goal[2]);
int map_plan_path(cm_ctx* c, const uint32_t start[2], uint32_t head[4]);
// The rollout layer behind the plan layer. traj_direction_table: the 2 * CM_TRAJ_HEADINGS floats of step 2 (built once).
// traj_samples: the n samples of step 1 between lo and hi. map_traj_configure: room for q's samples and the footprint, which
// is uploaded with the heading table (nullptr: the buffers go). map_traj_evaluate: the scores and traj.info for a window that
// cm_map_traj_evaluate has checked, from the start's window cell.
const float* traj_direction_table();
void traj_samples(float lo, float hi, uint32_t n, float* out);
int map_traj_configure(cm_ctx* c, const cm_traj_params* q, const float* foot_xy, uint32_t n_foot);
int map_traj_evaluate(cm_ctx* c, const cm_traj_window& w, const uint32_t start[2]);
// The frontier layer behind the plan layer. map_frontier_configure: room for the map's window and q's table (nullptr: the
// buffers go). map_frontier_update: labels, table and front.info of the current image, cost table and pot.
int map_frontier_configure(cm_ctx* c, const cm_frontier_params* q);
int map_frontier_update(cm_ctx* c);
// The scan matching layer behind the cost layer. map_match_configure: room for q's candidates over the map's window and the
// field table at radius R cells, which is built and uploaded (nullptr: the buffers go). map_match_evaluate: the volume and
// match.result for a prior that cm_map_match_evaluate has checked.
int map_match_configure(cm_ctx* c, const cm_match_params* q, uint32_t R);
int map_match_evaluate(cm_ctx* c, const float pose[12]);
// The localisation layer behind the cost layer. map_mcl_configure: room for q's particles and beams over the map's window and
// the field table at radius R cells (nullptr: the buffers go). The other four run a call that cm_api.cpp has checked: v holds
// the centre or the motion (x, y, yaw) and its three standard deviations. map_mcl_init_uniform refuses an image without a
// free cell itself (it learns the number from the device).
int map_mcl_configure(cm_ctx* c, const cm_mcl_params* q, uint32_t R);
int map_mcl_init_pose(cm_ctx* c, const float v[6]);
int map_mcl_init_uniform(cm_ctx* c);
int map_mcl_predict(cm_ctx* c, const float v[6]);
int map_mcl_update(cm_ctx* c);
// The beam model of the localisation layer: its memory and table (nullptr: back to the field score); the weights and the
// infos go stale, the particles and gen stay.
int map_mcl_beam_configure(cm_ctx* c, const cm_mcl_beam_params* q);
// The hypotheses mode: all its memory; nullptr gives it back. The averages start at 0.0.
int map_mcl_hyp_configure(cm_ctx* c, const cm_mcl_hyp_params* q);
// The cast layer behind the cost layer. map_cast_configure: room for q's rays over the map's window, the bearings (nullptr:
// evenly spaced) and the direction table uploaded (q nullptr: the buffers go). map_cast_evaluate runs a call that cm_api.cpp has
// checked: n poses on the host, or, with host_poses nullptr, the localisation layer's n particles in place.
// cast_direction_table: the CM_CAST_DIRS pairs of step 3 for range_cells into dst.
void cast_direction_table(uint32_t range_cells, int16_t* dst);
int map_cast_configure(cm_ctx* c, const cm_cast_params* q, const uint32_t* bearings);
int map_cast_evaluate(cm_ctx* c, const cm_cast_pose* host_poses, uint32_t n);
// A recorded state table into the configured map (cm_map_load has checked it): state, image, anchor, staleness.
int map_load(cm_ctx* c, const cm_map_cell* src, const int32_t anchor[2]);
// The search layer behind the cost layer. map_msearch_configure: room for q over the map's window, the field table at radius
// R cells built and uploaded, the roots built and uploaded (nullptr: the buffers go). map_msearch_evaluate: msearch.result and
// msearch.info for a prior that cm_map_match_search has checked; CM_CAPACITY leaves the result stale and the info written.
// msearch_level_offset: where level h starts in msearch.pyr.
int map_msearch_configure(cm_ctx* c, const cm_match_search_params* q, uint32_t R);
int map_msearch_evaluate(cm_ctx* c, const float pose[12]);
size_t msearch_level_offset(uint32_t nx, uint32_t ny, uint32_t h);
// The normal table of the last result (nrm_entries, n_out entries).
int normals(cm_ctx* c, const cm_normal_params& q);
// Registration of the n_src source records at src_dev against the last result: *out, and the correspondences in aln_fit.corr.
int align(cm_ctx* c, const cm_align_params& q, const void* src_dev, uint64_t n_src, cm_align_result* out);
// NDT registration of the n_src source records at src_dev against the last result's covariance table at cov (resolved, never
// {0, 0}): *out, and the correspondences in ndt_fit.corr.
int ndt(cm_ctx* c, const cm_ndt_params& q, const cm_cov_params& cov, const void* src_dev, uint64_t n_src, cm_ndt_result* out);
