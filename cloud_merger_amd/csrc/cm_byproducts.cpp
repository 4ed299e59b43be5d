// cm_byproducts.cpp — the tables computed from a frame's result on request, after the frame is done: the per-voxel covariance
// (voxel_cov), the cluster extraction (clusters) and the boxes of its clusters (cluster_boxes), normals and curvature (normals), the two registrations of a source cloud
// (align, ndt), and the tables computed from the frame's points rather than its result, the 2-D grid map (grid_map) and the rays cast over it (grid_rays), and the occupancy map those rays accumulate into over the frames (map_configure, map_integrate: the one table a
// merge does not drop) with the cost layer over its image (map_cost_configure, map_cost_update) and the plan layer behind that (map_plan_configure, map_plan_update, map_plan_path) and the rollout layer behind the plan (map_traj_configure, map_traj_evaluate) and the frontier layer behind it too (map_frontier_configure, map_frontier_update), and the scan matching of the frame against the map behind the cost layer (map_match_configure, map_match_evaluate). Each launches on the context's stream, reads what the frame left and writes only buffers of its own: nothing
// a later frame reads. What they share lives here once: the buffers of a radix sort (PairSort), a result's centroids in
// search-grid order (SearchIndex: result_bounds, then the caller's choice of grid, then build_search_index) and the
// Gauss-Newton loop of a registration (PoseFit, fit_pose). The structs are cm_ctx.hpp's; their buffers are DevBufs
// (cm_devbuf.hpp) that grow on demand and go with the context, so a call here states what it needs and frees nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "cm_align_solve.hpp"
#include "cm_cost_table.hpp"
#include "cm_ctx.hpp"
#include "cm_match_table.hpp"
#include "cm_mcl_beam_table.hpp"
#include "cm_mcl_math.hpp"
#include "cm_search.hpp"

namespace {

// What the grid kernels take of cm_grid_params: inv = 1.0f / cell, the fp32 division of step 1.
CmGridDev grid_dev(const cm_grid_params& q) {
    CmGridDev g;
    g.origin[0] = q.origin[0];
    g.origin[1] = q.origin[1];
    g.inv = 1.0f / q.cell;
    g.nx = q.nx;
    g.ny = q.ny;
    g.z_min = q.z_min;
    g.z_max = q.z_max;
    g.obstacle_height = q.obstacle_height;
    g.min_points = q.min_points;
    return g;
}

}  // namespace

int PairSort::reserve(cm_ctx* c, uint32_t n_slots, const char* what) {
    if (n_slots == 0) return CM_OK;
    const size_t tiles = n_slots / CM_TILE, groups = (tiles + CM_GROUP - 1) / CM_GROUP;
    bool ok = true;
    for (DevBuf<uint32_t>* b : {&keys_a, &keys_b, &vals_a, &vals_b}) ok = ok && b->reserve(n_slots);
    ok = ok && hist.reserve(tiles * CM_RADIX) && grp.reserve(CM_MAX_PASSES * groups * CM_RADIX) && totals.once(CM_RADIX);
    return ok ? CM_OK : fail(c, CM_HIP_ERROR, what);
}

int PoseFit::reserve(cm_ctx* c, uint64_t n, size_t corr_bytes, const char* what_state, const char* what_table) {
    if (!sums.once(CM_ALIGN_SUMS)) return fail(c, CM_HIP_ERROR, what_state);
    const size_t n_blocks = (n + CM_BLOCK - 1) / CM_BLOCK;
    if (!corr.reserve(n * corr_bytes) || !part.reserve(n_blocks * CM_ALIGN_STRIDE)) return fail(c, CM_HIP_ERROR, what_table);
    return CM_OK;
}

// The per-voxel covariance table of the last result into c->cov_entries (cm_kernels_cov.hip). Launches on the context's
// stream, reads what the frame left (descriptor, mask, out_key / out_cnt, cell grid) and writes only the cov buffers and
// `merged`: nothing a later frame reads.
int voxel_cov(cm_ctx* c, const cm_cov_params& q) {
    const uint64_t n_out = c->result.n_out;
    c->cov_have = false;
    if (n_out == 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->cov_entries.reserve(n_out * sizeof(cm_voxel_cov))) return fail(c, CM_HIP_ERROR, "cannot allocate the covariance table");
    const CmFrameDev& f = c->frame;
    const uint32_t nt = f.n_tiles, n_slots = f.n_padded;
    const uint32_t gw = (nt + CM_GROUP - 1) / CM_GROUP * CM_RADIX;
    PairSort& so = c->cov;
    if (const int e = so.reserve(c, n_slots, "cannot allocate the covariance sort's buffers")) return e;
    if (!c->cov_state.once(1) || !c->cov_tile_counts.once(c->cap_tiles) || !c->cov_words.once(2))
        return fail(c, CM_HIP_ERROR, "cannot allocate the covariance sort's state");
    if (!ensure_merged(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the fused cloud's buffer");
    hipStream_t st = c->stream;
    // the kept points in (sensor, point) order, as cm_merged_copy returns them
    frame_on_device(c);
    cmk_merged(st, c->d_frame, c->cov_tile_counts, c->cov_words, c->merged, nt, c->frame_mask);
    // (voxel number, record index) pairs, sorted by voxel number: as many 8-bit passes as the numbers need
    const uint32_t passes = (key_width(n_out) + CM_RADIX_BITS - 1) / CM_RADIX_BITS;
    CmCovGridDev g;
    for (int a = 0; a < 3; ++a) {
        g.inv[a] = f.inv_leaf[a];
        g.min_b[a] = c->cell_min_b[a];
        g.div_b[a] = static_cast<uint32_t>(c->cell_div_b[a]);
    }
    HIP_TRY(c, hipMemsetAsync(so.grp, 0, static_cast<size_t>(passes) * gw * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->cov_words + 1, 0, 4, st));
    cmk_cov_keys(st, c->merged, c->cov_words, g, c->out_key, static_cast<uint32_t>(n_out), passes, c->cov_state, so.keys_a, so.hist,
                 so.grp, nt);
    // ballot ranking whatever the context's probe found: stable by construction, the sums' order depends on it
    radix_sort_pairs(c, c->cov_state, so.pairs(gw), passes, nt, n_slots, false, nullptr, nullptr);
    cmk_cov_reduce(st, c->merged, c->cov_state, so.keys_a, so.vals_a, so.keys_b, so.vals_b, c->out_cnt, static_cast<uint32_t>(n_out),
                   q.min_points, q.eig_mult, c->cov_entries, c->cov_words + 1);
    HIP_TRY(c, hipGetLastError());
    uint32_t err = 0;
    HIP_TRY(c, hipMemcpyAsync(&err, c->cov_words + 1, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (err) return fail(c, CM_INTERNAL, "covariance: a voxel's points did not match its count in the result");
    c->cov_have = true;                              // (what ndt() may reuse)
    c->cov_min_points = q.min_points;
    c->cov_eig_mult = q.eig_mult;
    return CM_OK;
}

namespace {

// The stages a by-product marked (prof_mark) into c->stage_times, as wait_frame does for a frame's.
void collect_stage_times(cm_ctx* c) {
    if (!(c->flags & CM_FLAG_PROFILE)) return;
    cm_stage_times& t = c->stage_times;
    std::memset(&t, 0, sizeof t);
    const size_t n = c->prof_used ? c->prof_used - 1 : 0;
    for (size_t i = 0; i < n && i < CM_MAX_STAGES; ++i) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]);
        std::snprintf(t.name[i], sizeof t.name[i], "%s", c->prof_names[i].c_str());
        t.ms[i] = ms;
        t.n_stages = static_cast<uint32_t>(i + 1);
    }
}

// The stages an iterated by-product marked, one entry per name in order of first appearance, the milliseconds of equally
// named stages added up (collect_stage_times lists every launch; a registration has up to 65 evaluations).
void collect_stage_times_by_name(cm_ctx* c) {
    if (!(c->flags & CM_FLAG_PROFILE)) return;
    cm_stage_times& t = c->stage_times;
    std::memset(&t, 0, sizeof t);
    const size_t n = c->prof_used ? c->prof_used - 1 : 0;
    for (size_t i = 0; i < n; ++i) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]);
        char name[sizeof t.name[0]];
        std::snprintf(name, sizeof name, "%s", c->prof_names[i].c_str());
        uint32_t k = 0;
        while (k < t.n_stages && std::strcmp(t.name[k], name) != 0) ++k;
        if (k == CM_MAX_STAGES) continue;
        if (k == t.n_stages) { std::memcpy(t.name[k], name, sizeof name); ++t.n_stages; }
        t.ms[k] += ms;
    }
}

// How a by-product call closes where it makes one host round trip at its end: the end mark, the launches' errors, at most
// one copy of the call's info words into its page-locked buffer, the wait, the stage times.
int finish_call(cm_ctx* c, void* host = nullptr, const void* dev = nullptr, size_t bytes = 0) {
    prof_mark(c, "end");
    HIP_TRY(c, hipGetLastError());
    if (bytes) HIP_TRY(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    collect_stage_times(c);
    return CM_OK;
}

// A map layer given back: its struct assigned afresh (the buffers go with the old value), its state off. layers_drop_below
// walks the tree of cm_map_layers.hpp, so a configure call names no child.
void layer_drop(cm_ctx* c, int l) {
    switch (l) {
        case LAYER_MAP: c->map = MapLayer{}; break;
        case LAYER_COST: c->cost = CostLayer{}; break;
        case LAYER_PLAN: c->plan_layer = PlanLayer{}; break;
        case LAYER_TRAJ: c->traj = TrajLayer{}; break;
        case LAYER_FRONT: c->front = FrontLayer{}; break;
        case LAYER_MATCH: c->match = MatchLayer{}; break;
        case LAYER_SEARCH: c->msearch = SearchLayer{}; break;
        case LAYER_MCL: c->mcl = MclLayer{}; break;
        case LAYER_CAST: c->cast = CastLayer{}; break;
    }
    layer_reset(c->layers, l);
}
void layers_drop_below(cm_ctx* c, int node) {
    for (int l = LAYER_COUNT; l-- > 0;)
        if (layer_below(l, node)) layer_drop(c, l);
}

// The bounds of the last result's centroids (k_cl_bounds into the six `words`, one host round trip): what a search grid is
// laid over, and whose midpoint is a registration's pivot. The result holds at least one record.
int result_bounds(cm_ctx* c, uint32_t* words, float mn[3], float mx[3]) {
    hipStream_t st = c->stream;
    prof_mark(c, "k_cl_bounds");
    HIP_TRY(c, hipMemsetAsync(words, 0xFF, 12, st));
    HIP_TRY(c, hipMemsetAsync(words + 3, 0, 12, st));
    cmk_cl_bounds(st, c->out, static_cast<uint32_t>(c->result.n_out), words);
    uint32_t img[6];
    HIP_TRY(c, hipMemcpyAsync(img, words, sizeof img, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) { mn[a] = ord2f(img[a]); mx[a] = ord2f(img[3 + a]); }
    return CM_OK;
}

void bounds_midpoint(const float mn[3], const float mx[3], double pivot[3]) {
    for (int a = 0; a < 3; ++a)
        pivot[a] = static_cast<double>(mn[a]) + (static_cast<double>(mx[a]) - static_cast<double>(mn[a])) * 0.5;
}

// Room in ix for the last result (none for an empty one): n_states state records and the bounds words on the first call, the
// sort's buffers, the points and the aux words grown with the result. what_buffers, what_state: the error texts.
int reserve_search_index(cm_ctx* c, SearchIndex& ix, uint32_t n_states, const char* what_buffers, const char* what_state) {
    const uint32_t n_slots = round_up(static_cast<uint32_t>(c->result.n_out), CM_TILE);
    if (const int e = ix.sort.reserve(c, n_slots, what_buffers)) return e;
    if (!ix.pts.reserve(static_cast<size_t>(n_slots) * 16) || !ix.aux.reserve(static_cast<size_t>(n_slots) * 3))
        return fail(c, CM_HIP_ERROR, what_buffers);
    if (!ix.state.once(n_states) || !ix.bounds.once(6)) return fail(c, CM_HIP_ERROR, what_state);
    return CM_OK;
}

// The last result's centroids into ix in the order of `grid`, which the caller laid over their bounds (mn: the minimum):
// (cell key, result index) sorted by cell key — ballot ranking whatever the context's probe found —, the points gathered in
// that order, the (y,z)-row ranges. ix.grid is then what the search kernels take. what: the error text of a row table that
// cannot grow.
int build_search_index(cm_ctx* c, SearchIndex& ix, const ClusterGrid& grid, const float mn[3], const char* what) {
    const uint32_t n = static_cast<uint32_t>(c->result.n_out);
    const uint32_t n_slots = round_up(n, CM_TILE), nt = n_slots / CM_TILE;
    const uint32_t gw = (nt + CM_GROUP - 1) / CM_GROUP * CM_RADIX;
    if (!ix.rows.reserve(static_cast<size_t>(grid.dims[1]) * grid.dims[2] * 8)) return fail(c, CM_HIP_ERROR, what);
    for (int a = 0; a < 3; ++a) { ix.grid.min[a] = mn[a]; ix.grid.dims[a] = grid.dims[a]; }
    ix.grid.inv = grid.inv;
    hipStream_t st = c->stream;
    PairSort& so = ix.sort;
    const uint32_t passes = (grid.key_bits + CM_RADIX_BITS - 1) / CM_RADIX_BITS;
    HIP_TRY(c, hipMemsetAsync(so.grp, 0, static_cast<size_t>(passes) * gw * 4, st));
    prof_mark(c, "k_cl_keys");
    cmk_cl_keys(st, c->out, n, ix.grid, passes, ix.state, so.keys_a, so.hist, so.grp, nt);
    radix_sort_pairs(c, ix.state, so.pairs(gw), passes, nt, n_slots, false, nullptr, "k_scatter(cells)");
    prof_mark(c, "k_cl_gather");
    cmk_cl_gather(st, c->out, ix.state, so.vals_a, so.vals_b, n, ix.pts, ix.aux, ix.aux + n_slots, ix.aux + 2 * static_cast<size_t>(n_slots));
    prof_mark(c, "cl_rows");
    cmk_sorted_rows(st, nullptr, ix.state, so.keys_a, so.vals_a, so.keys_b, so.vals_b, ix.pts, ix.rows, n_slots, true);
    return CM_OK;
}

}  // namespace

// Euclidean cluster extraction on the last result (cm_kernels_cluster.hip): labels, cluster table and member lists into the
// cl buffers. Reads `out` — what cm_result_copy reads — and out_cnt where the context keeps it. Two host round trips: the
// bounds of the centroids (the search grid is decided on the host, cluster_grid) and the cluster count (the second sort's
// passes, the table's size). Under CM_FLAG_PROFILE the stage times of the call replace the frame's in cm_get_stage_times.
int clusters(cm_ctx* c, const cm_cluster_params& q, bool more_stages) {
    const uint32_t n = static_cast<uint32_t>(c->result.n_out);
    c->box_n = 0;
    c->cl_n_clusters = 0;
    c->cl_n_clustered = 0;
    c->cl_indices = nullptr;
    if (n == 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n_slots = round_up(n, CM_TILE), nt = n_slots / CM_TILE;
    const uint32_t gw = (nt + CM_GROUP - 1) / CM_GROUP * CM_RADIX;
    SearchIndex& ix = c->cl;
    if (const int e = reserve_search_index(c, ix, 2, "cannot allocate the cluster extraction's buffers",
                                           "cannot allocate the cluster extraction's state")) return e;
    if (!c->cl_root.reserve(n_slots) || !c->cl_num.reserve(n_slots) || !c->cl_labels.reserve(n_slots) ||
        !c->cl_tile_sums.reserve(static_cast<size_t>(nt) * 8))
        return fail(c, CM_HIP_ERROR, "cannot allocate the cluster extraction's buffers");
    if (!c->cl_words.once(2)) return fail(c, CM_HIP_ERROR, "cannot allocate the cluster extraction's state");
    hipStream_t st = c->stream;
    uint32_t* const w = c->cl_words;
    c->prof_used = 0;

    // the search grid: over the centroids' own bounds
    float mn[3], mx[3];
    if (const int e = result_bounds(c, ix.bounds, mn, mx)) return e;
    const ClusterGrid grid = cluster_grid(q.tolerance, mn, mx, CM_ROW_TABLE_CAP);
    if (const int e = build_search_index(c, ix, grid, mn, "cannot allocate the cluster extraction's row table")) return e;
    PairSort& so = ix.sort;
    CmFrameState* st_cell = ix.state;
    CmFrameState* st_num = ix.state + 1;
    uint32_t *parent = ix.aux, *size = ix.aux + n_slots, *npts = ix.aux + 2 * static_cast<size_t>(n_slots);

    // connected components, sizes, the roots the size filter keeps
    const float tol2 = q.tolerance * q.tolerance;
    prof_mark(c, "k_cl_hook");
    cmk_cl_hook(st, st_cell, so.keys_a, so.keys_b, ix.pts, ix.rows, n, tol2, parent);
    prof_mark(c, "k_cl_roots");
    cmk_cl_roots(st, parent, (c->flags & CM_FLAG_OCCUPANCY) ? c->out_cnt : nullptr, n, c->cl_root, size, npts);
    prof_mark(c, "k_cl_count");
    cmk_cl_count(st, c->cl_root, size, n, q.min_cluster_size, q.max_cluster_size, c->cl_tile_sums, w, nt);
    HIP_TRY(c, hipGetLastError());
    uint32_t counts[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(counts, w, sizeof counts, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint32_t n_clusters = counts[0];
    if (!c->cl_clusters.reserve(n_clusters * sizeof(cm_cluster))) return fail(c, CM_HIP_ERROR, "cannot allocate the cluster table");

    // numbers, labels, AABB, and the member lists: (cluster number, voxel index) sorted by cluster number, stable
    const uint32_t passes_num = (key_width(n_clusters ? n_clusters : 1u) + CM_RADIX_BITS - 1) / CM_RADIX_BITS;
    prof_mark(c, "k_cl_number");
    cmk_cl_number(st, c->cl_root, size, npts, c->cl_tile_sums, n, q.min_cluster_size, q.max_cluster_size, c->cl_num, c->cl_clusters, nt);
    HIP_TRY(c, hipMemsetAsync(so.grp, 0, static_cast<size_t>(passes_num) * gw * 4, st));
    prof_mark(c, "k_cl_labels");
    cmk_cl_labels(st, c->out, c->cl_root, c->cl_num, n, passes_num, st_num, c->cl_labels, so.keys_a, so.hist, so.grp, c->cl_clusters, nt);
    if (n_clusters) {
        radix_sort_pairs(c, st_num, so.pairs(gw), passes_num, nt, n_slots, false, nullptr, "k_scatter(lists)");
        prof_mark(c, "k_cl_decode");
        cmk_cl_decode(st, c->cl_clusters, n_clusters);
    }
    HIP_TRY(c, hipGetLastError());
    if (!more_stages) {
        prof_mark(c, "end");
        HIP_TRY(c, hipStreamSynchronize(st));
        collect_stage_times(c);
    }
    c->cl_n_clusters = n_clusters;
    c->cl_n_clustered = counts[1];
    c->cl_indices = (passes_num & 1u) ? so.vals_b : so.vals_a;
    return CM_OK;
}

void box_direction_table(uint32_t n_angles, float* cos_sin) {
    const double step = 1.5707963267948966 / static_cast<double>(n_angles);
    for (uint32_t a = 0; a < n_angles; ++a) {
        const double th = static_cast<double>(a) * step;
        cos_sin[2 * a] = static_cast<float>(std::cos(th));
        cos_sin[2 * a + 1] = static_cast<float>(std::sin(th));
    }
}

// Oriented boxes of the last result's clusters (cm_kernels_box.hip; the semantics are in include/cloudmerge.h). The cluster
// call first, its stream left running: no host round trip of its own. k_box_fit takes every cluster, and fits the ones of
// up to box_split members itself; the larger ones it lists, and three launches take them chunk by chunk. The host does not
// know how many were listed: the three grids are sized for the most there can be among n_clustered voxels, and none is
// launched where n_clustered <= box_split. Under CM_FLAG_PROFILE the stage times are the cluster call's, then these.
int cluster_boxes(cm_ctx* c, const cm_box_params& q) {
    if (const int e = clusters(c, q.cluster, true)) return e;
    const uint64_t n_clusters = c->cl_n_clusters, n_clustered = c->cl_n_clustered;
    hipStream_t st = c->stream;
    if (n_clusters == 0) {                           // (an empty result marked nothing)
        if (c->result.n_out) {
            prof_mark(c, "end");
            HIP_TRY(c, hipStreamSynchronize(st));
            collect_stage_times(c);
        }
        return CM_OK;
    }
    if (!c->box_entries.reserve(n_clusters * sizeof(cm_cluster_box))) return fail(c, CM_HIP_ERROR, "cannot allocate the box table");
    if (!c->box_dirs.once(sizeof c->box_dirs_host) || !c->box_words.once(2)) return fail(c, CM_HIP_ERROR, "cannot allocate the box fit's state");
    const uint64_t split = c->box_split;
    const uint64_t max_large = n_clustered / (split + 1u);
    const uint64_t max_chunks = max_large ? n_clustered / CM_BOX_CHUNK + max_large : 0u;
    if (!c->box_list.reserve(max_large * 8) || !c->box_ext.reserve(max_large * CM_BOX_MAX_ANGLES * 16) ||
        !c->box_work.reserve(max_chunks * 8) || !c->box_sums.reserve(max_chunks * CM_BOX_MAX_ANGLES))
        return fail(c, CM_HIP_ERROR, "cannot allocate the box fit's buffers");
    if (c->box_dirs_n != q.n_angles) {
        // (box_dirs_host is read by no copy in flight: every box call ends with the stream at rest)
        box_direction_table(q.n_angles, c->box_dirs_host);
        HIP_TRY(c, hipMemcpyAsync(c->box_dirs, c->box_dirs_host, static_cast<size_t>(q.n_angles) * 8, hipMemcpyHostToDevice, st));
        c->box_dirs_n = q.n_angles;
    }
    const double step = 1.5707963267948966 / static_cast<double>(q.n_angles);
    const uint32_t nk = static_cast<uint32_t>(n_clusters), na = q.n_angles;
    HIP_TRY(c, hipMemsetAsync(c->box_words, 0, 8, st));
    prof_mark(c, "k_box_fit");
    cmk_box_fit(st, c->out, c->cl_clusters, c->cl_indices, nk, c->box_dirs, na, step, q.criterion, q.d_min,
                static_cast<uint32_t>(split), c->box_entries, c->box_words, c->box_list, c->box_work, c->box_ext);
    if (max_large) {
        const uint32_t ml = static_cast<uint32_t>(max_large), mc = static_cast<uint32_t>(max_chunks);
        prof_mark(c, "k_box_extremes");
        cmk_box_extremes(st, c->out, c->cl_clusters, c->cl_indices, c->box_dirs, na, c->box_words, c->box_list, c->box_work, c->box_ext, mc);
        if (q.criterion == CM_BOX_CLOSENESS) {
            prof_mark(c, "k_box_sums");
            cmk_box_sums(st, c->out, c->cl_clusters, c->cl_indices, c->box_dirs, na, q.d_min, c->box_words, c->box_list, c->box_work,
                         c->box_ext, c->box_sums, mc);
        }
        prof_mark(c, "k_box_choose");
        cmk_box_choose(st, c->cl_clusters, c->box_dirs, na, step, q.criterion, c->box_words, c->box_list, c->box_ext, c->box_sums,
                       c->box_entries, ml);
    }
    prof_mark(c, "end");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    collect_stage_times(c);
    c->box_n = n_clusters;
    return CM_OK;
}

// The 2-D grid map of the last frame (cm_kernels_grid.hip; the semantics are in include/cloudmerge.h): nx * ny cm_grid_cell
// records into grid_cells and as many occupancy bytes into grid_image. One clear, one pass over the frame's raw points in
// place (the descriptor in HBM, the keep-mask behind cm_merged_copy, the ground mask behind cm_ground_copy), one pass over the
// cells; no host round trip but the wait at the end. A steady-state call allocates nothing. Under CM_FLAG_PROFILE the stage
// times of the call replace the frame's in cm_get_stage_times.
int grid_map(cm_ctx* c, const cm_grid_params& q, bool more_stages) {
    c->grid_have = c->ray_have = false;           // (a ray table goes with the grid it was cast over)
    const uint64_t n_cells = static_cast<uint64_t>(q.nx) * q.ny;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->grid_cells.reserve(n_cells * sizeof(cm_grid_cell)) || !c->grid_image.reserve(n_cells))
        return fail(c, CM_HIP_ERROR, "cannot allocate the grid map");
    const CmGridDev g = grid_dev(q);
    hipStream_t st = c->stream;
    c->prof_used = 0;
    prof_mark(c, "grid_clear");
    HIP_TRY(c, hipMemsetAsync(c->grid_cells, 0, n_cells * sizeof(cm_grid_cell), st));
    prof_mark(c, "k_grid_bin");
    // (an empty frame has no tiles and, on a fresh context, no descriptor in HBM: nothing is launched)
    frame_on_device(c);
    cmk_grid_bin(st, c->d_frame, g, c->frame_mask, c->frame_had_ground ? c->gmask : nullptr, c->grid_cells, c->frame.n_tiles);
    prof_mark(c, "k_grid_finish");
    cmk_grid_finish(st, c->grid_cells, c->grid_image, static_cast<uint32_t>(n_cells), q.obstacle_height, q.min_points);
    HIP_TRY(c, hipGetLastError());
    c->grid_n = n_cells;
    if (more_stages) return CM_OK;                // (grid_rays: it waits, and says then that the grid is there)
    prof_mark(c, "end");
    HIP_TRY(c, hipStreamSynchronize(st));
    collect_stage_times(c);
    c->grid_have = true;
    return CM_OK;
}

// Free-space ray casting over the grid map of the last frame (cm_kernels_rays.hip; the semantics are in include/cloudmerge.h):
// the grid map at q as grid_map leaves it, then nx * ny cm_grid_ray_cell records into ray_cells and as many cleared occupancy
// bytes into ray_image. The origin cells are the grid's step 1 applied on the host to the translations the frame was built
// with (frame_origin). One clear, a second pass over the frame's raw points in place (the end cells' bitmaps), the walk, one
// pass over the cells; no host round trip but the wait at the end. A steady-state call allocates nothing.
int grid_rays(cm_ctx* c, const cm_grid_params& q, const cm_ray_params& r) {
    const uint64_t n_cells = static_cast<uint64_t>(q.nx) * q.ny;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->ray_bits.reserve(static_cast<size_t>(c->max_sensors) * ((n_cells + 31) / 32)) ||
        !c->ray_cells.reserve(n_cells * sizeof(cm_grid_ray_cell)) || !c->ray_image.reserve(n_cells))
        return fail(c, CM_HIP_ERROR, "cannot allocate the ray tables");
    if (const int e = grid_map(c, q, true)) return e;
    const uint32_t words = static_cast<uint32_t>((n_cells + 31) / 32);
    const uint32_t n_sensors = c->frame.n_tiles ? c->frame.n_sensors : 0u;
    const CmGridDev g = grid_dev(q);
    CmRayDev rd;
    std::memset(&rd, 0, sizeof rd);
    rd.nx = q.nx;
    rd.max_range = r.max_range_cells;
    for (uint32_t s = 0; s < n_sensors; ++s) {
        // step 1 of the grid on the host: the same subtraction, product and floorf, each rounded to fp32 on its own
        const float cx = std::floor(static_cast<float>(static_cast<float>(c->frame_origin[s][0] - g.origin[0]) * g.inv));
        const float cy = std::floor(static_cast<float>(static_cast<float>(c->frame_origin[s][1] - g.origin[1]) * g.inv));
        if (!(cx >= 0.0f && cx < static_cast<float>(q.nx) && cy >= 0.0f && cy < static_cast<float>(q.ny))) continue;
        rd.ox[s] = static_cast<int>(cx);
        rd.oy[s] = static_cast<int>(cy);
        rd.has[s] = 1u;
    }
    hipStream_t st = c->stream;
    prof_mark(c, "ray_clear");
    if (n_sensors) HIP_TRY(c, hipMemsetAsync(c->ray_bits, 0, static_cast<size_t>(n_sensors) * words * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->ray_cells, 0, n_cells * sizeof(cm_grid_ray_cell), st));
    prof_mark(c, "k_ray_mark");
    frame_on_device(c);
    cmk_ray_mark(st, c->d_frame, g, c->frame_mask, c->frame_had_ground ? c->gmask : nullptr, c->ray_bits, words, c->frame.n_tiles);
    prof_mark(c, "k_ray_cast");
    cmk_ray_cast(st, c->ray_bits, words, rd, n_sensors, c->ray_cells);
    prof_mark(c, "k_ray_finish");
    cmk_ray_finish(st, c->grid_cells, c->ray_cells, c->ray_image, static_cast<uint32_t>(n_cells), r.min_pass);
    if (const int e = finish_call(c)) return e;
    c->grid_have = true;
    c->ray_n = n_cells;
    c->ray_have = true;
    return CM_OK;
}

namespace {

// Step 1 of the occupancy map on the host, one axis: floorf(w * inv), the product rounded to fp32 on its own; false where the
// cell does not exist.
bool map_world_axis(float w, float inv, int* g) {
    const float c = std::floor(static_cast<float>(w * inv));
    if (!(c > -1073741824.0f && c < 1073741824.0f)) return false;
    *g = static_cast<int>(c);
    return true;
}

// xf_row on the host: ((m0 x + m1 y) + m2 z) + m3, every operation rounded to fp32 on its own.
float map_row(const float* m, const float* t) {
    const float a = static_cast<float>(static_cast<float>(m[0] * t[0]) + static_cast<float>(m[1] * t[1]));
    return static_cast<float>(static_cast<float>(a + static_cast<float>(m[2] * t[2])) + m[3]);
}

}  // namespace

// The occupancy map's memory, all of it: two state tables, the image, the bitmaps of every sensor the context can hold and
// the scratch ray table, then cleared. nullptr gives it back.
int map_configure(cm_ctx* c, const cm_map_params* q) {
    HIP_TRY(c, hipSetDevice(c->device));
    layers_drop_below(c, LAYER_MAP);                   // the layers go with the map they were sized for
    if (!q) {
        layer_drop(c, LAYER_MAP);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_MAP);
    c->map.serial = 0;
    c->map.cur = 0;
    std::memset(&c->map.info, 0, sizeof c->map.info);
    const uint64_t n_cells = static_cast<uint64_t>(q->nx) * q->ny;
    const size_t words = (n_cells + 31) / 32;
    if (!c->map.state[0].reserve(n_cells * sizeof(cm_map_cell)) || !c->map.state[1].reserve(n_cells * sizeof(cm_map_cell)) ||
        !c->map.image.reserve(n_cells) || !c->map.bits.reserve(2 * static_cast<size_t>(c->max_sensors) * words) ||
        !c->map.rays.reserve(n_cells * sizeof(cm_grid_ray_cell)))
        return fail(c, CM_HIP_ERROR, "cannot allocate the occupancy map");
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->map.state[0], 0, n_cells * sizeof(cm_map_cell), st));
    HIP_TRY(c, hipMemsetAsync(c->map.image, 0xFF, n_cells, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->map.params = *q;
    c->map.info.nx = q->nx;
    c->map.info.ny = q->ny;
    c->layers[LAYER_MAP].on = true;
    return CM_OK;
}

bool map_vehicle_cell(const cm_ctx* c, const float pose[12], int v[2]) {
    const float inv = 1.0f / c->map.params.cell;
    return map_world_axis(pose[3], inv, &v[0]) && map_world_axis(pose[7], inv, &v[1]);
}

bool map_window_cell(const cm_ctx* c, float x, float y, uint32_t cell[2]) {
    const float inv = 1.0f / c->map.params.cell;
    int g[2];
    if (!map_world_axis(x, inv, &g[0]) || !map_world_axis(y, inv, &g[1])) return false;
    const int64_t ix = static_cast<int64_t>(g[0]) - c->map.info.anchor[0], iy = static_cast<int64_t>(g[1]) - c->map.info.anchor[1];
    if (ix < 0 || ix >= static_cast<int64_t>(c->map.info.nx) || iy < 0 || iy >= static_cast<int64_t>(c->map.info.ny)) return false;
    cell[0] = static_cast<uint32_t>(ix);
    cell[1] = static_cast<uint32_t>(iy);
    return true;
}

// The last frame into the occupancy map (cm_kernels_map.hip; the semantics are in include/cloudmerge.h). The window's anchor
// and the sensors' origin cells are step 1 on the host (fp32, explicit casts, as grid_rays does). One clear of the bitmaps
// and the scratch ray table, a pass over the frame's raw points in place (the E and H bitmaps), k_ray_cast unchanged on the
// E bitmaps, one pass over the cells that scrolls, updates and writes the image into the other state buffer; no host round
// trip but the wait at the end, and no allocation: cm_map_configure made them all.
int map_integrate(cm_ctx* c, const float pose[12], const int v[2]) {
    const cm_map_params& q = c->map.params;
    const uint64_t n_cells = static_cast<uint64_t>(q.nx) * q.ny;
    const uint32_t words = static_cast<uint32_t>((n_cells + 31) / 32);
    const uint32_t n_sensors = c->frame.n_tiles ? c->frame.n_sensors : 0u;
    HIP_TRY(c, hipSetDevice(c->device));
    CmMapDev g;
    std::memcpy(g.p, pose, sizeof g.p);
    g.inv = 1.0f / q.cell;
    g.ax = v[0] - static_cast<int>(q.nx / 2);          // (|v| < 2^30, nx / 2 <= 2^21: no overflow)
    g.ay = v[1] - static_cast<int>(q.ny / 2);
    g.nx = q.nx;
    g.ny = q.ny;
    g.z_min = q.z_min;
    g.z_max = q.z_max;
    CmRayDev rd;
    std::memset(&rd, 0, sizeof rd);
    rd.nx = q.nx;
    rd.max_range = q.max_range_cells;
    uint32_t cast = 0;
    for (uint32_t s = 0; s < n_sensors; ++s) {
        int o[2];
        if (!map_world_axis(map_row(pose, c->frame_origin[s]), g.inv, &o[0]) ||
            !map_world_axis(map_row(pose + 4, c->frame_origin[s]), g.inv, &o[1])) continue;
        const int64_t ix = static_cast<int64_t>(o[0]) - g.ax, iy = static_cast<int64_t>(o[1]) - g.ay;
        if (ix < 0 || ix >= static_cast<int64_t>(q.nx) || iy < 0 || iy >= static_cast<int64_t>(q.ny)) continue;
        rd.ox[s] = static_cast<int>(ix);
        rd.oy[s] = static_cast<int>(iy);
        rd.has[s] = 1u;
        cast |= 1u << s;
    }
    CmMapUpdateDev u;
    u.nx = q.nx;
    u.ny = q.ny;
    // the shift anchor_new - anchor_old: a window that shares no cell with the old one (or has no old one) carries nothing
    const int64_t sx = static_cast<int64_t>(g.ax) - c->map.info.anchor[0], sy = static_cast<int64_t>(g.ay) - c->map.info.anchor[1];
    const bool carry = c->map.info.n_frames != 0 && sx > -static_cast<int64_t>(q.nx) && sx < static_cast<int64_t>(q.nx) &&
                       sy > -static_cast<int64_t>(q.ny) && sy < static_cast<int64_t>(q.ny);
    u.carry = carry ? 1u : 0u;
    u.sx = carry ? static_cast<int32_t>(sx) : 0;
    u.sy = carry ? static_cast<int32_t>(sy) : 0;
    u.n_sensors = n_sensors;
    u.l_hit = q.l_hit;
    u.l_miss = q.l_miss;
    u.l_min = q.l_min;
    u.l_max = q.l_max;
    u.l_free = q.l_free;
    u.l_occ = q.l_occ;
    hipStream_t st = c->stream;
    c->prof_used = 0;
    prof_mark(c, "map_clear");
    if (n_sensors) HIP_TRY(c, hipMemsetAsync(c->map.bits, 0, 2 * static_cast<size_t>(n_sensors) * words * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->map.rays, 0, n_cells * sizeof(cm_grid_ray_cell), st));
    prof_mark(c, "k_map_mark");
    frame_on_device(c);
    cmk_map_mark(st, c->d_frame, g, c->frame_mask, c->frame_had_ground ? c->gmask : nullptr, c->map.bits, words, n_sensors, c->frame.n_tiles);
    prof_mark(c, "k_ray_cast");
    cmk_ray_cast(st, c->map.bits, words, rd, n_sensors, c->map.rays);
    prof_mark(c, "k_map_update");
    cmk_map_update(st, c->map.state[c->map.cur], c->map.state[c->map.cur ^ 1], c->map.rays, c->map.bits, words, u, c->map.image);
    if (const int e = finish_call(c)) return e;
    c->map.cur ^= 1;
    c->map.info.anchor[0] = g.ax;
    c->map.info.anchor[1] = g.ay;
    ++c->map.info.n_frames;
    c->map.info.sensors_cast = cast;
    c->map.serial = c->frame_serial;
    layers_mark_below(c->layers, LAYER_MAP, SINCE_INTEGRATE);      // every layer's tables are those of the image before this call
    return CM_OK;
}

// The cost layer's memory, all of it: the two tables, the column pass's obstacle words and carries, the cost table, which is
// built here (cm_cost_table.hpp) and uploaded. nullptr gives it back. The tables are stale until the first update.
int map_cost_configure(cm_ctx* c, const cm_cost_params* q, uint32_t R) {
    HIP_TRY(c, hipSetDevice(c->device));
    layers_drop_below(c, LAYER_COST);                  // the layers that read the cost layer go with it
    if (!q) {
        layer_drop(c, LAYER_COST);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_COST);
    const uint64_t n_cells = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    const size_t words = static_cast<size_t>((c->map.info.ny + CM_COST_ROWS - 1) / CM_COST_ROWS) * c->map.info.nx;
    const size_t n_lut = static_cast<size_t>(R) * R + 1;
    if (!c->cost.cells.reserve(n_cells) || !c->cost.dist2.reserve(n_cells) || !c->cost.masks.reserve(2 * words) || !c->cost.lut.reserve(n_lut))
        return fail(c, CM_HIP_ERROR, "cannot allocate the cost layer");
    c->cost.lut_host.assign(n_lut, 0);
    cm_cost_table(c->map.params.cell, q->inscribed_radius, q->inflation_radius, q->cost_scaling, R, c->cost.lut_host.data());
    HIP_TRY(c, hipMemcpyAsync(c->cost.lut, c->cost.lut_host.data(), n_lut, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->cost.params = *q;
    c->cost.radius = R;
    c->layers[LAYER_COST].on = true;
    return CM_OK;
}

// dist2 and cost of the map's current image (cm_kernels_cost.hip; the semantics are in include/cloudmerge.h): the obstacle
// words of every column, the carries between their blocks, then one pass over the rows that writes both tables. No host
// round trip but the wait at the end, and no allocation: cm_map_cost_configure made them all.
int map_cost_update(cm_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    CmCostDev g;
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.r2 = c->cost.radius * c->cost.radius;
    g.inflate_unknown = (c->cost.params.flags & CM_COST_INFLATE_UNKNOWN) ? 1u : 0u;
    uint32_t* masks = c->cost.masks;
    uint32_t* carry = masks + static_cast<size_t>((g.ny + CM_COST_ROWS - 1) / CM_COST_ROWS) * g.nx;
    hipStream_t st = c->stream;
    c->prof_used = 0;
    prof_mark(c, "k_cost_colmask");
    cmk_cost_colmask(st, c->map.image, g, masks);
    prof_mark(c, "k_cost_colcarry");
    cmk_cost_colcarry(st, masks, g, carry);
    prof_mark(c, "k_cost_rows");
    cmk_cost_rows(st, c->map.image, masks, carry, c->cost.lut, g, c->cost.dist2, c->cost.cells);
    if (const int e = finish_call(c)) return e;
    layer_mark_fresh(c->layers, LAYER_COST, c->frame_serial);
    layers_mark_below(c->layers, LAYER_COST, "the last cm_map_cost_update");
    c->cast.steps_fresh = false;                       // (the next evaluate rebuilds its skip table from the new dist2)
    c->mcl.beam_steps_fresh = false;                   // (and so does the next update under the beam model)
    return CM_OK;
}

// The plan layer's memory, all of it: the potential, the sweep counters and the two tile flag tables, the path buffer and
// the page-locked words the host reads counters and a path's head from. nullptr gives it back. pot is stale until the first
// update.
int map_plan_configure(cm_ctx* c, const cm_plan_params* q) {
    HIP_TRY(c, hipSetDevice(c->device));
    layers_drop_below(c, LAYER_PLAN);                  // the two layers that read the potential go with it
    if (!q) {
        layer_drop(c, LAYER_PLAN);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_PLAN);
    std::memset(&c->plan_layer.info, 0, sizeof c->plan_layer.info);
    const uint64_t n_cells = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    const size_t n_tiles = static_cast<size_t>((c->map.info.nx + CM_PLAN_TILE - 1) / CM_PLAN_TILE) * ((c->map.info.ny + CM_PLAN_TILE - 1) / CM_PLAN_TILE);
    if (!c->plan_layer.pot.reserve(n_cells) || !c->plan_layer.words.reserve(CM_PLAN_BATCH + 2 * n_tiles) ||
        !c->plan_layer.path.reserve(CM_PLAN_PATH_HEAD + static_cast<size_t>(q->max_path_cells)) || !c->plan_layer.host.reserve(std::max(CM_PLAN_BATCH, CM_PLAN_PATH_HEAD)))
        return fail(c, CM_HIP_ERROR, "cannot allocate the plan layer");
    c->plan_layer.params = *q;
    c->layers[LAYER_PLAN].on = true;
    return CM_OK;
}

namespace {

CmPlanDev plan_dev(const cm_ctx* c, const uint32_t goal[2]) {
    CmPlanDev g;
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.tiles_x = (g.nx + CM_PLAN_TILE - 1) / CM_PLAN_TILE;
    g.tiles_y = (g.ny + CM_PLAN_TILE - 1) / CM_PLAN_TILE;
    g.goal = goal[0] + goal[1] * g.nx;
    g.neutral = c->plan_layer.params.neutral;
    g.factor_q8 = c->plan_layer.params.cost_factor_q8;
    g.allow_unknown = (c->plan_layer.params.flags & CM_PLAN_ALLOW_UNKNOWN) ? 1u : 0u;
    return g;
}

}  // namespace

// pot of the cost layer's current table for one goal (cm_kernels_plan.hip; the semantics are in include/cloudmerge.h): the
// fill, then sweeps over the dirty tiles until one reports that no tile changed. The sweeps go out CM_PLAN_BATCH at a time,
// each with a counter of its own, and the host reads the batch's counters once: a sweep with no dirty tile costs a launch of
// workgroups that leave at once, a read per sweep a round trip. The two flag tables swap roles per sweep. Every sweep but the
// last fixes the final word of at least one more cell, so nx * ny sweeps suffice; reaching that bound is CM_INTERNAL. No
// allocation: cm_map_plan_configure made them all.
int map_plan_update(cm_ctx* c, const uint32_t goal[2]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const CmPlanDev g = plan_dev(c, goal);
    const size_t n_tiles = static_cast<size_t>(g.tiles_x) * g.tiles_y;
    const uint64_t bound = static_cast<uint64_t>(g.nx) * g.ny;
    uint32_t* counters = c->plan_layer.words;
    uint32_t* flags = counters + CM_PLAN_BATCH;
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_PLAN);          // (until the fixed point is reached below)
    layers_mark_below(c->layers, LAYER_PLAN, "the last cm_map_plan_update");
    c->prof_used = 0;
    prof_mark(c, "k_plan_init");
    cmk_plan_init(st, g, c->plan_layer.pot, flags);
    prof_mark(c, "k_plan_sweep");
    uint64_t launched = 0, n_sweeps = 0;
    while (!n_sweeps && launched < bound) {
        const uint32_t batch = static_cast<uint32_t>(std::min<uint64_t>(CM_PLAN_BATCH, bound - launched));
        HIP_TRY(c, hipMemsetAsync(counters, 0, CM_PLAN_BATCH * sizeof(uint32_t), st));
        for (uint32_t b = 0; b < batch; ++b) {
            const size_t cur = static_cast<size_t>((launched + b) & 1u) * n_tiles;
            cmk_plan_sweep(st, c->cost.cells, g, c->plan_layer.pot, flags + cur, flags + (n_tiles - cur), counters + b);
        }
        HIP_TRY(c, hipMemcpyAsync(c->plan_layer.host, counters, batch * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        for (uint32_t b = 0; b < batch && !n_sweeps; ++b)
            if (c->plan_layer.host[b] == 0u) n_sweeps = launched + b + 1;
        launched += batch;
    }
    prof_mark(c, "end");
    HIP_TRY(c, hipGetLastError());
    if (c->flags & CM_FLAG_PROFILE) HIP_TRY(c, hipStreamSynchronize(st));     // (the end mark only: the last batch was waited for)
    collect_stage_times(c);
    if (!n_sweeps) return fail(c, CM_INTERNAL, "the sweeps did not reach the fixed point within nx * ny launches");
    c->plan_layer.info.goal[0] = goal[0];
    c->plan_layer.info.goal[1] = goal[1];
    c->plan_layer.info.n_sweeps = static_cast<uint32_t>(n_sweeps);
    layer_mark_fresh(c->layers, LAYER_PLAN, c->frame_serial);
    return CM_OK;
}

// The walk of step 6 from the start's window cell into plan_path, and its head to the host: one launch, one copy of the head
// and one wait here; cm_map_plan_path then copies the n_cells words the head announces and waits a second time.
int map_plan_path(cm_ctx* c, const uint32_t start[2], uint32_t head[4]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const CmPlanDev g = plan_dev(c, c->plan_layer.info.goal);
    hipStream_t st = c->stream;
    c->prof_used = 0;
    prof_mark(c, "k_plan_path");
    cmk_plan_path(st, c->cost.cells, c->plan_layer.pot, g, start[0] + start[1] * g.nx, c->plan_layer.params.max_path_cells, c->plan_layer.path);
    if (const int e = finish_call(c, c->plan_layer.host, c->plan_layer.path, CM_PLAN_PATH_HEAD * sizeof(uint32_t))) return e;
    std::memcpy(head, c->plan_layer.host, CM_PLAN_PATH_HEAD * sizeof(uint32_t));
    if (head[1] == CM_PLAN_PATH_BROKEN_DEV) return fail(c, CM_INTERNAL, "the potential is not a fixed point: a reachable cell has no step");
    return CM_OK;
}

// The frontier layer's memory, all of it: the labels, a size word per cell with the scan's counts and the info words behind
// them, the table with its box scratch, and the page-locked words the host reads the info from. nullptr gives it back. The
// layer is stale until the first update.
int map_frontier_configure(cm_ctx* c, const cm_frontier_params* q) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_FRONT);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_FRONT);
    std::memset(&c->front.info, 0, sizeof c->front.info);
    const uint64_t n_cells = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    const size_t n_blocks = static_cast<size_t>((n_cells + CM_FRONT_BLOCK - 1) / CM_FRONT_BLOCK);
    if (!c->front.labels.reserve(n_cells) || !c->front.words.reserve(n_cells + n_blocks + CM_FRONT_INFO_WORDS) ||
        !c->front.table.reserve(q->max_frontiers) || !c->front.box.reserve(4 * static_cast<size_t>(q->max_frontiers)) ||
        !c->front.host.reserve(CM_FRONT_INFO_WORDS))
        return fail(c, CM_HIP_ERROR, "cannot allocate the frontier layer");
    c->front.params = *q;
    c->layers[LAYER_FRONT].on = true;
    return CM_OK;
}

// Labels, table and info of the current image, cost table and pot (cm_kernels_front.hip; the semantics are in
// include/cloudmerge.h): eight launches in a fixed order behind one clear of the info words, one copy of those words and one
// wait. No loop on the host, and no allocation: cm_map_frontier_configure made them all.
int map_frontier_update(cm_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_frontier_params& q = c->front.params;
    const uint64_t n_cells = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    CmFrontDev g;
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.tiles_x = (g.nx + CM_FRONT_TILE - 1) / CM_FRONT_TILE;
    g.tiles_y = (g.ny + CM_FRONT_TILE - 1) / CM_FRONT_TILE;
    g.n_blocks = static_cast<uint32_t>((n_cells + CM_FRONT_BLOCK - 1) / CM_FRONT_BLOCK);
    g.min_cells = q.min_cells;
    g.max_frontiers = q.max_frontiers;
    g.max_cost = q.max_cost;
    g.pot_scale = q.pot_scale;
    g.gain_scale = q.gain_scale;
    uint32_t* labels = c->front.labels;
    uint32_t* size = c->front.words;
    uint32_t* counts = size + n_cells;
    uint32_t* info = counts + g.n_blocks;
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_FRONT);
    c->prof_used = 0;
    HIP_TRY(c, hipMemsetAsync(info, 0, CM_FRONT_INFO_WORDS * sizeof(uint32_t), st));
    prof_mark(c, "k_front_local");
    cmk_front_local(st, c->map.image, c->cost.cells, g, labels, size, info);
    prof_mark(c, "k_front_merge");
    cmk_front_merge(st, g, labels);
    prof_mark(c, "k_front_flatten");
    cmk_front_flatten(st, g, labels, size);
    prof_mark(c, "k_front_count");
    cmk_front_count(st, g, labels, size, counts, info);
    prof_mark(c, "k_front_scan");
    cmk_front_scan(st, g, counts, info);
    prof_mark(c, "k_front_number");
    cmk_front_number(st, g, labels, size, counts, c->front.table, c->front.box);
    prof_mark(c, "k_front_table");
    cmk_front_table(st, g, c->plan_layer.pot, labels, size, c->front.table, c->front.box);
    prof_mark(c, "k_front_best");
    cmk_front_best(st, g, c->front.table, c->front.box, info);
    if (const int e = finish_call(c, c->front.host, info, CM_FRONT_INFO_WORDS * sizeof(uint32_t))) return e;
    const uint32_t* h = c->front.host;
    c->front.info.n_frontier_cells = h[0];
    c->front.info.n_components = h[1];
    c->front.info.n_frontiers = h[2];
    c->front.info.n_written = h[3];
    c->front.info.best = h[4];
    c->front.info._pad = 0u;
    c->front.info.best_score = static_cast<int64_t>(static_cast<uint64_t>(h[6]) | (static_cast<uint64_t>(h[7]) << 32));
    layer_mark_fresh(c->layers, LAYER_FRONT, c->frame_serial);
    return CM_OK;
}

// Step 2 of the rollout layer: CM_TRAJ_HEADINGS (cos, sin) pairs as box_direction_table builds its own, with the four axes
// set exactly. Built by the first caller and kept.
const float* traj_direction_table() {
    static const std::vector<float> table = [] {
        std::vector<float> t(2 * CM_TRAJ_HEADINGS);
        const double step = 6.283185307179586 / 4096.0;
        for (uint32_t a = 0; a < CM_TRAJ_HEADINGS; ++a) {
            const double th = static_cast<double>(a) * step;
            t[2 * a] = static_cast<float>(std::cos(th));
            t[2 * a + 1] = static_cast<float>(std::sin(th));
        }
        const float axes[4][2] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}, {0.0f, -1.0f}};
        for (uint32_t k = 0; k < 4; ++k) {
            t[2 * (k * 1024u)] = axes[k][0];
            t[2 * (k * 1024u) + 1] = axes[k][1];
        }
        return t;
    }();
    return table.data();
}

// Step 1's samples: lo + (float)i * ((hi - lo) / (float)(n - 1)), every operation rounded to fp32 on its own.
void traj_samples(float lo, float hi, uint32_t n, float* out) {
    out[0] = lo;
    if (n == 1) return;
    const float step = static_cast<float>(static_cast<float>(hi - lo) / static_cast<float>(n - 1u));
    for (uint32_t i = 1; i < n; ++i) out[i] = static_cast<float>(lo + static_cast<float>(static_cast<float>(i) * step));
}

// The rollout layer's memory, all of it: the scores, the info words and the two sample tables, the heading table and the
// footprint (both uploaded here), the page-locked words an evaluate uploads from and reads back into. nullptr gives it back.
// The scores are stale until the first evaluate.
int map_traj_configure(cm_ctx* c, const cm_traj_params* q, const float* foot_xy, uint32_t n_foot) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_TRAJ);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_TRAJ);
    std::memset(&c->traj.info, 0, sizeof c->traj.info);
    const size_t n = static_cast<size_t>(q->nv) * q->nw, n_tab = static_cast<size_t>(q->nv) + q->nw;
    // (the page-locked words also stage the footprint for its upload below)
    if (!c->traj.scores.reserve(n) || !c->traj.words.reserve(CM_TRAJ_INFO_WORDS + n_tab) || !c->traj.consts.reserve(2 * CM_TRAJ_HEADINGS + 2 * static_cast<size_t>(n_foot)) ||
        !c->traj.host.reserve(CM_TRAJ_INFO_WORDS + std::max(n_tab, 2 * static_cast<size_t>(n_foot))))
        return fail(c, CM_HIP_ERROR, "cannot allocate the rollout layer");
    c->traj.v.assign(q->nv, 0.0f);
    c->traj.w.assign(q->nw, 0.0f);
    std::memcpy(c->traj.host + CM_TRAJ_INFO_WORDS, foot_xy, 2 * static_cast<size_t>(n_foot) * sizeof(float));
    HIP_TRY(c, hipMemcpyAsync(c->traj.consts, traj_direction_table(), 2 * CM_TRAJ_HEADINGS * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->traj.consts + 2 * CM_TRAJ_HEADINGS, c->traj.host + CM_TRAJ_INFO_WORDS, 2 * static_cast<size_t>(n_foot) * sizeof(float),
                              hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->traj.params = *q;
    c->traj.n_foot = n_foot;
    c->layers[LAYER_TRAJ].on = true;
    return CM_OK;
}

// The scores of every sample of the window from the start's window cell (cm_kernels_traj.hip; the semantics are in
// include/cloudmerge.h). Step 1 on the host: the samples, the step lengths and the heading increments, written into the
// page-locked words. One upload, two launches, one copy of the info words back and one wait; no allocation:
// cm_map_traj_configure made them all.
int map_traj_evaluate(cm_ctx* c, const cm_traj_window& w, const uint32_t start[2]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_traj_params& q = c->traj.params;
    const double K = 4294967296.0 / 6.283185307179586;
    CmTrajDev g;
    g.x = w.x;
    g.y = w.y;
    g.inv = 1.0f / c->map.params.cell;
    g.ax = c->map.info.anchor[0];
    g.ay = c->map.info.anchor[1];
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.h0 = static_cast<uint32_t>(static_cast<int64_t>(std::rint(static_cast<double>(w.yaw) * K)));
    g.nv = q.nv;
    g.nw = q.nw;
    g.n_steps = q.n_steps;
    g.n_foot = c->traj.n_foot;
    g.occ_scale = q.occ_scale;
    g.goal_scale = q.goal_scale;
    g.allow_unknown = (q.flags & CM_TRAJ_ALLOW_UNKNOWN) ? 1u : 0u;
    uint32_t* const up = c->traj.host + CM_TRAJ_INFO_WORDS;
    for (uint32_t i = 0; i < q.nv; ++i) {
        const float s = static_cast<float>(c->traj.v[i] * w.dt);
        std::memcpy(up + i, &s, sizeof s);
    }
    for (uint32_t j = 0; j < q.nw; ++j)
        up[q.nv + j] = static_cast<uint32_t>(static_cast<int64_t>(std::rint((static_cast<double>(c->traj.w[j]) * static_cast<double>(w.dt)) * K)));
    uint32_t* const info = c->traj.words;
    uint32_t* const tab = info + CM_TRAJ_INFO_WORDS;
    const uint32_t n = q.nv * q.nw;
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_TRAJ);
    c->prof_used = 0;
    HIP_TRY(c, hipMemcpyAsync(tab, up, (static_cast<size_t>(q.nv) + q.nw) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    prof_mark(c, "k_traj_roll");
    cmk_traj_roll(st, c->cost.cells, c->plan_layer.pot, g, reinterpret_cast<const float*>(tab), tab + q.nv, c->traj.consts, c->traj.consts + 2 * CM_TRAJ_HEADINGS,
                  c->traj.scores);
    prof_mark(c, "k_traj_best");
    cmk_traj_best(st, c->traj.scores, n, info);
    if (const int e = finish_call(c, c->traj.host, info, CM_TRAJ_INFO_WORDS * sizeof(uint32_t))) return e;
    const uint32_t best = c->traj.host[0];
    if (best != CM_TRAJ_NONE && best >= n) return fail(c, CM_INTERNAL, "the best entry lies outside the table");
    c->traj.info.best = best;
    c->traj.info.n_valid = c->traj.host[1];
    c->traj.info.best_v = best == CM_TRAJ_NONE ? 0.0f : c->traj.v[best / q.nw];
    c->traj.info.best_w = best == CM_TRAJ_NONE ? 0.0f : c->traj.w[best % q.nw];
    c->traj.info.start[0] = start[0];
    c->traj.info.start[1] = start[1];
    layer_mark_fresh(c->layers, LAYER_TRAJ, c->frame_serial);
    return CM_OK;
}

// The matching layer's memory, all of it: the field with the table behind it (built here, cm_match_table.hpp, and uploaded),
// one bitmap per angle candidate, the volume with the info words behind it, the candidates' matrices and the page-locked words
// an evaluate uploads from and reads back into. nullptr gives it back. Volume and result are stale until the first evaluate.
int map_match_configure(cm_ctx* c, const cm_match_params* q, uint32_t R) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_MATCH);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_MATCH);
    std::memset(&c->match.result, 0, sizeof c->match.result);
    const size_t n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny, words = (n_cells + 31) / 32;
    const size_t n_k = 2 * static_cast<size_t>(q->n_a) + 1, n_vol = n_k * (2 * static_cast<size_t>(q->wx) + 1) * (2 * static_cast<size_t>(q->wy) + 1);
    const size_t n_lut = static_cast<size_t>(R) * R + 1;
    if (!c->match.field.reserve(n_cells + n_lut) || !c->match.bits.reserve(n_k * words) || !c->match.vol.reserve(n_vol + CM_MATCH_INFO_WORDS) ||
        !c->match.q.reserve(6 * n_k) || !c->match.host.reserve(CM_MATCH_INFO_WORDS + 6 * n_k))
        return fail(c, CM_HIP_ERROR, "cannot allocate the matching layer");
    c->match.lut_host.assign(n_lut, 0);
    cm_match_table_build(c->map.params.cell, q->sigma, q->max_dist, R, c->match.lut_host.data());
    HIP_TRY(c, hipMemcpyAsync(c->match.field + n_cells, c->match.lut_host.data(), n_lut, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->match.params = *q;
    c->match.radius = R;
    c->layers[LAYER_MATCH].on = true;
    return CM_OK;
}

// The last frame against the map around a prior (cm_kernels_match.hip; the semantics are in include/cloudmerge.h). Step 3 on
// the host: the candidates' matrices, written into the page-locked words. One upload, two clears, four launches, one copy of
// the info words back and one wait; steps 7 and 8 on the host from those words. No allocation: cm_map_match_configure made
// them all.
int map_match_evaluate(cm_ctx* c, const float pose[12]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_match_params& q = c->match.params;
    const size_t n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny;
    CmMatchDev g;
    g.tx = pose[3];
    g.ty = pose[7];
    g.inv = 1.0f / c->map.params.cell;
    g.ax = c->map.info.anchor[0];
    g.ay = c->map.info.anchor[1];
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.z_min = c->map.params.z_min;
    g.z_max = c->map.params.z_max;
    g.n_a = q.n_a;
    g.n_k = 2u * q.n_a + 1u;
    g.wx = q.wx;
    g.wy = q.wy;
    g.words = static_cast<uint32_t>((n_cells + 31) / 32);
    g.r2 = c->match.radius * c->match.radius;
    const uint32_t sx = 2u * q.wx + 1u, sy = 2u * q.wy + 1u;
    const size_t n_vol = static_cast<size_t>(g.n_k) * sx * sy;
    const float* const dirs = traj_direction_table();
    float* const up = reinterpret_cast<float*>(c->match.host + CM_MATCH_INFO_WORDS);
    for (uint32_t kk = 0; kk < g.n_k; ++kk) {
        const int k = static_cast<int>(kk) - static_cast<int>(q.n_a);
        const uint32_t e = static_cast<uint32_t>(k * static_cast<int>(q.a_stride)) & (CM_TRAJ_HEADINGS - 1u);
        const float cs = dirs[2 * e], sn = dirs[2 * e + 1];
        for (int j = 0; j < 3; ++j) {
            up[6 * kk + j] = static_cast<float>(static_cast<float>(cs * pose[j]) - static_cast<float>(sn * pose[4 + j]));
            up[6 * kk + 3 + j] = static_cast<float>(static_cast<float>(sn * pose[j]) + static_cast<float>(cs * pose[4 + j]));
        }
    }
    uint32_t* const info = c->match.vol + n_vol;
    const uint32_t n_tiles = c->frame.n_tiles;
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_MATCH);
    c->prof_used = 0;
    HIP_TRY(c, hipMemcpyAsync(c->match.q, up, 6 * static_cast<size_t>(g.n_k) * sizeof(float), hipMemcpyHostToDevice, st));
    prof_mark(c, "match_clear");
    HIP_TRY(c, hipMemsetAsync(c->match.bits, 0, static_cast<size_t>(g.n_k) * g.words * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->match.vol, 0, n_vol * 4, st));
    prof_mark(c, "k_match_field");
    cmk_match_field(st, c->cost.dist2, c->match.field + n_cells, g.r2, static_cast<uint32_t>(n_cells), c->match.field);
    prof_mark(c, "k_match_mark");
    frame_on_device(c);
    cmk_match_mark(st, c->d_frame, g, c->match.q, c->frame_mask, c->match.bits, n_tiles);
    prof_mark(c, "k_match_score");
    cmk_match_score(st, c->match.field, c->match.bits, g, c->match.vol);
    prof_mark(c, "k_match_best");
    cmk_match_best(st, c->match.vol, c->match.bits, g, info);
    if (const int e = finish_call(c, c->match.host, info, CM_MATCH_INFO_WORDS * sizeof(uint32_t))) return e;
    const uint32_t* const h = c->match.host;
    const uint32_t best = h[0];
    if (best >= n_vol) return fail(c, CM_INTERNAL, "the best entry lies outside the volume");
    cm_match_result& r = c->match.result;
    r.best = best;
    r.k = static_cast<int32_t>(best / (sx * sy)) - static_cast<int32_t>(q.n_a);
    r.j = static_cast<int32_t>((best / sx) % sy) - static_cast<int32_t>(q.wy);
    r.i = static_cast<int32_t>(best % sx) - static_cast<int32_t>(q.wx);
    r.n_cells = h[1];
    r.max_score = 255u * h[1];
    r.score = h[2];
    r.yaw = static_cast<float>(static_cast<double>(r.k * static_cast<int32_t>(q.a_stride)) * (6.283185307179586 / 4096.0));
    // step 7: the vertex of the parabola through the best entry and its two neighbours, per axis
    const auto sub = [&](bool both, uint32_t lo, uint32_t hi) {
        if (!(q.flags & CM_MATCH_SUBCELL) || !both) return 0.0;
        const int64_t den = static_cast<int64_t>(lo) - 2 * static_cast<int64_t>(h[2]) + static_cast<int64_t>(hi);
        if (den >= 0) return 0.0;
        const double v = 0.5 * static_cast<double>(static_cast<int64_t>(lo) - static_cast<int64_t>(hi)) / static_cast<double>(den);
        return v < -0.5 ? -0.5 : v > 0.5 ? 0.5 : v;
    };
    r.sub[0] = sub(r.i > -static_cast<int32_t>(q.wx) && r.i < static_cast<int32_t>(q.wx), h[3], h[4]);
    r.sub[1] = sub(r.j > -static_cast<int32_t>(q.wy) && r.j < static_cast<int32_t>(q.wy), h[5], h[6]);
    const uint32_t bk = best / (sx * sy);
    const double cell = static_cast<double>(c->map.params.cell);
    for (int j = 0; j < 3; ++j) {
        r.pose[j] = up[6 * bk + j];
        r.pose[4 + j] = up[6 * bk + 3 + j];
    }
    r.pose[3] = static_cast<float>(pose[3] + static_cast<float>((static_cast<double>(r.i) + r.sub[0]) * cell));
    r.pose[7] = static_cast<float>(pose[7] + static_cast<float>((static_cast<double>(r.j) + r.sub[1]) * cell));
    for (int j = 8; j < 12; ++j) r.pose[j] = pose[j];
    layer_mark_fresh(c->layers, LAYER_MATCH, c->frame_serial);
    return CM_OK;
}

// The beam model given back: its four buffers and its state; the field score is the layer's again.
static void mcl_beam_drop(cm_ctx* c) {
    MclLayer& m = c->mcl;
    m.beam_on = m.beam_steps_fresh = m.beam_info_have = false;
    m.beam_params = cm_mcl_beam_params{};
    m.beam_info = cm_mcl_beam_info{};
    m.beam_steps.release();
    m.beam_table.release();
    m.beam_counts.release();
    m.beam_host.release();
}

// The beam model's memory, all of it: one byte per window cell for the skips, the table (built here, cm_mcl_beam_table_build,
// and uploaded), the count words and their page-locked copy. nullptr gives it back. The particles and gen stay; the weight
// table and both infos are stale until the next update.
int map_mcl_beam_configure(cm_ctx* c, const cm_mcl_beam_params* q) {
    HIP_TRY(c, hipSetDevice(c->device));
    mcl_beam_drop(c);
    layer_mark_stale(c->layers, LAYER_MCL, "cm_map_mcl_beam_configure");
    if (!q) return CM_OK;
    MclLayer& m = c->mcl;
    const size_t n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny, n_tab = 2 * static_cast<size_t>(q->over_cells) + 3;
    if (!m.beam_steps.reserve((n_cells + 3) / 4 * 4) || !m.beam_table.reserve(n_tab) || !m.beam_counts.reserve(CM_MCL_BEAM_COUNTS) ||
        !m.beam_host.reserve(CM_MCL_BEAM_COUNTS)) {
        mcl_beam_drop(c);
        return fail(c, CM_HIP_ERROR, "cannot allocate the beam model");
    }
    std::vector<unsigned char> tab(n_tab, 0);
    cm_mcl_beam_table_build(*q, c->map.params.cell, tab.data());
    HIP_TRY(c, hipMemcpyAsync(m.beam_table, tab.data(), n_tab, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m.beam_params = *q;
    m.beam_on = true;
    return CM_OK;
}

// The hypotheses mode given back: its buffers and its state.
static void mcl_hyp_drop(cm_ctx* c) {
    MclLayer& m = c->mcl;
    m.hyp_on = m.hyp_have = false;
    m.hyp_params = cm_mcl_hyp_params{};
    m.hyp_info = cm_mcl_hyp_info{};
    m.hyp_cap_bits = 0;
    std::vector<cm_mcl_hyp>().swap(m.hyp_out);
    m.hyp_keys.release();
    m.hyp_slots.release();
    m.hyp_rec.release();
    m.hyp_words.release();
    m.hyp_bits.release();
    m.hyp_list.release();
    m.hyp_host.release();
}

// The hypotheses mode's memory, all of it (MclLayer's hyp_* fields say what each holds). nullptr gives it back. The particles
// and gen stay; the averages start at 0.0; the weight table, the infos and the hypotheses are stale until the next update.
int map_mcl_hyp_configure(cm_ctx* c, const cm_mcl_hyp_params* q) {
    HIP_TRY(c, hipSetDevice(c->device));
    mcl_hyp_drop(c);
    layer_mark_stale(c->layers, LAYER_MCL, "cm_map_mcl_hyp_configure");
    if (!q) return CM_OK;
    MclLayer& m = c->mcl;
    const size_t n = m.params.n_particles, n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny;
    uint32_t cap_bits = 6;
    while ((static_cast<size_t>(1) << cap_bits) < 4 * n) ++cap_bits;
    const size_t cap = static_cast<size_t>(1) << cap_bits;
    constexpr size_t rec_words = sizeof(CmMclHypRecDev) / sizeof(unsigned long long);
    m.hyp_out.reserve(CM_MCL_HYP_MAX);
    if (!m.hyp_keys.reserve(cap) || !m.hyp_slots.reserve(2 * cap + n) || !m.hyp_rec.reserve(n + CM_MCL_HYP_MAX) || !m.hyp_words.reserve(CM_MCL_HYP_WORDS) ||
        !m.hyp_bits.reserve((n_cells + 31) / 32) || !m.hyp_list.reserve(CM_MCL_ONE_BLOCK + n_cells) ||
        !m.hyp_host.reserve(CM_MCL_HYP_WORDS + CM_MCL_HYP_MAX * rec_words)) {
        mcl_hyp_drop(c);
        return fail(c, CM_HIP_ERROR, "cannot allocate the hypotheses of the localisation layer");
    }
    HIP_TRY(c, hipMemsetAsync(m.hyp_words, 0, CM_MCL_HYP_WORDS * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    m.hyp_cap_bits = cap_bits;
    m.hyp_params = *q;
    m.hyp_on = true;
    return CM_OK;
}

// The localisation layer's memory, all of it: two particle buffers, the weight table, the prefix sums with the info words
// behind them, the field with its table behind it (built here, cm_match_table.hpp, and uploaded), the one bitmap and the one
// list (behind the block counts) that serve the body cells and the free cells, the heading table and the page-locked words an
// update reads back. nullptr gives it back. No particles, gen = 0, weights and info stale until the first update.
int map_mcl_configure(cm_ctx* c, const cm_mcl_params* q, uint32_t R) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_MCL);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_MCL);
    mcl_beam_drop(c);
    mcl_hyp_drop(c);
    c->mcl.init = false;
    c->mcl.gen = 0;
    c->mcl.cur = 0;
    std::memset(&c->mcl.info, 0, sizeof c->mcl.info);
    const size_t n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny, side = 2 * static_cast<size_t>(q->range_cells) + 1;
    const size_t words = std::max((n_cells + 31) / 32, (side * side + 31) / 32);
    const size_t n_lut = static_cast<size_t>(R) * R + 1, n = q->n_particles;
    if (!c->mcl.parts[0].reserve(n) || !c->mcl.parts[1].reserve(n) || !c->mcl.wts.reserve(n) || !c->mcl.cum.reserve(n + CM_MCL_WORDS) ||
        !c->mcl.field.reserve(n_cells + n_lut) || !c->mcl.bits.reserve(words) ||
        !c->mcl.list.reserve(CM_MCL_ONE_BLOCK + std::max(static_cast<size_t>(q->max_beams), n_cells)) || !c->mcl.dirs.reserve(2 * CM_TRAJ_HEADINGS) ||
        !c->mcl.host.reserve(CM_MCL_WORDS))
        return fail(c, CM_HIP_ERROR, "cannot allocate the localisation layer");
    std::vector<unsigned char> lut(n_lut, 0);
    cm_match_table_build(c->map.params.cell, q->sigma, q->max_dist, R, lut.data());
    HIP_TRY(c, hipMemcpyAsync(c->mcl.field + n_cells, lut.data(), n_lut, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->mcl.dirs, traj_direction_table(), 2 * CM_TRAJ_HEADINGS * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->mcl.params = *q;
    c->mcl.radius = R;
    c->layers[LAYER_MCL].on = true;
    return CM_OK;
}

namespace {

CmMclDev mcl_dev(const cm_ctx* c) {
    const cm_mcl_params& q = c->mcl.params;
    CmMclDev g;
    g.inv = 1.0f / c->map.params.cell;
    g.cell = c->map.params.cell;
    g.ax = c->map.info.anchor[0];
    g.ay = c->map.info.anchor[1];
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.z_min = c->map.params.z_min;
    g.z_max = c->map.params.z_max;
    g.n = q.n_particles;
    g.max_beams = q.max_beams;
    g.range = q.range_cells;
    g.side = 2u * q.range_cells + 1u;
    return g;
}

// Step 2's scale of a standard deviation: (float)((double)sd * K1).
float mcl_scale(float sd) { return static_cast<float>(static_cast<double>(sd) * std::sqrt(3.0 / 4294967295.0)); }

// What an init_pose or predict call adds to a particle, and the call's gen taken.
CmMclMoveDev mcl_move(cm_ctx* c, const float v[6]) {
    CmMclMoveDev m;
    m.a = v[0];
    m.b = v[1];
    m.yaw = static_cast<double>(v[2]);
    m.sc_a = mcl_scale(v[3]);
    m.sc_b = mcl_scale(v[4]);
    m.sc_yaw = mcl_scale(v[5]);
    m.base = cm_mcl_base(c->mcl.params.seed, c->mcl.gen++);
    return m;
}

// R2: an init call puts the slow and the fast average of the hypotheses mode back to 0.0.
int mcl_hyp_restart(cm_ctx* c) {
    if (!c->mcl.hyp_on) return CM_OK;
    HIP_TRY(c, hipMemsetAsync(c->mcl.hyp_words + CM_MCL_HW_STATE_SLOW, 0, 2 * sizeof(unsigned long long), c->stream));
    return CM_OK;
}

}  // namespace

int map_mcl_init_pose(cm_ctx* c, const float v[6]) {
    HIP_TRY(c, hipSetDevice(c->device));
    c->mcl.init = false;
    layer_mark_stale(c->layers, LAYER_MCL, "the last cm_map_mcl_init_pose");
    c->mcl.cur = 0;
    c->prof_used = 0;
    prof_mark(c, "k_mcl_init_pose");
    cmk_mcl_init_pose(c->stream, mcl_move(c, v), c->mcl.params.n_particles, c->mcl.parts[0]);
    if (const int e = mcl_hyp_restart(c)) return e;
    if (const int e = finish_call(c)) return e;
    c->mcl.init = true;
    return CM_OK;
}

// The free cells by the ordered compaction of the image's bitmap; their number comes back to the host, which refuses an
// image without one before any particle is written.
int map_mcl_init_uniform(cm_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    const CmMclDev g = mcl_dev(c);
    const uint32_t n_cells = g.nx * g.ny, n_words = (n_cells + 31u) / 32u;
    unsigned long long* const words = c->mcl.cum + g.n;
    uint32_t* const counts = c->mcl.list;
    uint32_t* const list = c->mcl.list + CM_MCL_ONE_BLOCK;
    hipStream_t st = c->stream;
    c->prof_used = 0;
    prof_mark(c, "k_mcl_free_bits");
    cmk_mcl_free_bits(st, c->map.image, n_cells, c->mcl.bits);
    prof_mark(c, "k_mcl_compact");
    cmk_mcl_compact(st, c->mcl.bits, n_words, n_cells, counts, list, words);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->mcl.host, words, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->mcl.host[CM_MCL_W_NCELLS] == 0) return fail(c, CM_BAD_ARG, "the map's image holds no free cell");
    c->mcl.init = false;
    layer_mark_stale(c->layers, LAYER_MCL, "the last cm_map_mcl_init_uniform");
    c->mcl.cur = 0;
    prof_mark(c, "k_mcl_init_uniform");
    cmk_mcl_init_uniform(st, g, cm_mcl_base(c->mcl.params.seed, c->mcl.gen++), list, words, c->mcl.parts[0]);
    if (const int e = mcl_hyp_restart(c)) return e;
    if (const int e = finish_call(c)) return e;
    c->mcl.init = true;
    return CM_OK;
}

int map_mcl_predict(cm_ctx* c, const float v[6]) {
    HIP_TRY(c, hipSetDevice(c->device));
    layer_mark_stale(c->layers, LAYER_MCL, "the last cm_map_mcl_predict");
    c->prof_used = 0;
    prof_mark(c, "k_mcl_predict");
    cmk_mcl_predict(c->stream, mcl_move(c, v), c->mcl.params.n_particles, c->mcl.dirs, c->mcl.parts[c->mcl.cur]);
    if (const int e = finish_call(c)) return e;
    return CM_OK;
}

// Steps 6 to 11 (cm_kernels_mcl.hip; the semantics are in include/cloudmerge.h). Two clears, the field, the mark pass, the
// compaction, the score, the best particle, the weights with their sums, the spread, the prefix sums with the resampling
// decision, which is taken on the device, and the gather; then one copy of the info words back and one wait, the only host
// round trip. The host learns from the words whether the particles now live in the other buffer. No allocation.
int map_mcl_update(cm_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_mcl_params& q = c->mcl.params;
    const CmMclDev g = mcl_dev(c);
    const size_t n_cells = static_cast<size_t>(g.nx) * g.ny;
    const uint32_t body_words = static_cast<uint32_t>((static_cast<uint64_t>(g.side) * g.side + 31u) / 32u);
    const uint32_t r2 = c->mcl.radius * c->mcl.radius;
    unsigned long long* const words = c->mcl.cum + g.n;
    uint32_t* const counts = c->mcl.list;
    uint32_t* const list = c->mcl.list + CM_MCL_ONE_BLOCK;
    CmMclParticleDev* const src = c->mcl.parts[c->mcl.cur];
    CmMclParticleDev* const dst = c->mcl.parts[c->mcl.cur ^ 1];
    const uint64_t gen = c->mcl.gen++;
    const unsigned long long base = cm_mcl_base(q.seed, gen);
    const double beta = 1.0 / (255.0 * static_cast<double>(q.tau));
    const double thr = static_cast<double>(q.resample_frac) * static_cast<double>(q.n_particles);
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_MCL);
    c->prof_used = 0;
    prof_mark(c, "mcl_clear");
    HIP_TRY(c, hipMemsetAsync(c->mcl.bits, 0, static_cast<size_t>(body_words) * 4, st));
    HIP_TRY(c, hipMemsetAsync(words, 0, CM_MCL_WORDS * sizeof(unsigned long long), st));
    prof_mark(c, "k_match_field");
    cmk_match_field(st, c->cost.dist2, c->mcl.field + n_cells, r2, static_cast<uint32_t>(n_cells), c->mcl.field);
    prof_mark(c, "k_mcl_mark");
    frame_on_device(c);
    cmk_mcl_mark(st, c->d_frame, g, c->frame_mask, c->mcl.bits, c->frame.n_tiles);
    prof_mark(c, "k_mcl_compact");
    cmk_mcl_compact(st, c->mcl.bits, body_words, q.max_beams, counts, list, words);
    const bool beam = c->mcl.beam_on;
    CmMclBeamDev bm;
    bm.over = c->mcl.beam_params.over_cells;
    bm.plain = (c->mcl.beam_params.flags & CM_MCL_BEAM_PLAIN) ? 1u : 0u;
    bm.walks = c->mcl_beam_walks;
    c->mcl.beam_info_have = false;
    if (beam) {                                        // step 7 under the beam model: rays cast per beam
        HIP_TRY(c, hipMemsetAsync(c->mcl.beam_counts, 0, CM_MCL_BEAM_COUNTS * sizeof(unsigned long long), st));
        if (!bm.plain && !c->mcl.beam_steps_fresh) {
            prof_mark(c, "k_mcl_steps");
            cmk_cast_steps(st, c->cost.dist2, static_cast<uint32_t>(n_cells), c->mcl.beam_steps);
        }
        prof_mark(c, "k_mcl_beam");
        cmk_mcl_beam(st, c->map.image, c->mcl.beam_steps, c->mcl.beam_table, g, bm, list, words, c->mcl.dirs, src, c->mcl.wts, c->mcl.beam_counts);
        HIP_TRY(c, hipMemcpyAsync(c->mcl.beam_host, c->mcl.beam_counts, CM_MCL_BEAM_COUNTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    } else {
        prof_mark(c, "k_mcl_score");
        cmk_mcl_score(st, c->mcl.field, g, list, words, c->mcl.dirs, src, c->mcl.wts);
    }
    prof_mark(c, "k_mcl_best");
    cmk_mcl_best(st, src, g.n, words);
    prof_mark(c, "k_mcl_weights");
    cmk_mcl_weights(st, src, g.n, beta, c->mcl.dirs, c->mcl.wts, words);
    prof_mark(c, "k_mcl_spread");
    cmk_mcl_spread(st, src, g.n, c->mcl.wts, words);
    const bool hyp = c->mcl.hyp_on;
    constexpr size_t hyp_rec_words = sizeof(CmMclHypRecDev) / sizeof(unsigned long long);
    CmMclHypDev hy{};
    c->mcl.hyp_have = false;
    if (hyp) {                                         // the hypotheses over the particles as found, then R1 to R3
        const cm_mcl_hyp_params& hp = c->mcl.hyp_params;
        const size_t cap = static_cast<size_t>(1) << c->mcl.hyp_cap_bits;
        hy.on = 1u;
        hy.n = g.n;
        hy.cap_bits = c->mcl.hyp_cap_bits;
        hy.bin_q = hp.bin_q;
        hy.heading_bits = hp.heading_bits;
        hy.max_hyp = hp.max_hyp;
        hy.inject_max = hp.inject_max;
        hy.agg = c->mcl_hyp_agg;
        hy.a_slow = static_cast<double>(hp.alpha_slow);
        hy.a_fast = static_cast<double>(hp.alpha_fast);
        hy.keys = c->mcl.hyp_keys;
        hy.parent = c->mcl.hyp_slots;
        hy.comp = c->mcl.hyp_slots + cap;
        hy.slot = c->mcl.hyp_slots + 2 * cap;
        hy.rec = c->mcl.hyp_rec;
        hy.out = c->mcl.hyp_rec + g.n;
        hy.words = c->mcl.hyp_words;
        hy.free_list = c->mcl.hyp_list + CM_MCL_ONE_BLOCK;
        prof_mark(c, "mcl_hyp_clear");
        HIP_TRY(c, hipMemsetAsync(hy.keys, 0xFF, cap * sizeof(unsigned long long), st));
        HIP_TRY(c, hipMemsetAsync(hy.words, 0, CM_MCL_HW_CLEARED * sizeof(unsigned long long), st));
        prof_mark(c, "k_mcl_hyp_bins");
        cmk_mcl_hyp_bins(st, src, hy);
        prof_mark(c, "k_mcl_hyp_link");
        cmk_mcl_hyp_link(st, hy);
        prof_mark(c, "k_mcl_hyp_flatten");
        cmk_mcl_hyp_flatten(st, hy);
        prof_mark(c, "k_mcl_hyp_sums");
        cmk_mcl_hyp_sums(st, src, c->mcl.wts, c->mcl.dirs, hy);
        prof_mark(c, "k_mcl_hyp_spread");
        cmk_mcl_hyp_spread(st, src, c->mcl.wts, hy);
        prof_mark(c, "k_mcl_hyp_pick");
        cmk_mcl_hyp_pick(st, hy);
        if (hp.inject_max) {                           // the free cells of the current image, in the mode's own bitmap and list
            const uint32_t cells = static_cast<uint32_t>(n_cells);
            prof_mark(c, "k_mcl_free_bits");
            cmk_mcl_free_bits(st, c->map.image, cells, c->mcl.hyp_bits);
            prof_mark(c, "k_mcl_compact");
            cmk_mcl_compact(st, c->mcl.hyp_bits, (cells + 31u) / 32u, cells, c->mcl.hyp_list, c->mcl.hyp_list + CM_MCL_ONE_BLOCK, hy.words);
        }
        prof_mark(c, "k_mcl_hyp_recover");
        cmk_mcl_hyp_recover(st, hy, words);
    }
    prof_mark(c, "k_mcl_resample");
    cmk_mcl_resample(st, src, dst, g, c->mcl.wts, c->mcl.cum, base, cm_mcl_splitmix64(base ^ (1ull << 63)), thr,
                     (q.flags & CM_MCL_RESAMPLE_ALWAYS) ? 1u : 0u, words, hy);
    if (hyp) {
        HIP_TRY(c, hipMemcpyAsync(c->mcl.hyp_host, hy.words, CM_MCL_HYP_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(c->mcl.hyp_host + CM_MCL_HYP_WORDS, hy.out, static_cast<size_t>(hy.max_hyp) * sizeof(CmMclHypRecDev), hipMemcpyDeviceToHost, st));
    }
    if (const int e = finish_call(c, c->mcl.host, words, CM_MCL_WORDS * sizeof(unsigned long long))) return e;
    const unsigned long long* const h = c->mcl.host;
    if (h[CM_MCL_W_BEST] >= g.n || h[CM_MCL_W_SW] < CM_MCL_WEIGHT_ONE || h[CM_MCL_W_SW2] == 0) return fail(c, CM_INTERNAL, "the info words of the update are not a result");
    if (hyp) {
        const unsigned long long* const w = c->mcl.hyp_host;
        const cm_mcl_hyp_params& hp = c->mcl.hyp_params;
        const uint64_t n_hyp = w[CM_MCL_HW_NHYP];
        if (w[CM_MCL_HW_NBINS] < 1 || w[CM_MCL_HW_NBINS] > g.n || w[CM_MCL_HW_NCOMP] < 1 || w[CM_MCL_HW_NCOMP] > w[CM_MCL_HW_NBINS] ||
            n_hyp != std::min<uint64_t>(w[CM_MCL_HW_NCOMP], hp.max_hyp) || w[CM_MCL_HW_NINJECT] > hp.inject_max)
            return fail(c, CM_INTERNAL, "the words of the hypotheses are not a result");
        cm_mcl_hyp_info& hi = c->mcl.hyp_info;
        std::memset(&hi, 0, sizeof hi);
        hi.gen = gen;
        hi.n_bins = static_cast<uint32_t>(w[CM_MCL_HW_NBINS]);
        hi.n_components = static_cast<uint32_t>(w[CM_MCL_HW_NCOMP]);
        hi.n_hyp = static_cast<uint32_t>(n_hyp);
        (void)cm_mcl_kld_bound(hi.n_bins, hp.kld_err, hp.kld_z, &hi.n_kld);
        hi.n_inject = static_cast<uint32_t>(w[CM_MCL_HW_NINJECT]);
        hi.n_free = static_cast<uint32_t>(w[CM_MCL_HW_NFREE]);
        hi.sum_s = w[CM_MCL_HW_SUMS];
        std::memcpy(&hi.w_avg, w + CM_MCL_HW_WAVG, 8);
        std::memcpy(&hi.w_slow, w + CM_MCL_HW_WSLOW, 8);
        std::memcpy(&hi.w_fast, w + CM_MCL_HW_WFAST, 8);
        std::memcpy(&hi.p_inject, w + CM_MCL_HW_PINJECT, 8);
        const double total = static_cast<double>(h[CM_MCL_W_SW]);
        c->mcl.hyp_out.clear();                        // (capacity CM_MCL_HYP_MAX since the configure call: no allocation)
        for (uint64_t k = 0; k < n_hyp; ++k) {
            CmMclHypRecDev d;
            std::memcpy(&d, w + CM_MCL_HYP_WORDS + k * hyp_rec_words, sizeof d);
            cm_mcl_hyp o;
            std::memset(&o, 0, sizeof o);
            o.label = d.label;
            o.n = static_cast<uint32_t>(d.n);
            o.top = ~static_cast<uint32_t>(d.top);
            o.sum_w = d.sum_w;
            o.sum_wqx = static_cast<int64_t>(d.sum_wqx);
            o.sum_wqy = static_cast<int64_t>(d.sum_wqy);
            o.sum_wc = static_cast<int64_t>(d.sum_wc);
            o.sum_ws = static_cast<int64_t>(d.sum_ws);
            o.sum_wdxx = static_cast<int64_t>(d.sum_wdxx);
            o.sum_wdyy = static_cast<int64_t>(d.sum_wdyy);
            o.sum_wdxy = static_cast<int64_t>(d.sum_wdxy);
            if (d.sum_w) {
                const double sw = static_cast<double>(o.sum_w), den = sw * 1048576.0;
                o.share = sw / total;
                o.mean_x = (static_cast<double>(o.sum_wqx) / sw) / 1024.0;
                o.mean_y = (static_cast<double>(o.sum_wqy) / sw) / 1024.0;
                o.mean_yaw = std::atan2(static_cast<double>(o.sum_ws), static_cast<double>(o.sum_wc));
                o.var_xx = static_cast<double>(o.sum_wdxx) / den;
                o.var_yy = static_cast<double>(o.sum_wdyy) / den;
                o.var_xy = static_cast<double>(o.sum_wdxy) / den;
            }
            c->mcl.hyp_out.push_back(o);
        }
    }
    if (beam) {
        const unsigned long long* const b = c->mcl.beam_host;
        cm_mcl_beam_info& bi = c->mcl.beam_info;
        bi.n_rays = static_cast<uint64_t>(g.n) * std::min<uint64_t>(h[CM_MCL_W_NBEAMS], g.max_beams);
        bi.n_early = b[0];
        bi.n_at = b[1];
        bi.n_late = b[2];
        bi.n_beyond = b[3];
        bi.n_off = b[4];
        bi.n_skipped = b[5];
        if (b[0] + b[1] + b[2] + b[3] + b[4] + b[5] != bi.n_rays) return fail(c, CM_INTERNAL, "the outcome counts of the beam model do not add up to its rays");
        if (!bm.plain) c->mcl.beam_steps_fresh = true;
    }
    if (h[CM_MCL_W_RESAMPLED]) c->mcl.cur ^= 1;
    cm_mcl_info& r = c->mcl.info;
    std::memset(&r, 0, sizeof r);
    r.n_particles = g.n;
    r.n_cells = static_cast<uint32_t>(h[CM_MCL_W_NCELLS]);
    r.stride = static_cast<uint32_t>(h[CM_MCL_W_STRIDE]);
    r.n_beams = static_cast<uint32_t>(h[CM_MCL_W_NBEAMS]);
    r.gen = gen;
    r.resampled = static_cast<uint32_t>(h[CM_MCL_W_RESAMPLED]);
    r.best = static_cast<uint32_t>(h[CM_MCL_W_BEST]);
    const uint32_t bx = static_cast<uint32_t>(h[CM_MCL_W_BEST_X]), by = static_cast<uint32_t>(h[CM_MCL_W_BEST_Y]);
    std::memcpy(&r.best_x, &bx, 4);
    std::memcpy(&r.best_y, &by, 4);
    r.best_h = static_cast<uint32_t>(h[CM_MCL_W_BEST_H]);
    r.sum_w = h[CM_MCL_W_SW];
    r.sum_w2 = h[CM_MCL_W_SW2];
    r.sum_wqx = static_cast<int64_t>(h[CM_MCL_W_SWQX]);
    r.sum_wqy = static_cast<int64_t>(h[CM_MCL_W_SWQY]);
    r.sum_wc = static_cast<int64_t>(h[CM_MCL_W_SWC]);
    r.sum_ws = static_cast<int64_t>(h[CM_MCL_W_SWS]);
    r.sum_wdxx = static_cast<int64_t>(h[CM_MCL_W_SWDXX]);
    r.sum_wdyy = static_cast<int64_t>(h[CM_MCL_W_SWDYY]);
    r.sum_wdxy = static_cast<int64_t>(h[CM_MCL_W_SWDXY]);
    const double sw = static_cast<double>(r.sum_w);
    r.n_eff = (sw * sw) / static_cast<double>(r.sum_w2);
    r.mean_x = (static_cast<double>(r.sum_wqx) / sw) / 1024.0;
    r.mean_y = (static_cast<double>(r.sum_wqy) / sw) / 1024.0;
    r.mean_yaw = std::atan2(static_cast<double>(r.sum_ws), static_cast<double>(r.sum_wc));
    const double den = sw * 1048576.0;
    r.var_xx = static_cast<double>(r.sum_wdxx) / den;
    r.var_yy = static_cast<double>(r.sum_wdyy) / den;
    r.var_xy = static_cast<double>(r.sum_wdxy) / den;
    c->mcl.beam_info_have = beam;
    c->mcl.hyp_have = hyp;
    layer_mark_fresh(c->layers, LAYER_MCL, c->frame_serial);
    return CM_OK;
}

// Step 3 of the cast layer: the rollout layer's heading table scaled by range_cells and rounded, ties to even.
void cast_direction_table(uint32_t range_cells, int16_t* dst) {
    const float* const t = traj_direction_table();
    const double R = static_cast<double>(range_cells);
    for (uint32_t i = 0; i < 2 * CM_TRAJ_HEADINGS; ++i) dst[i] = static_cast<int16_t>(std::rint(static_cast<double>(t[i]) * R));
}

// The cast layer's memory, all of it: the rays, the poses an evaluate uploads, the bearings and the direction table (both
// uploaded here), the skip table, the count words and their page-locked copy. nullptr gives it back. The rays are stale until
// the first evaluate.
int map_cast_configure(cm_ctx* c, const cm_cast_params* q, const uint32_t* bearings) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_CAST);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_CAST);
    c->cast.steps_fresh = false;
    std::memset(&c->cast.info, 0, sizeof c->cast.info);
    const size_t n_cells = static_cast<size_t>(c->map.info.nx) * c->map.info.ny, nb = q->n_bearings;
    if (!c->cast.rays.reserve(static_cast<size_t>(q->max_poses) * nb) || !c->cast.poses.reserve(3 * static_cast<size_t>(q->max_poses)) ||
        !c->cast.bearings.reserve(nb) || !c->cast.dirs.reserve(CM_CAST_DIRS) || !c->cast.steps.reserve((n_cells + 3) / 4 * 4) ||
        !c->cast.words.reserve(CM_CAST_WORDS) || !c->cast.host.reserve(CM_CAST_WORDS))
        return fail(c, CM_HIP_ERROR, "cannot allocate the cast layer");
    std::vector<uint32_t> b(nb);
    for (size_t a = 0; a < nb; ++a) b[a] = bearings ? bearings[a] : static_cast<uint32_t>((static_cast<uint64_t>(a) << 32) / nb);
    std::vector<int16_t> dirs(2 * CM_CAST_DIRS);
    cast_direction_table(q->range_cells, dirs.data());
    HIP_TRY(c, hipMemcpyAsync(c->cast.bearings, b.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->cast.dirs, dirs.data(), CM_CAST_DIRS * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->cast.params = *q;
    c->layers[LAYER_CAST].on = true;
    return CM_OK;
}

// Steps 1 to 7 (cm_kernels_cast.hip; the semantics are in include/cloudmerge.h). One upload of the poses (none where they are
// the particles), one clear of the counts, the skip table where dist2 has changed since it was built, the rays, then one copy
// of the counts back and one wait. No allocation.
int map_cast_evaluate(cm_ctx* c, const cm_cast_pose* host_poses, uint32_t n) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_cast_params& q = c->cast.params;
    CmCastDev g;
    g.inv = 1.0f / c->map.params.cell;
    g.ax = c->map.info.anchor[0];
    g.ay = c->map.info.anchor[1];
    g.nx = c->map.info.nx;
    g.ny = c->map.info.ny;
    g.n_poses = n;
    g.n_bearings = q.n_bearings;
    g.pose_words = host_poses ? 3u : static_cast<uint32_t>(sizeof(CmMclParticleDev) / sizeof(uint32_t));
    g.plain = (q.flags & CM_CAST_PLAIN) ? 1u : 0u;
    const void* const poses = host_poses ? static_cast<const void*>(c->cast.poses) : static_cast<const void*>(c->mcl.parts[c->mcl.cur]);
    hipStream_t st = c->stream;
    layer_mark_failed(c->layers, LAYER_CAST);
    c->prof_used = 0;
    prof_mark(c, "cast_upload");
    if (host_poses) HIP_TRY(c, hipMemcpyAsync(c->cast.poses, host_poses, static_cast<size_t>(n) * sizeof(cm_cast_pose), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->cast.words, 0, CM_CAST_WORDS * sizeof(uint32_t), st));
    if (!g.plain && !c->cast.steps_fresh) {
        prof_mark(c, "k_cast_steps");
        cmk_cast_steps(st, c->cost.dist2, g.nx * g.ny, c->cast.steps);
    }
    prof_mark(c, "k_cast_rays");
    cmk_cast_rays(st, c->map.image, c->cast.steps, g, poses, c->cast.bearings, c->cast.dirs, c->cast.rays, c->cast.words);
    if (const int e = finish_call(c, c->cast.host, c->cast.words, CM_CAST_WORDS * sizeof(uint32_t))) return e;
    if (!g.plain) c->cast.steps_fresh = true;
    const uint32_t* const h = c->cast.host;
    if (static_cast<uint64_t>(h[0]) + h[1] + h[2] + h[3] != static_cast<uint64_t>(n) * q.n_bearings)
        return fail(c, CM_INTERNAL, "the status counts of the cast do not add up to its rays");
    cm_cast_info& r = c->cast.info;
    r.n_poses = n;
    r.n_bearings = q.n_bearings;
    r.n_max = h[CM_CAST_MAX];
    r.n_hit = h[CM_CAST_HIT];
    r.n_off_map = h[CM_CAST_OFF_MAP];
    r.n_no_origin = h[CM_CAST_NO_ORIGIN];
    layer_mark_fresh(c->layers, LAYER_CAST, c->frame_serial);
    return CM_OK;
}

// A recorded state table into the map: the table into the current state buffer, the image by step 8, the anchor; the layers
// behind go stale exactly as after an integration, and the frame at rest counts as not yet integrated.
int map_load(cm_ctx* c, const cm_map_cell* src, const int32_t anchor[2]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_map_params& q = c->map.params;
    const uint64_t n_cells = static_cast<uint64_t>(q.nx) * q.ny;
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemcpyAsync(c->map.state[c->map.cur], src, n_cells * sizeof(cm_map_cell), hipMemcpyHostToDevice, st));
    cmk_map_image(st, c->map.state[c->map.cur], static_cast<uint32_t>(n_cells), q.l_free, q.l_occ, c->map.image);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    c->map.info.anchor[0] = anchor[0];
    c->map.info.anchor[1] = anchor[1];
    c->map.info.n_frames = 1;
    c->map.info.sensors_cast = 0;
    c->map.serial = 0;
    layers_mark_below(c->layers, LAYER_MAP, "the last cm_map_load");
    return CM_OK;
}

size_t msearch_level_offset(uint32_t nx, uint32_t ny, uint32_t h) {
    size_t off = 0;
    for (uint32_t l = 0; l < h; ++l) off += static_cast<size_t>(nx + (1u << l) - 1u) * (ny + (1u << l) - 1u);
    return off;
}

namespace {

uint32_t msearch_roots_along(uint32_t w, uint32_t depth) { return (2u * w + (1u << depth)) >> depth; }     // ceil((2 w + 1) / 2^depth)

// Where the parts of msearch_nodes and msearch_host start.
struct MSearchLayout {
    size_t roots, list[2], u, words;   // msearch_nodes
    size_t h_counts, h_init, h_q;      // msearch_host (the words read back start at 0)
};
MSearchLayout msearch_layout(const cm_match_search_params& q, uint32_t n_roots) {
    MSearchLayout l;
    l.roots = 0;
    l.list[0] = n_roots;
    l.list[1] = l.list[0] + q.max_nodes;
    l.u = l.list[1] + q.max_nodes;
    l.words = l.u + q.max_nodes;
    l.h_counts = CM_MSEARCH_WORDS;
    l.h_init = l.h_counts + 256;
    l.h_q = l.h_init + CM_MSEARCH_WORDS;
    return l;
}

}  // namespace

// The search layer's memory, all of it: the pyramid with the field table behind it, one bitmap and one cell list per angle
// candidate with the counts behind them, the roots (built here and uploaded), two node lists, the scores and the info words,
// the candidates' matrices and the page-locked words. nullptr gives it back. Everything is stale until the first evaluate.
int map_msearch_configure(cm_ctx* c, const cm_match_search_params* q, uint32_t R) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!q) {
        layer_drop(c, LAYER_SEARCH);
        return CM_OK;
    }
    layer_reset(c->layers, LAYER_SEARCH);
    std::memset(&c->msearch.result, 0, sizeof c->msearch.result);
    std::memset(&c->msearch.info, 0, sizeof c->msearch.info);
    const uint32_t nx = c->map.info.nx, ny = c->map.info.ny;
    const size_t n_cells = static_cast<size_t>(nx) * ny, words = (n_cells + 31) / 32;
    const size_t n_k = 2 * static_cast<size_t>(q->n_a) + 1, n_lut = static_cast<size_t>(R) * R + 1;
    const uint32_t rx = msearch_roots_along(q->wx, q->depth), ry = msearch_roots_along(q->wy, q->depth);
    const uint32_t n_roots = static_cast<uint32_t>(n_k) * rx * ry;
    const MSearchLayout l = msearch_layout(*q, n_roots);
    const size_t n_pyr = msearch_level_offset(nx, ny, q->depth + 1u);
    if (!c->msearch.pyr.reserve(n_pyr + n_lut) || !c->msearch.bits.reserve(n_k * words) || !c->msearch.cells.reserve(n_k * q->max_cells + n_k) ||
        !c->msearch.nodes.reserve(l.words + CM_MSEARCH_WORDS) || !c->msearch.q.reserve(6 * n_k) ||
        !c->msearch.host.reserve(std::max(l.h_q + 6 * n_k, static_cast<size_t>(n_roots))))
        return fail(c, CM_HIP_ERROR, "cannot allocate the search layer");
    std::vector<unsigned char> lut(n_lut, 0);
    cm_match_table_build(c->map.params.cell, q->sigma, q->max_dist, R, lut.data());
    uint32_t* const roots = c->msearch.host;           // (the page-locked words are free until the first evaluate)
    size_t r = 0;
    for (uint32_t kk = 0; kk < n_k; ++kk)
        for (uint32_t b = 0; b < ry; ++b)
            for (uint32_t a = 0; a < rx; ++a) roots[r++] = (kk << 24) | ((b << q->depth) << 12) | (a << q->depth);
    HIP_TRY(c, hipMemcpyAsync(c->msearch.pyr + n_pyr, lut.data(), n_lut, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->msearch.nodes + l.roots, roots, static_cast<size_t>(n_roots) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->msearch.params = *q;
    c->msearch.radius = R;
    c->msearch.n_roots = n_roots;
    c->layers[LAYER_SEARCH].on = true;
    return CM_OK;
}

// The last frame against the map around a prior, by branch and bound (cm_kernels_msearch.hip; the semantics are in
// include/cloudmerge.h). The candidates' matrices and the info words' initial values go up from the page-locked words; field,
// pyramid, bitmaps and cell lists are made; the prior's leaf and the roots are scored and the descent for B runs on the
// device, each score launch reading its list's length from the info words. Then one host round trip per level: the live nodes
// and their children, which size the next launch and decide an overflow. The leaves' best entry, its four neighbours as leaves,
// one last copy; steps 7 and 8 on the host. No allocation: cm_map_match_search_configure made them all.
int map_msearch_evaluate(cm_ctx* c, const float pose[12]) {
    HIP_TRY(c, hipSetDevice(c->device));
    const cm_match_search_params& q = c->msearch.params;
    const uint32_t nx = c->map.info.nx, ny = c->map.info.ny, n_roots = c->msearch.n_roots;
    const size_t n_cells = static_cast<size_t>(nx) * ny;
    const MSearchLayout l = msearch_layout(q, n_roots);
    CmMatchDev g{};                                    // (for the exhaustive layer's mark kernel: no shifts)
    g.tx = pose[3];
    g.ty = pose[7];
    g.inv = 1.0f / c->map.params.cell;
    g.ax = c->map.info.anchor[0];
    g.ay = c->map.info.anchor[1];
    g.nx = nx;
    g.ny = ny;
    g.z_min = c->map.params.z_min;
    g.z_max = c->map.params.z_max;
    g.n_a = q.n_a;
    g.n_k = 2u * q.n_a + 1u;
    g.wx = 0;
    g.wy = 0;
    g.words = static_cast<uint32_t>((n_cells + 31) / 32);
    g.r2 = c->msearch.radius * c->msearch.radius;
    const CmMSearchDev m{nx, ny, g.n_k, q.n_a, q.wx, q.wy, q.max_cells};
    const float* const dirs = traj_direction_table();
    uint32_t* const hw = c->msearch.host;              // the info words read back
    uint32_t* const hcounts = c->msearch.host + l.h_counts;
    uint32_t* const init = c->msearch.host + l.h_init;
    float* const up = reinterpret_cast<float*>(c->msearch.host + l.h_q);
    for (uint32_t kk = 0; kk < g.n_k; ++kk) {
        const int k = static_cast<int>(kk) - static_cast<int>(q.n_a);
        const uint32_t e = static_cast<uint32_t>(k * static_cast<int>(q.a_stride)) & (CM_TRAJ_HEADINGS - 1u);
        const float cs = dirs[2 * e], sn = dirs[2 * e + 1];
        for (int j = 0; j < 3; ++j) {
            up[6 * kk + j] = static_cast<float>(static_cast<float>(cs * pose[j]) - static_cast<float>(sn * pose[4 + j]));
            up[6 * kk + 3 + j] = static_cast<float>(static_cast<float>(sn * pose[j]) + static_cast<float>(cs * pose[4 + j]));
        }
    }
    std::memset(init, 0, CM_MSEARCH_WORDS * sizeof(uint32_t));
    init[CM_MSEARCH_W_PROBE] = 1u;                     // the prior's leaf
    init[CM_MSEARCH_W_PRIOR] = (q.n_a << 24) | (q.wy << 12) | q.wx;
    init[CM_MSEARCH_W_ONE] = 1u;
    init[CM_MSEARCH_W_FOUR] = 4u;
    init[CM_MSEARCH_W_NROOTS] = n_roots;
    unsigned char* const pyr = c->msearch.pyr;
    const unsigned char* const lut = pyr + msearch_level_offset(nx, ny, q.depth + 1u);
    const auto level = [&](uint32_t h) { return pyr + msearch_level_offset(nx, ny, h); };
    uint32_t* const cells = c->msearch.cells;
    uint32_t* const counts = cells + static_cast<size_t>(g.n_k) * q.max_cells;
    uint32_t* const nodes = c->msearch.nodes;
    uint32_t* const words = nodes + l.words;
    uint32_t* const U = nodes + l.u;
    hipStream_t st = c->stream;
    cm_match_search_info& info = c->msearch.info;
    std::memset(&info, 0, sizeof info);
    info.depth = q.depth;
    info.n_roots = n_roots;
    info.overflow_level = -1;
    layer_mark_failed(c->layers, LAYER_SEARCH);
    c->prof_used = 0;
    HIP_TRY(c, hipMemcpyAsync(c->msearch.q, up, 6 * static_cast<size_t>(g.n_k) * sizeof(float), hipMemcpyHostToDevice, st));
    prof_mark(c, "msearch_clear");
    HIP_TRY(c, hipMemcpyAsync(words, init, CM_MSEARCH_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->msearch.bits, 0, static_cast<size_t>(g.n_k) * g.words * 4, st));
    HIP_TRY(c, hipMemsetAsync(counts, 0, static_cast<size_t>(g.n_k) * 4, st));
    prof_mark(c, "k_match_field");
    cmk_match_field(st, c->cost.dist2, lut, g.r2, static_cast<uint32_t>(n_cells), pyr);
    prof_mark(c, "k_msearch_pyramid");
    for (uint32_t h = 1; h <= q.depth; ++h) cmk_msearch_pyramid(st, level(h - 1u), level(h), nx, ny, h);
    prof_mark(c, "k_match_mark");
    frame_on_device(c);
    cmk_match_mark(st, c->d_frame, g, c->msearch.q, c->frame_mask, c->msearch.bits, c->frame.n_tiles);
    prof_mark(c, "k_msearch_list");
    cmk_msearch_list(st, c->msearch.bits, m, g.words, cells, counts);
    // A list's nodes times `splits` stripes of cells are the workgroups of a score launch: about 4096, no stripe under 1024
    // cells of room. More than one stripe adds into the scores, which are zero before: the info words' by their upload and by
    // k_msearch_pick, U by a clear.
    const auto splits_of = [&](uint32_t n) { return std::max(1u, std::min({4096u / n, (q.max_cells + 1023u) / 1024u, 64u})); };
    const auto score = [&](const uint32_t* list, const uint32_t* n_ptr, uint32_t n, uint32_t h, uint32_t* out) -> int {
        const uint32_t sp = splits_of(n);
        if (sp > 1u && out == U) HIP_TRY(c, hipMemsetAsync(U, 0, static_cast<size_t>(n) * sizeof(uint32_t), st));
        cmk_msearch_score(st, list, n_ptr, n, m, level(h), h, cells, counts, sp, out);
        return CM_OK;
    };
    // the bound B: the prior's leaf, the roots, the descent
    prof_mark(c, "k_msearch_score");
    if (const int e = score(words + CM_MSEARCH_W_PRIOR, words + CM_MSEARCH_W_ONE, 1, 0, words + CM_MSEARCH_W_PRIOR_U)) return e;
    if (const int e = score(nodes + l.roots, words + CM_MSEARCH_W_NROOTS, n_roots, q.depth, U)) return e;
    prof_mark(c, "k_msearch_pick");
    cmk_msearch_pick(st, nodes + l.roots, U, words + CM_MSEARCH_W_NROOTS, n_roots, m, q.depth, words);
    for (uint32_t h = q.depth; h-- > 0u;) {
        prof_mark(c, "k_msearch_score");
        if (const int e = score(words + CM_MSEARCH_W_TINY, words + CM_MSEARCH_W_TN, 4, h, words + CM_MSEARCH_W_TINY_U)) return e;
        prof_mark(c, "k_msearch_pick");
        cmk_msearch_pick(st, words + CM_MSEARCH_W_TINY, words + CM_MSEARCH_W_TINY_U, words + CM_MSEARCH_W_TN, 4, m, h, words);
    }
    // the level loop
    const uint32_t* cur = nodes + l.roots;
    uint32_t n_cur = n_roots;
    info.scored[q.depth] = n_roots;
    bool first = true;
    const auto fetch = [&]() -> int {                  // the info words (and once the counts) back, and a wait
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(hw, words, CM_MSEARCH_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (first) {
            HIP_TRY(c, hipMemcpyAsync(hcounts, counts, static_cast<size_t>(g.n_k) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(c, hipStreamSynchronize(st));
        if (first) {
            first = false;
            for (uint32_t kk = 0; kk < g.n_k; ++kk)
                if (hcounts[kk] > q.max_cells) {
                    info.overflow_level = CM_MATCH_SEARCH_OVERFLOW_CELLS;
                    info.scored[q.depth] = 0u;
                    return fail(c, CM_CAPACITY, "a candidate has more cells than max_cells");
                }
        }
        return CM_OK;
    };
    for (uint32_t h = q.depth; h >= 1u; --h) {
        uint32_t* const next = nodes + l.list[h & 1u];
        prof_mark(c, "k_msearch_select");
        cmk_msearch_select(st, cur, U, n_cur, m, h, words + CM_MSEARCH_W_B, next, q.max_nodes, words + CM_MSEARCH_W_LEVEL + 2u * h);
        if (const int e = fetch()) { prof_mark(c, "end"); collect_stage_times_by_name(c); return e; }
        info.bound = hw[CM_MSEARCH_W_B];
        info.n_probe = hw[CM_MSEARCH_W_PROBE];
        info.live[h] = hw[CM_MSEARCH_W_LEVEL + 2u * h];
        info.scored[h - 1u] = hw[CM_MSEARCH_W_LEVEL + 2u * h + 1u];
        if (info.scored[h - 1u] > q.max_nodes) {
            info.overflow_level = static_cast<int32_t>(h - 1u);
            prof_mark(c, "end");
            collect_stage_times_by_name(c);
            return fail(c, CM_CAPACITY, "a level has more nodes than max_nodes");
        }
        if (info.scored[h - 1u] == 0u) return fail(c, CM_INTERNAL, "no live node at a level");
        cur = next;
        n_cur = info.scored[h - 1u];
        HIP_TRY(c, hipMemcpyAsync(words + CM_MSEARCH_W_TN, hw + CM_MSEARCH_W_LEVEL + 2u * h + 1u, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        prof_mark(c, "k_msearch_score");
        if (const int e = score(cur, words + CM_MSEARCH_W_TN, n_cur, h - 1u, U)) return e;
    }
    prof_mark(c, "k_msearch_best");
    cmk_msearch_best(st, cur, U, n_cur, m, counts, words);
    prof_mark(c, "k_msearch_score");
    if (const int e = score(words + CM_MSEARCH_W_NEIGH, words + CM_MSEARCH_W_FOUR, 4, 0, words + CM_MSEARCH_W_NEIGH_U)) return e;
    prof_mark(c, "end");
    const int fe = fetch();
    collect_stage_times_by_name(c);
    if (fe) return fe;
    info.bound = hw[CM_MSEARCH_W_B];
    info.n_probe = hw[CM_MSEARCH_W_PROBE];
    info.live[0] = hw[CM_MSEARCH_W_LIVE0];
    const uint32_t node = hw[CM_MSEARCH_W_BEST];
    const uint32_t sx = 2u * q.wx + 1u, sy = 2u * q.wy + 1u;
    const uint32_t bk = node >> 24, bj = (node >> 12) & 4095u, bi = node & 4095u;
    if (bk >= g.n_k || bj >= sy || bi >= sx) return fail(c, CM_INTERNAL, "the best entry lies outside the range");
    cm_match_result& r = c->msearch.result;
    r.best = (bk * sy + bj) * sx + bi;
    r.k = static_cast<int32_t>(bk) - static_cast<int32_t>(q.n_a);
    r.j = static_cast<int32_t>(bj) - static_cast<int32_t>(q.wy);
    r.i = static_cast<int32_t>(bi) - static_cast<int32_t>(q.wx);
    r.n_cells = hw[CM_MSEARCH_W_NCELLS];
    r.max_score = 255u * r.n_cells;
    r.score = hw[CM_MSEARCH_W_SCORE];
    r.yaw = static_cast<float>(static_cast<double>(r.k * static_cast<int32_t>(q.a_stride)) * (6.283185307179586 / 4096.0));
    // step 7: the vertex of the parabola through the best entry and its two neighbours, per axis
    const auto sub = [&](bool both, uint32_t lo, uint32_t hi) {
        if (!(q.flags & CM_MATCH_SUBCELL) || !both) return 0.0;
        const int64_t den = static_cast<int64_t>(lo) - 2 * static_cast<int64_t>(r.score) + static_cast<int64_t>(hi);
        if (den >= 0) return 0.0;
        const double v = 0.5 * static_cast<double>(static_cast<int64_t>(lo) - static_cast<int64_t>(hi)) / static_cast<double>(den);
        return v < -0.5 ? -0.5 : v > 0.5 ? 0.5 : v;
    };
    const uint32_t* const nu = hw + CM_MSEARCH_W_NEIGH_U;
    r.sub[0] = sub(bi > 0u && bi + 1u < sx, nu[0], nu[1]);
    r.sub[1] = sub(bj > 0u && bj + 1u < sy, nu[2], nu[3]);
    const double cell = static_cast<double>(c->map.params.cell);
    for (int j = 0; j < 3; ++j) {
        r.pose[j] = up[6 * bk + j];
        r.pose[4 + j] = up[6 * bk + 3 + j];
    }
    r.pose[3] = static_cast<float>(pose[3] + static_cast<float>((static_cast<double>(r.i) + r.sub[0]) * cell));
    r.pose[7] = static_cast<float>(pose[7] + static_cast<float>((static_cast<double>(r.j) + r.sub[1]) * cell));
    for (int j = 8; j < 12; ++j) r.pose[j] = pose[j];
    layer_mark_fresh(c->layers, LAYER_SEARCH, c->frame_serial);
    return CM_OK;
}

// Normals and curvature of the last result (cm_kernels_normals.hip): one cm_voxel_normal per result record into nrm_entries.
// The search index over a grid decided on the host (normals_grid), then the exact k-nearest-neighbour search in two launches.
// Reads `out`. Two host round trips: the bounds of the centroids and the length of the second launch's list (an empty list
// costs no launch). Under CM_FLAG_PROFILE the stage times of the call replace the frame's in cm_get_stage_times; the second
// launch's stage is named "k_nrm_rings n=<centroids it took>".
int normals(cm_ctx* c, const cm_normal_params& q) {
    const uint32_t n = static_cast<uint32_t>(c->result.n_out);
    c->nrm_n_listed = 0;
    c->nrm_have = false;
    if (n == 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t n_slots = round_up(n, CM_TILE);
    SearchIndex& ix = c->nrm;
    if (const int e = reserve_search_index(c, ix, 1, "cannot allocate the normal estimation's buffers",
                                           "cannot allocate the normal estimation's state")) return e;
    if (!c->nrm_list.reserve(static_cast<size_t>(n_slots) * 8) || !c->nrm_entries.reserve(static_cast<size_t>(n_slots) * sizeof(cm_voxel_normal)))
        return fail(c, CM_HIP_ERROR, "cannot allocate the normal estimation's buffers");
    if (!c->nrm_words.once(2)) return fail(c, CM_HIP_ERROR, "cannot allocate the normal estimation's state");
    hipStream_t st = c->stream;
    uint32_t* const w = c->nrm_words;
    c->prof_used = 0;

    // the list count of the first search launch, cleared ahead of result_bounds' stage mark on purpose: the same order of
    // device work as with the clear behind the mark, only its few bytes are no longer timed as "k_cl_bounds"
    HIP_TRY(c, hipMemsetAsync(w, 0, 8, st));
    // the search grid: over the centroids' own bounds
    float mn[3], mx[3];
    if (const int e = result_bounds(c, ix.bounds, mn, mx)) return e;
    const ClusterGrid grid = normals_grid(q.search_cell, c->plan.params.leaf, q.k, mn, mx, CM_ROW_TABLE_CAP);
    if (const int e = build_search_index(c, ix, grid, mn, "cannot allocate the normal estimation's row table")) return e;
    const PairSort& so = ix.sort;

    // the neighbourhoods and the planes: the 3x3x3 cells first, then whoever needs more, ring by ring
    prof_mark(c, "k_nrm_knn(block)");
    cmk_nrm_knn(st, ix.state, so.keys_a, so.keys_b, ix.pts, ix.rows, c->out, ix.grid, n, q.k, q.viewpoint, c->nrm_entries, c->nrm_list, w,
                n, true);
    HIP_TRY(c, hipGetLastError());
    uint32_t listed = 0;
    HIP_TRY(c, hipMemcpyAsync(&listed, w, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (listed > n) return fail(c, CM_INTERNAL, "normals: the first search launch listed more centroids than the result holds");
    if (listed) {
        char name[24];                                    // (the stage's name carries the length of its list: 24 bytes with the NUL)
        std::snprintf(name, sizeof name, "k_nrm_rings n=%u", listed);
        prof_mark(c, name);
        cmk_nrm_knn(st, ix.state, so.keys_a, so.keys_b, ix.pts, ix.rows, c->out, ix.grid, n, q.k, q.viewpoint, c->nrm_entries, c->nrm_list,
                    w, listed, false);
    }
    prof_mark(c, "end");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    collect_stage_times(c);
    c->nrm_n_listed = listed;
    c->nrm_have = true;
    c->nrm_k = q.k;
    return CM_OK;
}

namespace {

// What align's and ndt's parameters share, and what their outcomes share.
struct FitParams {
    uint32_t max_iterations, min_correspondences;
    double rot_eps, trans_eps;
};
struct FitOutcome {
    double s[CM_ALIGN_SUMS];             // H (21), g (6), the error sum, then the bits of n_corr: the final evaluation's
    uint64_t n_corr;
    uint32_t iterations, flags;          // flags: CM_ALIGN_*, whose four meanings are CM_NDT_*'s (cm_api.cpp asserts it)
};

// The Gauss-Newton loop of a registration: up to max_iterations times evaluate, solve, update `pose` about `pivot`
// (cm_align_solve.hpp), then one evaluation at the final pose, whose sums *o holds. launch(P) enqueues one evaluation of the
// n_src source records at the pose P: the correspondences into fit.corr, the per-block sums into fit.part; k_aln_sum and one
// host round trip of 28 doubles and a count follow (readback: that stage's name). Under CM_FLAG_PROFILE the stage times of
// the call replace the frame's, one entry per name, summed over the evaluations.
template <class Launch>
int fit_pose(cm_ctx* c, PoseFit& fit, const FitParams& q, uint32_t n_src, double pose[12], const double pivot[3], Launch&& launch,
             const char* readback, FitOutcome* o) {
    hipStream_t st = c->stream;
    const uint32_t n_blocks = (n_src + CM_BLOCK - 1) / CM_BLOCK;
    double* const s = o->s;
    auto evaluate = [&]() -> int {
        CmAlignPoseDev P;
        std::memcpy(P.m, pose, sizeof P.m);
        std::memcpy(P.p0, pivot, sizeof P.p0);
        launch(P);
        prof_mark(c, "k_aln_sum");
        cmk_aln_sum(st, fit.part, n_blocks, fit.sums);
        prof_mark(c, readback);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(s, fit.sums, sizeof o->s, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        std::memcpy(&o->n_corr, &s[CM_ALIGN_TERMS], 8);
        return CM_OK;
    };
    uint32_t flags = 0, it = 0;
    for (; it < q.max_iterations; ++it) {
        if (const int e = evaluate()) return e;
        if (o->n_corr < q.min_correspondences) break;
        double x[6];
        if (!cm_align_solve(s, s + 21, x)) { flags |= CM_ALIGN_SINGULAR; break; }
        cm_align_update(pose, x, pivot);
        if (cm_align_norm3(x) < q.rot_eps && cm_align_norm3(x + 3) < q.trans_eps) { flags |= CM_ALIGN_CONVERGED; ++it; break; }
    }
    o->iterations = it;
    if (q.max_iterations && it == q.max_iterations && !(flags & CM_ALIGN_CONVERGED)) flags |= CM_ALIGN_MAX_ITER_HIT;
    if (const int e = evaluate()) return e;
    prof_mark(c, "end");
    if (c->flags & CM_FLAG_PROFILE) HIP_TRY(c, hipStreamSynchronize(st));
    collect_stage_times_by_name(c);
    if (o->n_corr < q.min_correspondences) flags |= CM_ALIGN_FEW;
    o->flags = flags;
    fit.have = true;
    fit.n_src = n_src;
    return CM_OK;
}

}  // namespace

// Point-to-plane registration of a source cloud against the last result (cm_kernels_align.hip; the semantics are in
// include/cloudmerge.h). The normals table first: the one the context holds for this result at normals_k, else normals()
// with viewpoint 0 and search_cell 0. Then the search index over cluster_grid of the matching radius, once per call; the
// bounds also give the pivot. Then the loop (fit_pose), per evaluation k_aln_eval. Reads `out` and nrm_entries. The stage
// times are without those of a normals call it made; "aln_readback" is the round trip with the host's solve.
int align(cm_ctx* c, const cm_align_params& q, const void* src_dev, uint64_t n_src64, cm_align_result* out) {
    const uint32_t n = static_cast<uint32_t>(c->result.n_out);
    const uint32_t n_src = static_cast<uint32_t>(n_src64);
    SearchIndex& ix = c->aln;
    PoseFit& fit = c->aln_fit;
    fit.have = false;
    std::memset(out, 0, sizeof *out);
    std::memcpy(out->pose, q.guess, sizeof out->pose);
    HIP_TRY(c, hipSetDevice(c->device));
    if (n && !(c->nrm_have && c->nrm_k == q.normals_k)) {
        cm_normal_params np{};
        np.k = q.normals_k;
        if (const int e = normals(c, np)) return e;
    }
    if (const int e = reserve_search_index(c, ix, 1, "cannot allocate the registration's search buffers",
                                           "cannot allocate the registration's state")) return e;
    if (const int e = fit.reserve(c, n_src64, sizeof(cm_align_corr), "cannot allocate the registration's state",
                                  "cannot allocate the registration's correspondence table")) return e;
    c->prof_used = 0;

    CmClusterGridDev gd{};
    if (n) {
        // the search grid: over the centroids' own bounds, whose midpoint is the pivot
        float mn[3], mx[3];
        if (const int e = result_bounds(c, ix.bounds, mn, mx)) return e;
        bounds_midpoint(mn, mx, out->pivot);
        const ClusterGrid grid = cluster_grid(q.max_corr_dist, mn, mx, CM_ROW_TABLE_CAP);
        if (const int e = build_search_index(c, ix, grid, mn, "cannot allocate the registration's row table")) return e;
        HIP_TRY(c, hipGetLastError());
        gd = ix.grid;
    }

    const float r2 = q.max_corr_dist * q.max_corr_dist;
    const PairSort& so = ix.sort;
    FitOutcome o{};
    const int e = fit_pose(c, fit, {q.max_iterations, q.min_correspondences, q.rot_eps, q.trans_eps}, n_src, out->pose, out->pivot,
                           [&](const CmAlignPoseDev& P) {
                               prof_mark(c, "k_aln_eval");
                               cmk_aln_eval(c->stream, ix.state, so.keys_a, so.keys_b, ix.pts, ix.rows, c->out, c->nrm_entries, src_dev,
                                            n_src, n, gd, r2, P, fit.corr, fit.part);
                           },
                           "aln_readback", &o);
    out->iterations = o.iterations;          // (an evaluation that failed leaves the updates applied so far)
    if (e != CM_OK) return e;
    std::memcpy(out->H, o.s, sizeof out->H);
    std::memcpy(out->g, o.s + 21, sizeof out->g);
    out->sse = o.s[27];
    out->rms = o.n_corr ? std::sqrt(o.s[27] / static_cast<double>(o.n_corr)) : 0.0;
    out->n_corr = o.n_corr;
    out->flags = o.flags;
    return CM_OK;
}

// NDT registration of a source cloud against the last result's covariance table (cm_kernels_ndt.hip; the semantics are in
// include/cloudmerge.h). The table first: the one the context holds for this result at these parameters, else voxel_cov().
// Then k_cl_bounds on the result for the pivot, one round trip per call. Then align()'s loop (fit_pose), per evaluation
// k_ndt_eval. Reads `out`, out_key and cov_entries. Among the stage times "voxel_cov" is the covariance call it made (absent
// when the table was held), "ndt_readback" the round trip with the host's solve.
int ndt(cm_ctx* c, const cm_ndt_params& q, const cm_cov_params& cov, const void* src_dev, uint64_t n_src64, cm_ndt_result* out) {
    const uint32_t n = static_cast<uint32_t>(c->result.n_out);
    const uint32_t n_src = static_cast<uint32_t>(n_src64);
    PoseFit& fit = c->ndt_fit;
    fit.have = false;
    // the constants of the score, PCL's gauss_d1 / gauss_d2 at the frame's voxel volume
    const CmFrameDev& f = c->frame;
    const float* const leaf = c->plan.params.leaf;
    const double res3 = (static_cast<double>(leaf[0]) * static_cast<double>(leaf[1])) * static_cast<double>(leaf[2]);
    const double p = static_cast<double>(q.outlier_ratio);
    const double c1 = 10.0 * (1.0 - p), c2 = p / res3;
    const double d3 = -std::log(c2);
    const double d1 = -std::log(c1 + c2) - d3;
    const double d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / d1);
    if (!(std::isfinite(d2) && d2 > 0.0)) return fail(c, CM_BAD_ARG, "the score's d2 is not finite and > 0 at this outlier_ratio and leaf");
    const double d2h = d2 * 0.5;
    HIP_TRY(c, hipSetDevice(c->device));
    c->prof_used = 0;
    if (n && !(c->cov_have && c->cov_min_points == cov.min_points && c->cov_eig_mult == cov.eig_mult)) {
        prof_mark(c, "voxel_cov");                   // (there only when the call computed the table)
        if (const int e = voxel_cov(c, cov)) return e;
    }
    if (const int e = fit.reserve(c, n_src64, sizeof(cm_ndt_corr), "cannot allocate the NDT registration's state",
                                  "cannot allocate the NDT registration's correspondence table")) return e;
    if (!c->ndt_bounds.once(6)) return fail(c, CM_HIP_ERROR, "cannot allocate the NDT registration's state");
    // nothing is refused from here on: a refused call leaves *out as it was
    std::memset(out, 0, sizeof *out);
    std::memcpy(out->pose, q.guess, sizeof out->pose);
    out->gauss_d1 = d1;
    out->gauss_d2 = d2;

    CmCovGridDev g{};
    if (n) {
        // the pivot: the midpoint of the centroids' own bounds
        float mn[3], mx[3];
        if (const int e = result_bounds(c, c->ndt_bounds, mn, mx)) return e;
        bounds_midpoint(mn, mx, out->pivot);
        // the grid of out_key, as voxel_cov hands it to k_cov_keys
        for (int a = 0; a < 3; ++a) {
            g.inv[a] = f.inv_leaf[a];
            g.min_b[a] = c->cell_min_b[a];
            g.div_b[a] = static_cast<uint32_t>(c->cell_div_b[a]);
        }
    }

    FitOutcome o{};
    const int e = fit_pose(c, fit, {q.max_iterations, q.min_correspondences, q.rot_eps, q.trans_eps}, n_src, out->pose, out->pivot,
                           [&](const CmAlignPoseDev& P) {
                               prof_mark(c, "k_ndt_eval");
                               cmk_ndt_eval(c->stream, c->out_key, n, c->cov_entries, src_dev, n_src, g, q.neighborhood, d2h, P, fit.corr,
                                            fit.part);
                           },
                           "ndt_readback", &o);
    out->iterations = o.iterations;          // (an evaluation that failed leaves the updates applied so far)
    if (e != CM_OK) return e;
    std::memcpy(out->H, o.s, sizeof out->H);
    std::memcpy(out->g, o.s + 21, sizeof out->g);
    out->score = o.s[27];
    out->n_corr = o.n_corr;
    out->flags = o.flags;
    return CM_OK;
}
