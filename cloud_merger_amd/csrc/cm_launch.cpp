// cm_launch.cpp — frame assembly and the frame's launch sequences: the general path (cm_kernels.hip, with the ground and
// outlier pre-stages), the bucket path's fixed-grid and quantile passes (cm_kernels_v2/v3/v4.hip), the replays of a frame the
// bucket path hands back, and the table merge. Which route a frame takes is decided in cm_route.cpp: everything here reads
// c->plan. What is computed from a result afterwards, on request, is cm_byproducts.cpp's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "cm_ctx.hpp"

void prof_mark(cm_ctx* c, const char* name) {
    if (!(c->flags & CM_FLAG_PROFILE)) return;
    if (c->prof_used >= c->prof_ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->prof_ev.push_back(e);
        c->prof_names.emplace_back();
    }
    c->prof_names[c->prof_used] = name;
    (void)hipEventRecord(c->prof_ev[c->prof_used], c->stream);
    ++c->prof_used;
}

namespace {

// Records c->frame as the descriptor HBM holds. true: it differs from the one uploaded last, and the caller uploads it (or
// hands do_setup to a first pass that does).
bool descriptor_changed(cm_ctx* c) {
    if (c->frame_uploaded_valid && std::memcmp(&c->frame, &c->frame_uploaded, sizeof c->frame) == 0) return false;
    c->frame_uploaded = c->frame;
    c->frame_uploaded_valid = true;
    return true;
}

// Group-total arrays of the radix passes. The two pass-0 arrays alternate per launch of a first pass (k_keys, k2_hist0,
// kg_classify, k_table_keys): it accumulates into one and clears the other for the next launch. Passes 1..3 live behind
// them at stride gw (cleared by the first pass, filled by the histogram passes).
struct GrpArrays {
    uint32_t *p0, *p0_next, *rest;
    uint32_t stride;                 // words of one pass-0 array
    uint32_t gw;                     // words the frame in c->frame uses of one array
};

GrpArrays next_grp(cm_ctx* c) {
    const size_t gstride = static_cast<size_t>(c->cap_groups) * CM_RADIX;
    const uint32_t par = c->frame_seq++ & 1u;
    return {c->grp + gstride * par, c->grp + gstride * (par ^ 1u), c->grp + 2 * gstride, static_cast<uint32_t>(gstride),
            (c->frame.n_tiles + CM_GROUP - 1) / CM_GROUP * CM_RADIX};
}

// The last launch of a frame is enqueued: cm_wait waits for ev_done.
int end_frame(cm_ctx* c) {
    prof_mark(c, "end");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_done, c->stream));
    c->cur ^= 1;
    c->pending = true;
    c->pending_trivial = false;
    return CM_OK;
}

}  // namespace

void frame_on_device(cm_ctx* c) {
    if (!c->frame.n_padded) return;                    // (an empty frame has no tiles: its readers launch nothing)
    if (descriptor_changed(c)) cmk_setup(c->stream, c->frame, c->d_frame, c->d_tiles);
}

void radix_sort_pairs(cm_ctx* c, CmFrameState* st, const SortPairs& b, uint32_t n_pass, uint32_t nt, uint32_t n_slots,
                      bool lds_rank, uint32_t* tile_kept, const char* scatter_mark) {
    const uint32_t n_groups = (nt + CM_GROUP - 1) / CM_GROUP, gw = n_groups * CM_RADIX;
    const bool big = n_groups > CM_DIRECT_GROUPS;
    auto mark = [&](const char* name) { if (scatter_mark) prof_mark(c, name); };
    for (uint32_t pass = 0; pass < n_pass; ++pass) {
        const bool even = (pass & 1u) == 0;
        const uint32_t* kin = even ? b.keys_a : b.keys_b;
        const uint32_t* vin = even ? b.vals_a : b.vals_b;
        uint32_t* kout = even ? b.keys_b : b.keys_a;
        uint32_t* vout = even ? b.vals_b : b.vals_a;
        uint32_t* grp = pass == 0 ? b.grp0 : b.grp_rest + static_cast<size_t>(pass - 1) * gw;
        if (pass > 0) { mark("k_hist"); cmk_hist(c->stream, st, kin, b.hist, grp, pass, nt); }
        if (big) { mark("k_gscan"); cmk_gscan(c->stream, st, grp, b.totals, pass, n_groups); }
        mark(scatter_mark);
        cmk_scatter(c->stream, st, kin, vin, kout, vout, b.hist, grp, big ? b.totals : nullptr, pass, nt, n_groups, n_slots,
                    lds_rank, tile_kept);
    }
}

namespace {

// The record passes of the bucket kernels behind k2_hist0 — the voxel stage, or the outlier stage's sort by the radius
// grid: pass p scatters by the key bits low + 8 p; the passes behind the first run over grids of nt_later tiles. The
// arguments from mask on are cmk2_scatter's (pack, sparse: pass 0 only; misrank: the last pass only).
void record_passes(cm_ctx* c, CmFrameState* state, const GrpArrays& gr, uint32_t g, uint32_t low, uint32_t nt_later,
                   const unsigned char* mask, int use_cell, int fold, bool pack, bool sparse, bool misrank, bool ballot,
                   uint32_t* tile_kept, const char* scatter_mark) {
    const CmFrameDev& f = c->frame;
    const uint32_t nt = f.n_tiles, n_groups = (nt + CM_GROUP - 1) / CM_GROUP, n_groups_later = (nt_later + CM_GROUP - 1) / CM_GROUP;
    for (uint32_t pass = 0; pass < g; ++pass) {
        uint32_t* grp = pass == 0 ? gr.p0 : gr.rest + static_cast<size_t>(pass - 1) * gr.gw;
        const uint32_t nt_p = pass == 0 ? nt : nt_later, n_groups_p = pass == 0 ? n_groups : n_groups_later;
        const bool big_p = n_groups_p > CM_DIRECT_GROUPS;
        if (pass > 0) { prof_mark(c, "k2_hist"); cmk2_hist(c->stream, state, c->dig, c->hist, grp, nt_p); }
        if (big_p) { prof_mark(c, "k_gscan"); cmk_gscan(c->stream, state, grp, c->totals, pass, n_groups_p); }
        prof_mark(c, scatter_mark);
        cmk2_scatter(c->stream, pass == 0, c->d_frame, c->d_tiles, state, (pass & 1u) ? c->rec_a : c->rec_b,
                     (pass & 1u) ? c->rec_b : c->rec_a, c->dig, c->hist, grp, big_p ? c->totals : nullptr, low + 8 * pass,
                     pass + 1 < g ? low + 8 * (pass + 1) : 32u, nt_p, n_groups_p, f.n_padded, c->records, nt, fold, mask, use_cell,
                     (pack && pass == 0) ? c->rec_b : nullptr, c->wave_cnt, (misrank && pass + 1 == g) ? 1 : 0, tile_kept,
                     sparse && pass == 0, ballot);
    }
}

int bootstrap_box(cm_ctx* c) {
    if (descriptor_changed(c)) cmk_setup(c->stream, c->frame, c->d_frame, c->d_tiles);
    float mn[3], mx[3], leaf[3];
    uint64_t cnt = 0;
    const int e = measure_bounds(c, c->frame.n_tiles, mn, mx, &cnt);
    if (e != CM_OK) return e;
    c->route.pred.ok = false;
    if (cnt) {
        for (int a = 0; a < 3; ++a) leaf[a] = 1.0f / c->frame.inv_leaf[a];
        c->route.set_predicted_box(mn, mx, leaf);
    }
    return CM_OK;
}

int bucket_buffers(cm_ctx* c) {
    const size_t npad = c->cap_padded, nt = c->cap_tiles, nt4 = std::min<uint32_t>(c->cap_tiles, CM4_MAX_TILES);
    const bool ok = c->rec_a.once(npad * 16) && c->rec_b.once(npad * 16) && c->dig.once(npad) && c->tile_state.once(npad / 1024 + 2) &&
                    c->records.once(nt * 8) && c->wave_cnt.once(nt * CM2_WAVES) &&
                    // the quantile passes'
                    c->spl[0].once(CM4_MAX_BUCKETS + 4) && c->spl[1].once(CM4_MAX_BUCKETS + 4) && c->qcnt.once(nt4 * (CM4_BINS / 2)) &&
                    c->qtot.once(CM4_BINS) && c->qbid.once(nt4 * CM_TILE) && c->qbofs.once(CM4_BINS + 4) && c->qbig.once(CM4_MAX_BIG + 4);
    return ok ? CM_OK : fail(c, CM_HIP_ERROR, "cannot allocate the bucket path's buffers");
}

// The bucket path's voxel stage for the frame in c->frame as c->plan has it: the quantile passes, or pl.g fixed-grid 8-bit
// passes over the key bits above pl.low, then the local finish. mask / st_outlier: what the pre-stages left.
int launch_bucket(cm_ctx* c, const unsigned char* mask, const CmFrameState* st_outlier) {
    const FramePlan& pl = c->plan;
    CmFrameDev& f = c->frame;
    hipStream_t st = c->stream;
    { const int e = bucket_buffers(c); if (e != CM_OK) return e; }
    // (a descriptor that changed since the last frame — new clouds, new poses — goes to HBM with the first pass itself)
    const bool do_setup = descriptor_changed(c);
    CmFrameState* state = c->d_state[c->cur];
    CmFrameState* state_next = c->d_state[c->cur ^ 1];
    c->from_crop = pl.b_grid_mode == 1 || (pl.b_grid_mode == 2 && !pl.predicted);
    c->frame_mask = mask;
    const uint32_t nt = f.n_tiles;
    const bool ballot = !c->route.lds_rank;        // ranks by ballots where the returning LDS adds are not (known to be) lane-ordered
    uint32_t* skey = c->out_key ? c->keys_a : nullptr;
    if (pl.quant) {
        // One global pass into the buckets the last frame's quantiles cut (cm_kernels_v4.hip), one finish workgroup per bucket.
        const uint32_t nb = pl.nb, sub = pl.sub;
        const uint32_t nbins = (nb + (1u << sub) - 1u) >> sub;
        const uint32_t* spl = c->spl[c->route.spl_cur];
        uint32_t* spl_next = c->spl[c->route.spl_cur ^ 1];
        prof_mark(c, "k4_hist");
        cmk4_hist(st, f, c->d_frame, c->d_tiles, do_setup, state, spl, c->qcnt, c->qbid, c->tile_state, pl.n_tile_state, c->records,
                  pl.b_grid_mode, pl.predicted ? 1 : 0, nt, nb, sub ? nullptr : c->qbig, sub, c->hist_resident);
        prof_mark(c, "k4_colscan");
        // (shared bins: a bin beyond 2^sub finish capacities holds a bucket beyond one; the finish itself checks the buckets)
        if (sub) cmk4_colscan(st, state, c->h_state_dev, c->qcnt, c->qtot, nt, CM4_CAP << sub, CM4_CAP << sub, nullptr);
        else cmk4_colscan(st, state, c->h_state_dev, c->qcnt, c->qtot, nt, CM4_CAP, pl.big_armed ? CM4_CAP_BIG : CM4_CAP, c->qbig);
        prof_mark(c, "k4_scatter");
        cmk4_scatter(st, c->d_frame, c->d_tiles, state, c->qbid, c->qcnt, c->qtot, c->qbofs, nbins, c->rec_a, c->records, nt,
                     pl.predicted ? 1 : 0, c->d_tile_kept, nt, sub ? c->dig : nullptr, ballot, sub ? nullptr : c->qbig, sub);
        // (tile_info: one word pair per bucket; the group totals of the kept voxels behind them — pl.n_tile_state words)
        uint32_t* grp_cnt = reinterpret_cast<uint32_t*>(c->tile_state + nb);
        prof_mark(c, "k3_local");
        cmk3_local(st, c->d_frame, state, c->h_state_dev, c->rec_a, c->tile_state, grp_cnt, c->rec_b, skey, c->vals_a, false, 0u,
                   0u, spl, c->qbofs, nb, spl_next, ballot, sub, sub ? c->dig : nullptr);
        if (pl.big_armed) {
            // the few buckets that grew beyond what the usual finish workgroup holds (k4_colscan listed them): the large shape
            prof_mark(c, "k3_local(big)");
            cmk3_local_big(st, c->d_frame, state, c->h_state_dev, c->rec_a, c->tile_state, grp_cnt, c->rec_b, skey, c->vals_a, spl,
                           c->qbofs, nb, spl_next, c->qbig, ballot);
        }
        prof_mark(c, "k3_compact");
        cmk3_compact(st, state, state_next, c->h_state_dev, c->tile_state, grp_cnt, c->rec_b, skey, c->vals_a, c->out, c->out_key,
                     c->out_cnt, false, 0u, nb);
        return end_frame(c);
    }
    if (pl.mode == 1 && !ensure_partial(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the partial table");
    const GrpArrays g = next_grp(c);
    prof_mark(c, "k2_hist0");
    cmk2_hist0(st, f, c->d_frame, c->d_tiles, do_setup, state, c->hist, g.p0, g.p0_next, g.rest, g.gw, g.stride, c->tile_state,
               f.n_padded / 1024 + 2, c->records, pl.b_grid_mode, pl.predicted ? 1 : 0, pl.low, pl.g, nt, mask, st_outlier, 0,
               pl.pack ? c->rec_b : nullptr, c->wave_cnt);
    record_passes(c, state, g, pl.g, pl.low, pl.nt_later, mask, 0, pl.predicted ? 1 : 0, pl.pack, pl.sparse,
                  c->route.debug_misrank != 0, ballot, c->d_tile_kept, "k2_scatter");
    const void* rec_sorted = ((pl.g - 1) & 1u) ? c->rec_b : c->rec_a;
    if (pl.k3) {
        // k3_local stages every tile's centroids in the record buffer the last pass read from (dead by now), at the
        // tile's own place; k3_compact moves them to `out`. Cells and counts (CM_FLAG_OCCUPANCY) ride in the general
        // path's key / value arrays, which the bucket path does not use.
        void* stage = ((pl.g - 1) & 1u) ? c->rec_a : c->rec_b;
        if (pl.mode == 1) {
            if (!c->stage32.once(static_cast<size_t>(c->cap_padded) * 32)) return fail(c, CM_HIP_ERROR, "cannot allocate the partial table's staging");
            stage = c->stage32;
        }
        uint32_t* grp_cnt = reinterpret_cast<uint32_t*>(c->tile_state + f.n_padded / 2048);
        prof_mark(c, "k3_local");
        // (the finish also leaves the quantiles of its sorted records: the next frame's splitters, cm_kernels_v4.hip; with
        // L = 0 a tile's sorted range may reach beyond what it holds in LDS — the frame then says so: CmFrameState.spl_incomplete)
        uint32_t* spl_next = pl.mode == 0 ? c->spl[c->route.spl_cur ^ 1] : nullptr;
        cmk3_local(st, c->d_frame, state, c->h_state_dev, rec_sorted, c->tile_state, grp_cnt, stage, skey, c->vals_a, pl.mode == 1,
                   pl.low, pl.nt_later * CM_TILE, nullptr, nullptr, 0u, spl_next, ballot);
        prof_mark(c, "k3_compact");
        cmk3_compact(st, state, state_next, c->h_state_dev, c->tile_state, grp_cnt, stage, skey, c->vals_a,
                     pl.mode == 1 ? c->partial : c->out, c->out_key, c->out_cnt, pl.mode == 1, pl.nt_later * CM_TILE);
    } else {
        prof_mark(c, "k2_local");
        cmk2_local(st, c->d_frame, state, state_next, c->h_state_dev, rec_sorted, c->tile_state,
                   reinterpret_cast<uint32_t*>(c->tile_state + (f.n_padded / 1024 + 1)), c->out, c->out_key, c->out_cnt,
                   pl.mode == 1 ? c->partial : nullptr, pl.low, f.n_padded);
    }
    return end_frame(c);
}

// Keys + radix sort of one stage of the general path (the voxel grid, or the outlier stage's radius grid).
void keys_and_sort(cm_ctx* c, CmFrameState* stg, int gmode, int use_cell, const unsigned char* mask,
                   const CmFrameState* st_outlier, uint32_t n_pass) {
    const CmFrameDev& f = c->frame;
    const uint32_t nt = f.n_tiles;
    const uint32_t n_seg_groups = (f.n_padded / CM_SEG_TILE + CM_SEG_GROUP - 1) / CM_SEG_GROUP + 1;
    const uint32_t n_partials = nt < CM_MINMAX_BLOCKS ? nt : CM_MINMAX_BLOCKS;
    const GrpArrays g = next_grp(c);
    prof_mark(c, use_cell ? "k_keys(outlier)" : "k_keys");
    cmk_keys(c->stream, c->d_frame, stg, c->keys_a, c->hist, g.p0, g.p0_next, g.rest, g.gw, g.stride, c->seg_groups, n_seg_groups,
             c->partials, n_partials, gmode, use_cell, mask, st_outlier, nt);
    radix_sort_pairs(c, stg, {c->keys_a, c->keys_b, c->vals_a, c->vals_b, c->hist, c->totals, g.p0, g.rest}, n_pass, nt, f.n_padded,
                     c->route.lds_rank, use_cell ? nullptr : c->d_tile_kept, "k_scatter");
}

// The outlier stages' sort: the points `in` marks (nullptr: every valid point) by the grid of f.inv_cell, into d_state_o
// and (bucket kernels) sorted_pts. *gathered: the bucket kernels left the points in sorted order already.
int cell_sort(cm_ctx* c, const unsigned char* in, bool* gathered) {
    const FramePlan& pl = c->plan;
    const CmFrameDev& f = c->frame;
    hipStream_t st = c->stream;
    if (!ensure_cell_sort(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the outlier stage's buffers");
    HIP_TRY(c, hipMemsetAsync(c->d_state_o, 0, sizeof(CmFrameState), st));
    const uint32_t nt = f.n_tiles, g = pl.g_o;
    if (g) {
        // Bucket kernels on the radius grid: records (x, y, z, padded index) grouped by the high key bits in g
        // passes, then sorted tile by tile in LDS and written back in order — what the general path's (key, index)
        // sort + gather produce, in fewer passes over less data. A radius cell too full for a tile hands the
        // frame back (CM_DEV_ERR_BUCKET_PRE).
        { const int e = bucket_buffers(c); if (e != CM_OK) return e; }
        const uint32_t low = pl.kb_o > 8 * g ? pl.kb_o - 8 * g : 0;
        const GrpArrays gr = next_grp(c);
        prof_mark(c, "k2_hist0(outlier)");
        cmk2_hist0(st, f, c->d_frame, c->d_tiles, false, c->d_state_o, c->hist, gr.p0, gr.p0_next, gr.rest, gr.gw, gr.stride,
                   c->tile_state, f.n_padded / 1024 + 2, c->records, 1, 0, low, g, nt, in, nullptr, 1, pl.pack_o ? c->rec_b : nullptr,
                   c->wave_cnt);
        record_passes(c, c->d_state_o, gr, g, low, nt, in, 1, 0, pl.pack_o, false, false, false, nullptr, "k2_scatter(outlier)");
        prof_mark(c, "k2_local(sort)");
        cmk2_local_sort(st, c->d_frame, c->d_state_o, c->h_state_dev, ((g - 1) & 1u) ? c->rec_b : c->rec_a,
                        (g & 1u) ? c->keys_b : c->keys_a, c->sorted_pts, low, f.n_padded);
    } else {
        if (!pl.gm_o) {
            prof_mark(c, "k_minmax");
            cmk_minmax(st, c->d_frame, c->partials, nt < CM_MINMAX_BLOCKS ? nt : CM_MINMAX_BLOCKS, in);
        }
        keys_and_sort(c, c->d_state_o, pl.gm_o, 1, in, nullptr, pl.gm_o ? (pl.kb_o + CM_RADIX_BITS - 1) / CM_RADIX_BITS : CM_MAX_PASSES);
    }
    *gathered = g != 0;
    return CM_OK;
}

// Radius outlier filter over the points `in` marks (nullptr: every valid point), neighbours counted inside a
// point's class only when `cls` is given; survivors are marked in `out`.
int radius_filter(cm_ctx* c, const unsigned char* in, const unsigned char* cls, unsigned char* out) {
    bool gathered = false;
    const int e = cell_sort(c, in, &gathered);
    if (e != CM_OK) return e;
    prof_mark(c, "outlier_mask");
    cmk_outlier_mask(c->stream, c->d_frame, c->d_state_o, c->keys_a, c->vals_a, c->keys_b, c->vals_b, c->sorted_pts,
                     c->rows, out, c->frame.n_padded, cls, c->merged_total + 8, gathered);
    return CM_OK;
}

// Statistical outlier removal over every valid point: the sort by the search grid, the row table, the
// k-nearest-neighbour search, the exact statistics and the keep-mask (c->mask, zeroed by the caller).
int sor_filter(cm_ctx* c) {
    const CmFrameDev& f = c->frame;
    hipStream_t st = c->stream;
    bool gathered = false;
    const int e = cell_sort(c, nullptr, &gathered);
    if (e != CM_OK) return e;
    prof_mark(c, "sor_rows");
    cmk_sorted_rows(st, c->d_frame, c->d_state_o, c->keys_a, c->vals_a, c->keys_b, c->vals_b, c->sorted_pts, c->rows,
                    f.n_padded, gathered);
    HIP_TRY(c, hipMemsetAsync(c->sor_d, 0xFF, static_cast<size_t>(f.n_padded) * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->sor_words, 0, CM_SOR_WORD_STATS * 8, st));
    const cm_sor_params& q = c->plan.sor_p;          // (a set call after the enqueue does not reach this frame or its redo)
    const uint32_t k = q.mean_k;
    prof_mark(c, "k_sor_knn");
    cmk_sor_knn(st, c->d_frame, c->d_state_o, c->keys_a, c->keys_b, c->sorted_pts, c->rows, c->sor_d, c->sor_list, c->sor_words,
                f.n_padded, k, true);
    prof_mark(c, "k_sor_knn(list)");
    cmk_sor_knn(st, c->d_frame, c->d_state_o, c->keys_a, c->keys_b, c->sorted_pts, c->rows, c->sor_d, c->sor_list, c->sor_words,
                f.n_padded, k, false);
    prof_mark(c, "k_sor_bins");
    cmk_sor_bins(st, c->d_state_o, c->sor_d, c->sor_words, f.n_padded);
    prof_mark(c, "k_sor_threshold");
    cmk_sor_threshold(st, c->d_state_o, c->sor_words, k, q.std_mul);
    prof_mark(c, "k_sor_mask");
    cmk_sor_mask(st, c->d_state_o, c->sor_d, c->sor_words, c->mask, f.n_padded);
    return CM_OK;
}

// The general path (cm_kernels.hip) for the frame in c->frame, behind the pre-stages; or only the pre-stages, when the
// bucket path takes the voxel stage (pl.post_bucket).
int launch_classic(cm_ctx* c) {
    const FramePlan& pl = c->plan;
    CmFrameDev& f = c->frame;
    hipStream_t st = c->stream;
    if (descriptor_changed(c)) { prof_mark(c, "k_setup"); cmk_setup(st, f, c->d_frame, c->d_tiles); }
    CmFrameState* state = c->d_state[c->cur];
    CmFrameState* state_next = c->d_state[c->cur ^ 1];
    c->from_crop = pl.grid_mode != 0;
    const bool ground_outl = c->ground_on && pl.mode == 0 && c->ground_outlier_radius > 0.0f;
    c->frame_mask = nullptr;
    c->frame_had_ground = false;
    const uint32_t nt = f.n_tiles, nseg = f.n_padded / CM_SEG_TILE;
    if (c->ground_on && pl.mode == 0) {
        // Zone-wise ground removal first (per sensor, before the fuse): it leaves a keep-mask for the voxel
        // grid and the fused no-ground cloud, and a ground mask for the fused ground cloud.
        const size_t npad = c->cap_padded, nz = CM_DEV_MAX_SENSORS * CM_DEV_MAX_ZONES, nh = nz * CM_GROUND_BATCH;
        const bool ok = ensure_mask(c) && c->gmask.once(npad) && ensure_sorted_pts(c) && c->d_ground.once(1) && c->d_state_g.once(1) &&
                        c->zone_off.once(nz + 1) && c->d_planes.once(nz) && c->hyp0.once(nh * 16) && c->valid0.once(nh) &&
                        c->counts0.once(nh) && c->chunk_sums.once((npad / CM_GROUND_CHUNK + nz + 1) * 10) &&
                        (!ground_outl || (c->bmask.once(npad) && c->zcode.once(npad)));
        if (!ok) return fail(c, CM_HIP_ERROR, "cannot allocate the ground stage's buffers");
        if (!c->ground_uploaded) { cmkg_setup(st, c->ground, c->d_ground); c->ground_uploaded = true; }
        // (masks and the slab sort's state cleared by ONE launch: they were five hipMemsetAsync calls per tick)
        prof_mark(c, "kg_clear");
        cmkg_clear(st, f.n_padded, c->mask, 0, c->gmask, 0, ground_outl ? c->bmask : nullptr, 0, ground_outl ? c->zcode : nullptr, 0xFF,
                   c->d_state_g, nullptr);
        const GrpArrays g = next_grp(c);
        prof_mark(c, "kg_classify");
        cmkg_classify(st, c->d_frame, c->d_ground, c->d_state_g, c->keys_a, c->hist, g.p0, g.p0_next, g.rest, g.gw, g.stride, c->mask,
                      ground_outl ? c->zcode : nullptr, nt);
        radix_sort_pairs(c, c->d_state_g, {c->keys_a, c->keys_b, c->vals_a, c->vals_b, c->hist, c->totals, g.p0, g.rest}, 1, nt,
                         f.n_padded, c->route.lds_rank, nullptr, "k_scatter(slabs)");
        prof_mark(c, "kg_ransac");
        cmkg_planes(st, c->d_frame, c->d_ground, c->d_state_g, c->keys_b, c->vals_b, c->sorted_pts, c->zone_off, c->hyp0,
                    c->valid0, c->counts0, c->chunk_sums, c->d_planes, ground_outl ? c->bmask : c->mask, c->gmask, f.n_padded);
        if (ground_outl) {
            // removeGround's outlierRemoval(no_ground_cloud_ptr) (:119): among the band points of a slab that are
            // not ground, those with no neighbour within the radius go; survivors join the keep-mask
            const int e = radius_filter(c, c->bmask, c->zcode, c->mask);
            if (e != CM_OK) return e;
        }
        c->frame_mask = c->mask;
        c->frame_had_ground = true;
    }
    if (pl.outl) {
        // Radius outlier removal first: it decides which points the voxel grid sees at all.
        if (!ensure_mask(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the outlier stage's buffers");
        HIP_TRY(c, hipMemsetAsync(c->mask, 0, f.n_padded, st));
        const int e = radius_filter(c, nullptr, nullptr, c->mask);
        if (e != CM_OK) return e;
        c->frame_mask = c->mask;
    }
    if (pl.sor) {
        // Statistical outlier removal: like the radius stage, it decides which points the voxel grid sees at all.
        HIP_TRY(c, hipMemsetAsync(c->mask, 0, f.n_padded, st));
        const int e = sor_filter(c);
        if (e != CM_OK) return e;
        c->frame_mask = c->mask;
    }
    const CmFrameState* st_outlier = (pl.outl || ground_outl || pl.sor) ? c->d_state_o : nullptr;
    if (pl.post_bucket) return launch_bucket(c, c->frame_mask, st_outlier);   // the voxel stage, with the keep-mask
    if (!c->from_crop) {
        prof_mark(c, "k_minmax");
        cmk_minmax(st, c->d_frame, c->partials, nt < CM_MINMAX_BLOCKS ? nt : CM_MINMAX_BLOCKS, c->frame_mask);
    }
    keys_and_sort(c, state, pl.grid_mode, 0, c->frame_mask, st_outlier,
                  c->from_crop ? (pl.key_bits + CM_RADIX_BITS - 1) / CM_RADIX_BITS : CM_MAX_PASSES);
    prof_mark(c, "k_seg_count");
    uint32_t* seg_groups = nseg > CM_SEG_DIRECT_TILES ? c->seg_groups : nullptr;
    cmk_seg_count(st, state, c->keys_a, c->keys_b, c->seg_tile_counts, seg_groups, pl.mode == 1 ? 1u : f.min_pts, nseg);
    prof_mark(c, "k_seg_reduce");
    if (pl.mode == 1 && !ensure_partial(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the partial table");
    cmk_seg_reduce(st, pl.mode, c->d_frame, state, state_next, c->h_state_dev, c->keys_a, c->vals_a, c->keys_b,
                   c->vals_b, c->seg_tile_counts, seg_groups, pl.mode == 1 ? c->partial : c->out, c->out_key,
                   c->out_cnt, nseg);
    return end_frame(c);                               // (k_seg_reduce wrote the state record to h_state)
}

// The frame again, after the bucket path handed it back (RouteState::settle says how). Its clouds are still where they
// were: a slot's active buffer is not written to before the next frame is enqueued, whatever the subscriber threads submit
// meanwhile.
int replay(cm_ctx* c, Replay how) {
    FramePlan& pl = c->plan;
    RouteState& rt = c->route;
    if (how == Replay::fixed_grid) {                   // stale splitters: the fixed-grid passes in the same box
        rt.size_fixed_grid(pl, c->frame, c->n_in);
        c->h_state->err = 0;
        c->prof_used = 0;
        return launch_bucket(c, nullptr, nullptr);
    }
    if (how == Replay::measured_box) {                 // a box miss and nothing else: the same path, in a box that fits
        // (everything that can still say "no" works on copies: a refusal leaves c->frame as the general path expects it)
        const Box pred0 = rt.pred;
        CmFrameDev f = c->frame;
        if (rt.measured_box(pl, f, *c->h_state, c->n_in)) {
            const CmFrameDev f0 = c->frame;
            c->frame = f;
            c->h_state->err = 0;
            c->prof_used = 0;
            if (launch_bucket(c, nullptr, nullptr) == CM_OK) return CM_OK;
            c->frame = f0;
            rt.pred = pred0;
        }
    }
    // every other cause, or a second hand-back: the general path, same descriptor
    c->prof_used = 0;
    pl.bucket = pl.post_bucket = pl.measured = pl.predicted = false;
    pl.g_o = 0;
    if (!c->frame.n_padded) return fail(c, CM_INTERNAL, "frame could not be redone");
    return launch_classic(c);
}

// The grid PCL itself would report for a frame sorted in the predicted box (same order): the cloud's exact bounds, which
// the frame also produced (A.4 steps 2, 4).
void exact_grid(const CmFrameState& h, const float inv_leaf[3], cm_result& r) {
    unsigned long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        const float lo = h.min_p[a] * inv_leaf[a], hi = h.max_p[a] * inv_leaf[a];
        r.min_b[a] = static_cast<int32_t>(std::floor(lo));
        r.max_b[a] = static_cast<int32_t>(std::floor(hi));
        r.div_b[a] = r.max_b[a] - r.min_b[a] + 1;
        cells *= static_cast<unsigned long long>(r.div_b[a]);
    }
    r.key_bits = key_width(cells);
}

}  // namespace

// Builds the frame descriptor: in c->frame, or for a peek in *peek. It is assembled in a local and stored once nothing can
// refuse the call any more: c->frame, c->n_in and c->n_sensors_used describe the last frame for as long as its result is
// served (the by-product calls read its clouds through them), so neither a refusal nor a peek may touch them.
int build_frame(cm_ctx* c, const cm_params* p, CmFrameDev* peek, std::vector<std::unique_lock<std::mutex>>& locks) {
    const bool consume = peek == nullptr;
    for (uint32_t s = 0; s < c->max_sensors; ++s) locks.emplace_back(c->slots[s].mu);

    // Frame assembly policy (pc_preprocessing_main.cpp:134-157).
    uint32_t have = 0, fresh = 0;
    for (uint32_t s = 0; s < c->max_sensors; ++s) {
        if (c->slots[s].has_data) have |= 1u << s;
        if (c->slots[s].fresh) fresh |= 1u << s;
    }
    const uint32_t required = p->required_sensor_mask ? p->required_sensor_mask : have;
    if (have == 0 || (required & ~fresh) != 0) return CM_NOT_READY;

    CmFrameDev f;
    std::memset(&f, 0, sizeof f);
    uint32_t base = 0, k = 0;
    uint64_t n_in = 0;
    // the clouds the frame will read: a slot's staged cloud if it has a fresh one, else the one its last frame read
    // (a stale optional sensor rides along like :141)
    for (uint32_t s = 0; s < c->max_sensors; ++s) {
        Slot& sl = c->slots[s];
        if (!sl.has_data) continue;
        const SlotCloud& sc = sl.fresh ? sl.staged : sl.active;
        const uint64_t nb = static_cast<uint64_t>(base) + round_up(sc.n, CM_TILE);
        if (nb > c->cap_padded) return fail(c, CM_CAPACITY, "frame exceeds cm_limits.max_points_total");
        if (c->motion_on && sl.time_type != CM_TIME_NONE && sc.n && static_cast<uint64_t>(sl.time_off) + 4u > sc.step)
            return fail(c, CM_BAD_ARG, "sensor " + std::to_string(s) + ": time field at byte " + std::to_string(sl.time_off) +
                                           " does not fit point_step " + std::to_string(sc.step));
        base = static_cast<uint32_t>(nb);
    }
    base = 0;
    if (consume) c->stats_n_sensors = 0;
    for (uint32_t s = 0; s < c->max_sensors; ++s) {
        Slot& sl = c->slots[s];
        if (!sl.has_data) continue;
        if (sl.fresh) {
            // an H2D copy enqueued without waiting (cm_submit_cloud_async): the frame's stream waits for it, not the host
            if (sl.copy_pending) HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.ev_copy, 0));
            if (consume) {                   // the frame takes the staged cloud over; submits now go to the other buffer
                sl.active = sl.staged;
                sl.active_buf = sl.staged.dptr == sl.buf[0] ? 0 : sl.staged.dptr == sl.buf[1] ? 1 : -1;
                sl.active_bytes_h2d = sl.bytes_h2d;
                sl.active_gen = sl.gen;
                sl.copy_pending = false;
            }
        }
        const SlotCloud& sc = (sl.fresh && !consume) ? sl.staged : sl.active;   // (!consume: cm_local_bounds' peek)
        CmSensorDev& d = f.s[k];
        d.data = static_cast<const unsigned char*>(sc.dptr);
        d.n = sc.n; d.base = base; d.point_step = sc.step; d.slot = s;
        d.off_x = sc.ox; d.off_y = sc.oy; d.off_z = sc.oz; d.off_i = sc.oi;
        const bool al16 = (reinterpret_cast<uintptr_t>(sc.dptr) & 15u) == 0;
        if (al16 && sc.step == 16 && sc.ox == 0 && sc.oy == 4 && sc.oz == 8 && sc.oi == 12) d.layout = CM_LAYOUT_XYZI16;
        else if (al16 && sc.step == 32 && sc.ox == 0 && sc.oy == 4 && sc.oz == 8 && sc.oi == 16) d.layout = CM_LAYOUT_PCL32;
        else d.layout = CM_LAYOUT_GENERIC;
        std::memcpy(d.m, sl.m, sizeof d.m);
        n_in += sc.n;
        if (consume) {
            c->frame_origin[k][0] = sl.m[3];         // what the frame is built with, whatever deskew does to d.m below
            c->frame_origin[k][1] = sl.m[7];
            c->frame_origin[k][2] = sl.m[11];
            c->stats_sensor[k] = s; c->stats_n[k] = sc.n;
            c->stats_fresh[k] = sl.fresh ? 1u : 0u;
            c->stats_bytes[k] = sl.fresh ? sl.active_bytes_h2d : 0u;
            c->stats_gen[k] = sl.active_gen;
            c->stats_n_sensors = k + 1;
        }
        ++k;
        base += round_up(sc.n, CM_TILE);
    }
    f.n_sensors = k;
    f.n_padded = base;
    f.n_tiles = base / CM_TILE;
    if (consume) c->last_motion = false;
    if (consume && c->motion_on && f.n_padded) {
        // Ego-motion compensation: one pre-pass over the raw clouds writes the compensated points at their padded indices,
        // then every sensor of the descriptor reads those — 16-byte records, identity matrix — and each route runs unchanged.
        const cm_motion& mo = c->motion;
        CmMotionDev md;
        std::memset(&md, 0, sizeof md);
        md.n_sensors = k;
        for (uint32_t j = 0; j < k; ++j) {
            md.s[j] = f.s[j];
            const Slot& sl = c->slots[f.s[j].slot];
            md.time_off[j] = sl.time_off;
            md.time_type[j] = sl.time_type;
            // (the difference of the stamps in 64 bits, wrapping rather than overflowing, then fp64 seconds rounded to fp32)
            const int64_t d = static_cast<int64_t>(static_cast<uint64_t>(mo.stamp_ns[f.s[j].slot]) - static_cast<uint64_t>(mo.t_ref_ns));
            md.dt0[j] = static_cast<float>(static_cast<double>(d) * 1e-9);
        }
        for (int a = 0; a < 3; ++a) { md.v[a] = mo.v[a]; md.w[a] = mo.w[a]; }
        md.k[0] = mo.w[1] * mo.v[2] - mo.w[2] * mo.v[1];       // k = w x v (fp32, no contraction: built with -ffp-contract=off)
        md.k[1] = mo.w[2] * mo.v[0] - mo.w[0] * mo.v[2];
        md.k[2] = mo.w[0] * mo.v[1] - mo.w[1] * mo.v[0];
        prof_mark(c, "k_motion");
        cmk_motion(c->stream, md, c->motion_buf, f.n_padded);
        static const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        for (uint32_t j = 0; j < k; ++j) {
            CmSensorDev& d = f.s[j];
            d.data = c->motion_buf + static_cast<size_t>(d.base) * 16;
            d.point_step = 16;
            d.off_x = 0; d.off_y = 4; d.off_z = 8; d.off_i = 12;
            d.layout = CM_LAYOUT_XYZI16;
            std::memcpy(d.m, identity, sizeof d.m);
        }
        c->last_motion = true;
    }
    f.crop_enable = p->crop_enable ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        f.crop_min[a] = p->crop_min[a];
        f.crop_max[a] = p->crop_max[a];
        f.inv_leaf[a] = 1.0f / p->leaf[a];          // Array4f::Ones() / leaf_size_: fp32 division
    }
    f.min_pts = p->min_points_per_voxel;
    f.downsample_all = p->downsample_all_data ? 1u : 0u;
    if (!consume) {
        *peek = f;
        return CM_OK;
    }
    c->frame = f;
    c->n_in = n_in;
    c->n_sensors_used = k;
    for (auto& sl : c->slots) sl.fresh = false;       // flag reset, :151-157
    return CM_OK;
}

int fuse_points(cm_ctx* c, uint32_t* tile_counts, void* out, const unsigned char* mask, uint32_t* total) {
    frame_on_device(c);
    cmk_merged(c->stream, c->d_frame, tile_counts, c->merged_total, out, c->frame.n_tiles, mask);
    HIP_TRY(c, hipMemcpyAsync(total, c->merged_total, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CM_OK;
}

int measure_bounds(cm_ctx* c, uint32_t n_tiles, float mn[3], float mx[3], uint64_t* n_valid) {
    const uint32_t n_partials = n_tiles < CM_MINMAX_BLOCKS ? n_tiles : CM_MINMAX_BLOCKS;
    cmk_minmax(c->stream, c->d_frame, c->partials, n_partials, nullptr);
    std::vector<float> rec(static_cast<size_t>(n_partials) * 8);
    HIP_TRY(c, hipMemcpyAsync(rec.data(), c->partials, rec.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const float inf = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; ++a) { mn[a] = inf; mx[a] = -inf; }
    uint64_t cnt = 0;
    for (uint32_t r = 0; r < n_partials; ++r) {
        uint32_t k;
        std::memcpy(&k, &rec[r * 8 + 6], 4);
        if (!k) continue;
        cnt += k;
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], rec[r * 8 + a]);
            mx[a] = std::max(mx[a], rec[r * 8 + 3 + a]);
        }
    }
    *n_valid = cnt;
    return CM_OK;
}

int enqueue(cm_ctx* c, const cm_params* p, int mode, const float* bounds) {
    if (!c || !p) return CM_BAD_ARG;
    for (int a = 0; a < 3; ++a)
        if (!(p->leaf[a] > 0.0f) || !std::isfinite(p->leaf[a])) return fail(c, CM_BAD_ARG, "leaf must be > 0");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) return fail(c, CM_BAD_ARG, "previous frame not waited for (cm_wait)");

    // Everything that can reject the call is checked before the frame is assembled: assembling
    // consumes the sensors' "fresh" flags (:151-157), and a rejected call must not lose a frame.
    float inv_leaf[3], inv_cell[3] = {0.f, 0.f, 0.f};
    for (int a = 0; a < 3; ++a) inv_leaf[a] = 1.0f / p->leaf[a];
    const bool outl = p->outlier_enable != 0;
    if (outl && mode != 0) return fail(c, CM_BAD_ARG, "outlier removal needs the whole fused cloud on one GPU (not with partial tables)");
    if (c->ground_on && (outl || mode != 0)) return fail(c, CM_BAD_ARG, "ground removal is not combined with outlier_enable or partial tables");
    if (outl && (!(p->outlier_radius > 0.0f) || !std::isfinite(p->outlier_radius))) return fail(c, CM_BAD_ARG, "outlier_radius must be > 0");
    const bool outl_g = c->ground_on && c->ground_outlier_radius > 0.0f;      // the ground stage's own radius filter
    const bool any_outl = outl || outl_g;
    const float o_radius = outl ? p->outlier_radius : c->ground_outlier_radius;
    const uint32_t o_min_nb = outl ? p->outlier_min_neighbors : c->ground_outlier_min_nb;
    if (any_outl) for (int a = 0; a < 3; ++a) inv_cell[a] = 1.0f / (o_radius * 1.01f);   // candidate grid a little wider than r
    uint32_t key_bits = 0, kb_o = 0;
    int grid_mode = 0;                               // 0: data min/max (k_minmax), 1: crop box, 2: bounds handed in
    if (p->crop_enable && box_grid(p->crop_min, p->crop_max, inv_leaf, &key_bits)) grid_mode = 1;
    else if (mode == 1 && bounds && box_grid(bounds, bounds + 3, inv_leaf, &key_bits)) grid_mode = 2;
    else if (mode == 1) return fail(c, CM_BAD_ARG, "partial table needs the crop box or the fused cloud's bounds to fix the grid");
    int gm_o = 0;                                    // grid of the outlier stage: crop box or data min/max
    if (any_outl && p->crop_enable) {
        if (!box_grid(p->crop_min, p->crop_max, inv_cell, &kb_o))
            return fail(c, CM_CAPACITY, "outlier radius too small for the crop box (radius grid exceeds 32 bits)");
        gm_o = 1;
    }

    if (mode == 1 && c->motion_on) return fail(c, CM_BAD_ARG, "ego-motion compensation is not combined with partial tables (cm_set_ego_motion(NULL) first)");
    const bool sor = c->sor_on;
    if (sor && mode != 0)
        return fail(c, CM_BAD_ARG, "statistical outlier removal needs the whole fused cloud on one GPU (not with partial tables)");
    if (sor && outl) return fail(c, CM_BAD_ARG, "statistical outlier removal is not combined with outlier_enable");
    if (sor && c->ground_on) return fail(c, CM_BAD_ARG, "statistical outlier removal is not combined with ground removal");
    // (its search grid: over the crop box when there is one and a cell fits it — gm_o 1 — else over the cloud's bounds,
    // measured below: so for a crop box whose extent overflows fp32)
    float sor_cell_m = sor ? sor_cell(c->sor.search_cell, c->sor_last_mean) : 0.0f;
    if (sor) gm_o = sor_crop_grid(*p, &sor_cell_m, &kb_o);

    std::vector<std::unique_lock<std::mutex>> locks;
    c->prof_used = 0;                                // (k_motion, when compensation is on, is the frame's first stage)
    const int bf = build_frame(c, p, nullptr, locks);
    if (bf != CM_OK) return bf;
    CmFrameDev& f = c->frame;
    if (mode == 1 && bounds) {
        for (int a = 0; a < 3; ++a) { f.ext_min[a] = bounds[a]; f.ext_max[a] = bounds[3 + a]; }
    }
    if (sor && f.n_padded) {
        if (!gm_o) {
            // the grid over the cloud's own bounds (k_minmax, as the device will see them): a host round trip, then a cell
            // whose grid fits with room to spare. A cloud whose extent overflows fp32 fits none: one cell (inv_cell 0,
            // compute_grid's one cell per axis), every point a candidate of every other.
            if (descriptor_changed(c)) cmk_setup(c->stream, f, c->d_frame, c->d_tiles);
            float mn[3], mx[3];
            uint64_t cnt = 0;
            const int e = measure_bounds(c, f.n_tiles, mn, mx, &cnt);
            if (e != CM_OK) return e;
            if (cnt) sor_cell_m = sor_bounds_cell(sor_cell_m, mn, mx, &kb_o);
        }
        for (int a = 0; a < 3; ++a) inv_cell[a] = 1.0f / sor_cell_m;
        for (int a = 0; a < 3; ++a) f.inv_cell[a] = inv_cell[a];
    }
    c->last_sor = sor;                               // (after the last step that can fail: a failed enqueue leaves the last frame's)
    if (any_outl) {
        for (int a = 0; a < 3; ++a) f.inv_cell[a] = inv_cell[a];
        f.outlier_r2 = static_cast<float>(static_cast<double>(o_radius) * static_cast<double>(o_radius));
        f.outlier_min_nb = o_min_nb;
    }
    c->have_result = false;
    invalidate_result_tables(c);
    ++c->frame_serial;
    c->last_mode = mode;
    c->bytes_d2h = 0;
    if (c->pub_pending[0]) {
        // A copy-out (cm_result_publish_async) may still be reading the last frame's result: this frame writes the other
        // pair of buffers, and waits ON THE DEVICE for whatever copy-out read those (two frames ago: long done).
        std::swap(c->out, c->out_other);
        std::swap(c->out32, c->out32_other);
        std::swap(c->ev_pub[0], c->ev_pub[1]);
        std::swap(c->pub_pending[0], c->pub_pending[1]);
        if (c->pub_pending[0]) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_pub[0], 0));
            c->pub_pending[0] = false;
        }
    }

    if (f.n_padded == 0) {                             // every submitted cloud is empty
        c->frame_had_ground = c->ground_on && mode == 0;   // ... so are the ground cloud and every slab (no stale planes)
        c->trivial_grid = false;
        if (mode == 1) {
            // An empty share of a fused cloud still belongs to the shared grid: cm_merge_tables on this context
            // reports and decodes cells with it.
            const float* lo = grid_mode == 1 ? p->crop_min : bounds;
            const float* hi = grid_mode == 1 ? p->crop_max : bounds + 3;
            uint32_t kb = 0;
            if (box_grid(lo, hi, inv_leaf, &kb, c->cell_min_b, c->cell_div_b)) {
                c->trivial_grid = true;
                for (int a = 0; a < 3; ++a) { c->trivial_box[a] = lo[a]; c->trivial_box[3 + a] = hi[a]; }
            }
        }
        c->pending = true;
        c->pending_trivial = true;
        return CM_OK;
    }

    FramePlan& pl = c->plan;
    pl = FramePlan();
    pl.params = *p;
    pl.mode = mode;
    pl.grid_mode = grid_mode;
    pl.key_bits = key_bits;
    pl.outl = outl;
    pl.sor = sor;
    pl.sor_p = c->sor;
    pl.pre = outl || c->ground_on || sor;
    pl.gm_o = gm_o;
    pl.kb_o = kb_o;
    RouteState& rt = c->route;
    const bool spl_ok = rt.spl_valid;        // (valid again once this frame has finished and left its own splitters)
    rt.spl_valid = false;
    c->h_state->err = 0;                     // the bucket kernels write error words straight into the host record
    if (rt.needs_box(pl)) {                  // (first frame of a context without a crop box, or after a point left the box)
        const int e = bootstrap_box(c);
        if (e < 0) return e;
    }
    rt.plan(pl, f, bounds, inv_cell, spl_ok, c->n_in, c->cap_padded);
    if (pl.bucket && !pl.post_bucket) return launch_bucket(c, nullptr, nullptr);
    return launch_classic(c);
}

int wait_frame(cm_ctx* c, cm_result* res) {
    if (!c) return CM_BAD_ARG;
    if (!c->pending) return fail(c, CM_BAD_ARG, "no frame enqueued");
    HIP_TRY(c, hipSetDevice(c->device));
    cm_result r;
    std::memset(&r, 0, sizeof r);
    r.n_sensors = c->n_sensors_used;
    r.n_in = c->n_in;
    if (c->pending_trivial) {
        r.status = CM_EMPTY_INPUT;
        if (c->last_sor) {
            c->sor_stats = cm_sor_stats{0, 0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN(),
                                        std::numeric_limits<double>::infinity()};
        }
        if (c->last_mode == 1 && c->trivial_grid) {
            r.bounds_from_crop = 1;
            for (int a = 0; a < 3; ++a) {
                r.min_b[a] = c->cell_min_b[a]; r.div_b[a] = c->cell_div_b[a]; r.max_b[a] = r.min_b[a] + r.div_b[a] - 1;
                r.min_p[a] = c->trivial_box[a]; r.max_p[a] = c->trivial_box[3 + a];
            }
        }
    } else {
        HIP_TRY(c, hipEventSynchronize(c->ev_done));
        FramePlan& pl = c->plan;
        RouteState& rt = c->route;
        // (h is the pinned host record: after a replay, the replayed frame's)
        for (Replay how; (how = rt.settle(pl, *c->h_state)) != Replay::none;) {
            if (how == Replay::fixed_grid && rt.verbose)
                std::fprintf(stderr, "[cloudmerge] quantile frame handed back: err %u, n_valid %u, spl_n %u\n", c->h_state->err,
                             c->h_state->n_valid, rt.spl_n);
            pl.redone = true;
            const int e = replay(c, how);
            if (e != CM_OK) { c->pending = false; return e; }
            HIP_TRY(c, hipEventSynchronize(c->ev_done));
        }
        if (c->last_sor) {
            static_assert(sizeof(CmSorStatsDev) == sizeof(cm_sor_stats), "cm_sor_stats layout");
            HIP_TRY(c, hipMemcpy(&c->sor_stats, c->sor_words + CM_SOR_WORD_STATS, sizeof c->sor_stats, hipMemcpyDeviceToHost));
            if (rt.verbose) {                               // (CM_VERBOSE: how many points the second search launch took)
                uint32_t listed = 0;
                HIP_TRY(c, hipMemcpy(&listed, c->sor_words + CM_SOR_WORD_LIST, 4, hipMemcpyDeviceToHost));
                std::fprintf(stderr, "[cloudmerge] sor: n_valid %llu, second search launch %u points\n",
                             static_cast<unsigned long long>(c->sor_stats.n_valid), listed);
            }
            if (c->sor_stats.mean > 0.0 && std::isfinite(c->sor_stats.mean)) c->sor_last_mean = c->sor_stats.mean;
        }
        const CmFrameState& h = *c->h_state;
        if (h.err) {
            c->pending = false;
            if (h.err == CM_DEV_ERR_UNSORTED && rt.lds_rank) {
                // The sorted keys were not sorted: stop trusting lane-ordered LDS adds on this device.
                rt.lds_rank = false;
                return fail(c, CM_INTERNAL, "radix sort check failed with LDS-add ranking; switched to ballot ranking, resubmit the frame");
            }
            return fail(c, CM_INTERNAL, "device reported an internal error");
        }
        if (h.status == CM_DEV_ABORTED) {                  // (a stage gave up and nobody redid the frame: cannot happen)
            c->pending = false;
            return fail(c, CM_INTERNAL, "a device stage aborted the frame");
        }
        if (h.status == CM_DEV_OUTLIER_GRID) {
            c->pending = false;
            return fail(c, CM_CAPACITY, "outlier radius too small for the cloud's extent (radius grid exceeds its limits)");
        }
        r.status = h.status;
        r.bounds_from_crop = c->from_crop ? 1u : 0u;
        for (int a = 0; a < 3; ++a) {
            r.min_b[a] = h.min_b[a]; r.max_b[a] = h.max_b[a]; r.div_b[a] = h.div_b[a];
            r.min_p[a] = h.min_p[a]; r.max_p[a] = h.max_p[a];
            c->cell_min_b[a] = h.min_b[a]; c->cell_div_b[a] = h.div_b[a];
        }
        r.key_bits = h.key_bits;
        r.sort_passes = h.n_passes;
        r.path_flags = (rt.lds_rank ? CM_PATH_LDS_RANK : 0u) | (pl.redone ? CM_PATH_REDONE : 0u) | (c->last_motion ? CM_PATH_MOTION : 0u) |
                       (c->last_sor ? CM_PATH_SOR : 0u);
        if (pl.bucket)
            r.path_flags |= CM_PATH_BUCKET | (pl.predicted ? CM_PATH_PREDICTED : 0u) | (pl.pack ? CM_PATH_PACKED : 0u) |
                            (pl.k3 ? CM_PATH_SPLIT : 0u) | (pl.quant ? CM_PATH_QUANTILE : 0u);
        if (pl.predicted && h.status == CM_OK) exact_grid(h, c->frame.inv_leaf, r);
        rt.adopt(pl, h, c->frame, c->frame_mask != nullptr);
        if (h.status == CM_OK) {
            r.n_merged = h.n_valid;
            r.n_out = h.n_out;
        } else if (h.status == CM_GRID_OVERFLOW) {
            // PCL: "output = *input_" — hand back the merged cloud, unvoxelised (A.4 step 3).
            uint32_t total = 0;
            const int e = fuse_points(c, c->seg_counts, c->out, c->frame_mask, &total);
            if (e != CM_OK) return e;
            r.n_merged = total;
            r.n_out = total;
        }
        if (c->flags & CM_FLAG_PROFILE) {
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
            if (c->prof_used >= 2) (void)hipEventElapsedTime(&r.device_ms, c->prof_ev[0], c->prof_ev[c->prof_used - 1]);
        }
    }
    c->pending = false;
    c->result = r;
    c->have_result = true;
    if (res) *res = r;
    return r.status;
}

// The tables take the place of the sensor clouds: table t owns a tile-aligned range of the padded index space, so the point
// index a key carries maps back to (table, entry).
int merge_tables(cm_ctx* c, const void* const* dev_tables, const uint64_t* n_entries, uint32_t n_tables, const cm_params* p,
                 cm_result* res) {
    CmFrameDev& f = c->frame;
    std::memset(&f, 0, sizeof f);
    uint32_t base = 0;
    uint64_t total = 0;
    for (uint32_t t = 0; t < n_tables; ++t) {
        if (n_entries[t] && (!dev_tables[t] || (reinterpret_cast<uintptr_t>(dev_tables[t]) & 15u)))
            return fail(c, CM_BAD_ARG, "table pointers must be 16-byte aligned device memory");
        CmSensorDev& d = f.s[t];
        d.data = static_cast<const unsigned char*>(dev_tables[t]);
        d.n = static_cast<uint32_t>(n_entries[t]);
        d.base = base;
        d.slot = t;
        d.point_step = 32;
        const uint64_t nb = static_cast<uint64_t>(base) + round_up(d.n, CM_TILE);
        if (nb > c->cap_padded) return fail(c, CM_CAPACITY, "tables exceed cm_limits.max_points_total");
        base = static_cast<uint32_t>(nb);
        total += n_entries[t];
    }
    f.n_sensors = n_tables;
    f.n_padded = base;
    f.n_tiles = base / CM_TILE;
    f.min_pts = p->min_points_per_voxel;
    f.downsample_all = 1;
    cm_result r;
    std::memset(&r, 0, sizeof r);
    if (c->have_result && c->last_mode == 1) {       // keep the shared grid of this rank's partial table
        for (int a = 0; a < 3; ++a) {
            r.min_b[a] = c->result.min_b[a]; r.max_b[a] = c->result.max_b[a]; r.div_b[a] = c->result.div_b[a];
            r.min_p[a] = c->result.min_p[a]; r.max_p[a] = c->result.max_p[a];
        }
        r.bounds_from_crop = c->result.bounds_from_crop;
    }
    r.n_sensors = n_tables;
    r.n_in = total;
    c->have_result = false;
    invalidate_result_tables(c);
    ++c->frame_serial;
    c->last_mode = 2;
    c->prof_used = 0;
    if (f.n_padded == 0) {
        r.status = CM_EMPTY_INPUT;
        c->result = r; c->have_result = true;
        if (res) *res = r;
        return r.status;
    }
    hipStream_t st = c->stream;
    cmk_setup(st, f, c->d_frame, c->d_tiles);
    c->frame_uploaded = f;
    c->frame_uploaded_valid = true;
    CmFrameState* state = c->d_state[c->cur];
    CmFrameState* state_next = c->d_state[c->cur ^ 1];
    const uint32_t nt = f.n_tiles, nseg = f.n_padded / CM_SEG_TILE;
    const GrpArrays g = next_grp(c);
    if (!c->table_entries.once(static_cast<size_t>(c->cap_padded) * 32)) return fail(c, CM_HIP_ERROR, "cannot allocate the merged table");
    cmk_table_keys(st, c->d_frame, state, c->keys_a, c->hist, g.p0, g.p0_next, g.rest, g.gw, g.stride, c->seg_groups,
                   (nseg + CM_SEG_GROUP - 1) / CM_SEG_GROUP + 1, 32u, nt);
    radix_sort_pairs(c, state, {c->keys_a, c->keys_b, c->vals_a, c->vals_b, c->hist, c->totals, g.p0, g.rest}, CM_MAX_PASSES, nt,
                     f.n_padded, c->route.lds_rank, nullptr, nullptr);
    uint32_t* seg_groups = nseg > CM_SEG_DIRECT_TILES ? c->seg_groups : nullptr;
    cmk_seg_count(st, state, c->keys_a, c->keys_b, c->seg_tile_counts, seg_groups, 1u, nseg);
    cmk_seg_reduce(st, 2, c->d_frame, state, state_next, c->h_state_dev, c->keys_a, c->vals_a, c->keys_b, c->vals_b,
                   c->seg_tile_counts, seg_groups, c->table_entries, nullptr, nullptr, nseg);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    c->cur ^= 1;
    const CmFrameState& h = *c->h_state;
    if (h.err) {
        if (h.err == CM_DEV_ERR_UNSORTED && c->route.lds_rank) c->route.lds_rank = false;
        return fail(c, CM_INTERNAL, "device reported an internal error while merging tables");
    }
    const uint32_t n_merged = h.status == CM_OK ? h.n_out : 0;       // distinct voxels over all tables
    uint32_t n_out = 0;
    if (n_merged) {
        cmk_table_finish(st, c->table_entries, n_merged, p->min_points_per_voxel, c->seg_counts, c->merged_total,
                         c->out, c->out_key, c->out_cnt);
        HIP_TRY(c, hipMemcpyAsync(&n_out, c->merged_total, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    r.status = n_merged ? CM_OK : CM_EMPTY_INPUT;
    r.n_merged = n_merged;
    r.n_out = n_out;
    r.key_bits = 32; r.sort_passes = CM_MAX_PASSES;
    r.path_flags = c->route.lds_rank ? CM_PATH_LDS_RANK : 0u;
    c->result = r;
    c->have_result = true;
    if (res) *res = r;
    return r.status;
}
