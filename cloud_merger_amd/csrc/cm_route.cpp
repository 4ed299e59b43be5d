// cm_route.cpp — the route policy (cm_route.hpp). No launches and no HIP: what runs is cm_launch.cpp's business.
#include "cm_route.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

bool box_grid(const float bmin[3], const float bmax[3], const float inv[3], uint32_t* key_bits, int32_t* min_b, int32_t* div_b) {
    long long d[3];
    unsigned long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        const float ext = (bmax[a] - bmin[a]) * inv[a];
        if (!(ext < 2147483648.0f) || ext < 0.0f) return false;
        d[a] = static_cast<long long>(ext) + 1;
        const int lo = static_cast<int>(std::floor(bmin[a] * inv[a]));
        const int hi = static_cast<int>(std::floor(bmax[a] * inv[a]));
        if (hi < lo) return false;
        cells *= static_cast<unsigned long long>(hi - lo + 1);
        if (min_b) { min_b[a] = lo; div_b[a] = hi - lo + 1; }
    }
    if (d[0] * d[1] * d[2] > 2147483647LL || cells > 0xFFFFFFFFull) return false;
    *key_bits = key_width(cells);
    return true;
}

uint32_t key_width(unsigned long long cells) {
    uint32_t bits = 1;
    while (bits < 32 && (cells - 1) >> bits) ++bits;
    return bits;
}

uint32_t bucket_passes(uint32_t kb, uint64_t est, uint32_t extra) {
    // Dense frames — on average a point or more per cell of the box (the reference's own 10 cm grid on its ROI, or any
    // coarse leaf): sort the whole index globally. The finish then has nothing left to sort, a "bucket" is one voxel, and
    // a voxel of any size is summed by the long-run jobs of k3_local: no bucket can be too large, nothing is handed back.
    if (kb <= 8 * CM_MAX_PASSES && (est >> kb) >= 1) return (kb + 7) / 8;
    uint32_t g = 1 + (kb > CM2_MAX_LOW_BITS + 8 ? (kb - CM2_MAX_LOW_BITS - 1) / 8 : 0);
    while (g < CM_MAX_PASSES && (est >> (8 * g)) > 256) ++g;
    g += extra;
    if (g > 1 && 8 * (g - 1) >= kb) return 0;         // nothing left for the local finish to add
    return g <= CM_MAX_PASSES ? g : 0;
}

float sor_cell(float requested, double last_mean) {
    if (requested > 0.0f) return requested;
    if (!(last_mean > 0.0) || !std::isfinite(last_mean)) return 0.5f;
    return static_cast<float>(std::min(5.0, std::max(0.05, last_mean)));
}

float sor_fit_cell(float cell, const float bmin[3], const float bmax[3], uint32_t row_cap, uint32_t* key_bits) {
    for (;; cell *= 2.0f) {
        const float inv = 1.0f / cell;
        const float iv[3] = {inv, inv, inv};
        int32_t mb[3], db[3];
        // (a box whose extent overflows fp32 fits no finite cell: the caller takes another grid, key_bits stays as it was)
        if (!std::isfinite(cell)) return 0.0f;
        if (!box_grid(bmin, bmax, iv, key_bits, mb, db)) continue;
        if (static_cast<uint64_t>(db[1]) * static_cast<uint64_t>(db[2]) > row_cap) continue;
        if (db[0] >= (1 << 24) || db[1] >= (1 << 24) || db[2] >= (1 << 24)) continue;
        return cell;
    }
}

int sor_crop_grid(const cm_params& p, float* cell, uint32_t* key_bits) {
    if (!p.crop_enable) return 0;
    const float fit = sor_fit_cell(*cell, p.crop_min, p.crop_max, CM_ROW_TABLE_CAP / 2, key_bits);
    if (!(fit > 0.0f)) return 0;
    *cell = fit;
    return 1;
}

float sor_bounds_cell(float cell, const float mn[3], const float mx[3], uint32_t* key_bits) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = mn[a] - cell; hi[a] = mx[a] + cell; }
    const float fit = sor_fit_cell(cell, lo, hi, CM_ROW_TABLE_CAP / 4, key_bits);
    return fit > 0.0f ? fit : std::numeric_limits<float>::infinity();
}

namespace {

// The grid over [mn, mx] whose cell is `start` doubled until it fits (cm_route.hpp, cluster_grid).
ClusterGrid fit_centroid_grid(float start, const float mn[3], const float mx[3], uint32_t row_cap) {
    ClusterGrid g;
    g.doublings = 0;
    float ext[3];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        ext[a] = mx[a] - mn[a];
        finite = finite && std::isfinite(ext[a]);
    }
    for (float cell = start; finite && std::isfinite(cell); cell *= 2.0f, ++g.doublings) {
        const float inv = 1.0f / cell;
        unsigned long long d[3];
        bool fits = true;
        for (int a = 0; a < 3 && fits; ++a) {
            const float v = ext[a] * inv;
            fits = v >= 0.0f && v < static_cast<float>(CM_CLUSTER_AXIS_CAP);
            if (fits) d[a] = static_cast<unsigned long long>(std::floor(v)) + 1ull;
        }
        if (!fits || d[1] * d[2] > row_cap || d[0] * d[1] * d[2] > 0xFFFFFFFFull) continue;
        g.cell = cell;
        g.inv = inv;
        for (int a = 0; a < 3; ++a) g.dims[a] = static_cast<uint32_t>(d[a]);
        g.key_bits = key_width(d[0] * d[1] * d[2]);
        return g;
    }
    g.cell = std::numeric_limits<float>::infinity();
    g.inv = 0.0f;
    g.dims[0] = g.dims[1] = g.dims[2] = 1u;
    g.key_bits = 1;
    return g;
}

}  // namespace

ClusterGrid cluster_grid(float tolerance, const float mn[3], const float mx[3], uint32_t row_cap) {
    return fit_centroid_grid(tolerance * 1.00390625f, mn, mx, row_cap);
}

ClusterGrid normals_grid(float search_cell, const float leaf[3], uint32_t k, const float mn[3], const float mx[3], uint32_t row_cap) {
    float cell = search_cell;
    if (!(cell > 0.0f)) {
        float l = std::max(leaf[0], std::max(leaf[1], leaf[2]));
        if (!(l > 0.0f) || !std::isfinite(l)) l = 1.0f;
        cell = l * std::cbrt(static_cast<float>(k));
    }
    return fit_centroid_grid(cell, mn, mx, row_cap);
}

// A cloud near the limit of PCL's 32-bit index leaves no room for an eighth of its extent on every side: take what
// fits (a frame right behind one that reached far out would otherwise lose its box, and with it the bucket path).
void RouteState::set_predicted_box(const float mn[3], const float mx[3], const float leaf[3]) {
    float inv[3];
    for (int a = 0; a < 3; ++a) inv[a] = 1.0f / leaf[a];
    for (float part = 8.0f; part <= 1024.0f; part *= 2.0f) {
        for (int a = 0; a < 3; ++a) {
            const float ext = mx[a] - mn[a];
            const float margin = std::max(ext / part, (part <= 8.0f ? 8.0f : 2.0f) * leaf[a]);
            pred.min[a] = mn[a] - margin;
            pred.max[a] = mx[a] + margin;
        }
        uint32_t kb = 0;
        if (box_grid(pred.min, pred.max, inv, &kb)) break;
    }
    pred.ok = true;
}

// Keeps the predicted box while the cloud stays comfortably inside it and the box is not wastefully
// large (so the frame descriptor, and with it the key width, stays put from frame to frame).
void RouteState::update_predicted_box(const float mn[3], const float mx[3], const float leaf[3]) {
    bool redo = !pred.ok;
    for (int a = 0; a < 3 && !redo; ++a) {
        const float margin = std::max((mx[a] - mn[a]) / 8.0f, 8.0f * leaf[a]);
        const float lo = mn[a] - pred.min[a], hi = pred.max[a] - mx[a];
        redo = !(lo >= margin / 4.0f && lo <= 3.0f * margin && hi >= margin / 4.0f && hi <= 3.0f * margin);
    }
    if (!redo) {
        // ... and not a box so much larger than the cloud needs that it costs a global pass: after a frame that reached
        // far out the box would otherwise stay wide — and the index one digit longer — for as long as the cloud fits it
        float inv[3], tmin[3], tmax[3];
        for (int a = 0; a < 3; ++a) {
            inv[a] = 1.0f / leaf[a];
            const float margin = std::max((mx[a] - mn[a]) / 8.0f, 8.0f * leaf[a]);
            tmin[a] = mn[a] - margin; tmax[a] = mx[a] + margin;
        }
        uint32_t kb_now = 0, kb_tight = 0;
        if (box_grid(pred.min, pred.max, inv, &kb_now) && box_grid(tmin, tmax, inv, &kb_tight))
            redo = bucket_passes(kb_tight, 0, 0) < bucket_passes(kb_now, 0, 0);
    }
    if (redo) set_predicted_box(mn, mx, leaf);
}

// Bucket path: centroids of one GPU's whole frame, with a box known before the first point is read — the crop box, or the
// last frame's bounds plus a margin (verified on the device). Frames with pre-stages (ground / outlier removal, which leave
// a keep-mask) can use it too when the crop box fixes the grid: the pre-stages run first, then the bucket path takes the
// voxel stage. (Without lane-ordered LDS adds the bucket kernels rank by ballots: same results, more instructions.)
bool RouteState::bucket_applies(const FramePlan& pl) const {
    return !classic_only && (pl.mode == 0 || pl.mode == 1) && (!pl.pre || pl.grid_mode == 1);
}

bool RouteState::needs_box(const FramePlan& pl) const {
    return bucket_applies(pl) && !v2_off_frames && pl.grid_mode == 0 && !pred.ok;
}

// A crop box that dropped more than half of the last frame's points: k2_hist0 then also packs the survivors' records
// (into the record buffer the first scatter does not write), and the first scatter reads those instead of going
// through every raw point a second time — the raw clouds are read once, not twice.
bool RouteState::pack_survivors(const CmFrameDev& f, uint64_t n_in) const {
    return f.crop_enable && last_n_merged && 2 * last_n_merged < n_in;
}

void RouteState::plan(FramePlan& pl, CmFrameDev& f, const float* bounds, const float inv_cell[3], bool spl_ok, uint64_t n_in,
                      uint32_t cap_padded) {
    const cm_params& p = pl.params;
    if (!bucket_applies(pl)) return;
    if (v2_off_frames) { --v2_off_frames; return; }
    int gm = pl.grid_mode;
    uint32_t kb = pl.key_bits;
    if (gm == 0) {
        if (pred.ok && box_grid(pred.min, pred.max, f.inv_leaf, &kb, f.box_min_b, f.box_div_b)) {
            gm = 2;
            for (int a = 0; a < 3; ++a) { f.ext_min[a] = pred.min[a]; f.ext_max[a] = pred.max[a]; }
        } else {
            pred.ok = false;
        }
    }
    if (gm == 1 && !box_grid(p.crop_min, p.crop_max, f.inv_leaf, &kb, f.box_min_b, f.box_div_b)) gm = 0;
    if (gm == 2 && pl.mode == 1 && !box_grid(bounds, bounds + 3, f.inv_leaf, &kb, f.box_min_b, f.box_div_b)) gm = 0;
    // (the bucket kernels form the linear index on the 24-bit multiplier: fewer than 2^24 cells per axis)
    for (int a = 0; a < 3 && gm != 0; ++a)
        if (f.box_div_b[a] >= (1 << 24)) gm = 0;
    if (gm == 0) return;
    f.box_key_bits = kb;
    f.box_predicted = (gm == 2 && pl.mode == 0) ? 1u : 0u;
    // (points: what the last frame kept after crop and masks, plus a quarter, when there was one; a frame
    // that overflows anyway is handed back and v2_extra_passes adds a pass for the frames after it)
    const uint64_t est = last_n_merged ? std::min<uint64_t>(n_in, last_n_merged + last_n_merged / 4) : n_in;
    const uint32_t g = bucket_passes(kb, est, v2_extra_passes);
    if (!g) return;
    pl.bucket = true;
    pl.b_grid_mode = gm;
    pl.g = g;
    pl.low = kb > 8 * g ? kb - 8 * g : 0;
    // Quantile passes (one global pass instead of g): the last frame of this context left the quantiles of its
    // sorted records, as indices of this very grid, and this frame is about as large.
    bool quant = pl.mode == 0 && !pl.pre && !quant_never && !finish_v2 && spl_ok && g >= 2 && kb < 32 &&
                 f.n_tiles <= CM4_MAX_TILES && !(gm == 1 && pack_survivors(f, n_in)) &&
                 std::memcmp(spl_min_b, f.box_min_b, sizeof spl_min_b) == 0 &&
                 std::memcmp(spl_div_b, f.box_div_b, sizeof spl_div_b) == 0 &&
                 std::memcmp(spl_inv_leaf, f.inv_leaf, sizeof spl_inv_leaf) == 0;
    const uint32_t nb = quant ? cm_quant_buckets(spl_n) : 0;
    quant = quant && nb != 0 && spl_n / nb <= CM4_MAX_AVG && est <= 2ull * spl_n + CM_TILE &&
            nb + nb / 64 + 2 <= cap_padded / 1024 + 2 &&      // (tile_info + group totals fit their array)
            // Above 2048 buckets: still one pass, 2 or 4 neighbouring buckets to a bin (cm_device.h cm_quant_sub_shift;
            // cfg3's dense variant, 13.7 M records: 0.38-0.41 against 0.46-0.50 ms per frame for three fixed-grid passes).
            (nb <= CM4_BINS || quant_sub);
    if (quant && quant_off_frames) { --quant_off_frames; quant = false; }
    if (quant) {
        // more buckets than the pass has bins: 2^sub neighbouring buckets share a bin, the pass leaves the low bits of every
        // record's bucket number as a byte beside it and the finish picks its records out of the bin (k3_local<SUB>)
        pl.quant = true;
        pl.predicted = gm == 2;
        pl.k3 = true;
        pl.nb = nb;
        pl.sub = cm_quant_sub_shift(nb);
        // tile_info (one word pair per bucket) and, behind it, the group totals of the kept voxels: zeroed by k4_hist. The
        // number of buckets comes from the LAST frame's size — a frame of a twentieth of its predecessor's points has fewer
        // slots / 1024 than buckets (found by scripts/fuzz_shared_bins.py: the totals were then left as the last frame had them)
        pl.n_tile_state = std::max<uint32_t>(f.n_padded / 1024 + 2, nb + nb / 64 + 2);
        // The large finish shape (buckets of up to CM4_CAP_BIG records, one workgroup per CU) costs a launch of its own — 6 us on a
        // frame alone even when it has nothing to do — so it is only armed for 16 frames behind a hand-back or a frame that used
        // it; unarmed, any bucket beyond the usual shape's capacity hands the frame back (and arms it).
        pl.big_armed = !pl.sub && quant_big_arm > 0;
        if (quant_big_arm) --quant_big_arm;
        return;
    }
    if (pl.pre) {
        pl.post_bucket = true;
        // the outlier stage's own sort can use the bucket kernels as well: the crop box fixes its grid too (its bucket sort
        // builds on k2_local's lane-ordered ranking)
        uint32_t kb_o = pl.kb_o;
        bool pre_bucket = lds_rank && pl.gm_o == 1 && box_grid(p.crop_min, p.crop_max, inv_cell, &kb_o, f.cell_min_b, f.cell_div_b) &&
                          static_cast<uint64_t>(f.cell_div_b[1]) * static_cast<uint64_t>(f.cell_div_b[2]) <= CM_ROW_TABLE_CAP &&
                          f.cell_div_b[0] < (1 << 24) && f.cell_div_b[1] < (1 << 24) && f.cell_div_b[2] < (1 << 24);
        f.cell_key_bits = kb_o; f._pad_cell = 0;
        if (pre_bucket && pre_bucket_off) { --pre_bucket_off; pre_bucket = false; }
        pl.g_o = pre_bucket ? bucket_passes(kb_o, n_in, 0) : 0;
        pl.pack_o = pack_survivors(f, n_in);
    }
    size_fixed_grid(pl, f, n_in);
}

void RouteState::size_fixed_grid(FramePlan& pl, const CmFrameDev& f, uint64_t n_in) {
    pl.quant = false;
    pl.predicted = pl.b_grid_mode == 2 && pl.mode == 0;   // mode 1: the bounds handed in are the fused cloud's own
    pl.pack = !pl.predicted && pack_survivors(f, n_in);
    // (fewer than a sixteenth of the points survived the last frame's crop: eight tiles per workgroup, and few enough that
    // a wave's share of a tile is one load — k2_scatter_sparse takes a chunk of more than 64 records through a loop)
    pl.sparse = pl.pack && !debug_misrank && 16ull * last_n_merged < n_in;
    // The passes behind the first, and the finish, work on the records pass 0 kept. When a crop box dropped most points of
    // the last frame their grids are sized for what that frame kept (+ 50 % + two tiles), not for the padded frame — most of
    // those workgroups would only find out that they have nothing to do. Verified on the device: k3_compact raises
    // CM_DEV_ERR_GRID when the records need more, the frame is redone and the next frames use whole grids again.
    pl.nt_later = f.n_tiles;
    if (pl.mode == 0 && !pl.predicted && f.crop_enable && last_n_merged && !grid_shrink_off && !finish_v2) {
        const uint64_t est = last_n_merged + last_n_merged / 2 + 2 * CM_TILE;
        pl.nt_later = static_cast<uint32_t>(std::min<uint64_t>(f.n_tiles, (est + CM_TILE - 1) / CM_TILE));
    }
    if (grid_shrink_off) --grid_shrink_off;
    pl.k3 = !finish_v2 || !lds_rank;                      // (k2_local ranks by returning LDS adds only)
}

Replay RouteState::settle(const FramePlan& pl, CmFrameState& h) {
    if (pl.measured) {                                    // the redo in a measured box: a second hand-back goes to the general path
        if (h.outside) pred.ok = false;
        return h.outside || h.err ? Replay::general : Replay::none;
    }
    if (pl.bucket && pl.quant && !h.outside &&
        (h.err == CM_DEV_ERR_QUANT || h.err == CM_DEV_ERR_UNSORTED || h.err == CM_DEV_ERR_BUCKET)) {
        // A frame of the quantile passes whose buckets did not come out as predicted (one too large for the finish, or —
        // never seen — an index outside its bucket's range): the splitters are stale. Redone at once with the fixed-grid
        // passes in the same box, which leave the splitters of THIS scene, so the next frame may try at once: an abrupt
        // change costs one hand-back. A hand-back costs about a quarter of a frame more than the fixed-grid passes alone and
        // a good attempt saves a sixth, so attempts pay while fewer than one in three fail: the quantile passes only rest —
        // 8, 16, ... 128 frames — once three of the last eight attempts were handed back (a scene whose dense surfaces keep
        // moving across voxel layers: the index is z-major, so a ground plane that tilts by half a voxel at range moves its
        // points to other buckets).
        quant_hist = ((quant_hist << 1) | 1u) & 0xFFu;
        quant_good = 0;
        quant_big_arm = 16;                               // (the next frames may have buckets of two to four times the usual size)
        if (__builtin_popcount(quant_hist) >= 3) {
            quant_off_frames = quant_rest;
            if (quant_rest < 128) quant_rest *= 2;
            quant_hist = 0;
        }
        return Replay::fixed_grid;
    }
    // The bucket path hands a frame back when a point lay outside the predicted box, when a bucket did not fit LDS, or
    // when a workgroup gave up waiting for its predecessors: it is redone (the sensors' clouds are still in place) and
    // the cause is dealt with.
    if (pl.bucket && (h.outside || h.err == CM_DEV_ERR_BUCKET || h.err == CM_DEV_ERR_BUCKET_PRE || h.err == CM_DEV_ERR_LOOKBACK ||
                      h.err == CM_DEV_ERR_UNSORTED || h.err == CM_DEV_ERR_GRID)) {
        if (h.err == CM_DEV_ERR_GRID) grid_shrink_off = 64;   // more records than the last frame promised: whole grids for a while
        if (h.outside) pred.ok = false;
        // The finish found records out of bucket order: a global pass mis-ranked. Stop trusting lane-ordered LDS adds
        // on this device: from here on every kernel of the context ranks by ballots (this frame is redone on the
        // general path; the next ones take the bucket path again, ballot-ranked).
        if (h.err == CM_DEV_ERR_UNSORTED) { lds_rank = false; h.err = 0; debug_misrank = 0; }   // (the test hook fires once)
        if (h.err == CM_DEV_ERR_BUCKET) {
            if (v2_extra_passes < CM_MAX_PASSES) ++v2_extra_passes;
            if (v2_good_frames < 8 && v2_retry_after < (1u << 20)) v2_retry_after *= 2;   // the retry failed at once
            v2_good_frames = 0;
        }
        if (h.err == CM_DEV_ERR_BUCKET_PRE) {             // a radius cell too full for a tile: more passes would not help
            pre_bucket_off = pre_bucket_backoff;
            if (pre_bucket_backoff < (1u << 20)) pre_bucket_backoff *= 2;
        }
        if (h.err == CM_DEV_ERR_LOOKBACK) v2_off_frames = 0xFFFFFFFFu;
        return Replay::measured_box;
    }
    // (counted on the general path too: extra passes can add up to "no bucket path at all", and that must not be for ever)
    if (!pl.redone && v2_extra_passes && ++v2_good_frames >= v2_retry_after) {
        --v2_extra_passes;                                // the scene may have thinned out: try with less global sorting
        v2_good_frames = 0;
    }
    return Replay::none;
}

// A frame of the bucket path whose predicted box a point left: k2_hist0 measured the cloud's exact bounds all the same
// (its per-tile records, folded by the first scatter's workgroup 0 before it left), so the frame is redone at once in a box
// around those — on the bucket path again, without the general path's min/max pass.
bool RouteState::measured_box(FramePlan& pl, CmFrameDev& f, const CmFrameState& h, uint64_t n_in) {
    if (!h.outside || h.err || !pl.predicted || pl.mode != 0 || pl.pre || classic_only || h.n_valid_k0 == 0 || f.n_padded == 0)
        return false;
    float leaf[3];
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(h.min_p[a]) || !std::isfinite(h.max_p[a]) || h.min_p[a] > h.max_p[a]) return false;
        leaf[a] = pl.params.leaf[a];
    }
    const Box pred0 = pred;
    set_predicted_box(h.min_p, h.max_p, leaf);
    uint32_t kb = 0;
    if (!box_grid(pred.min, pred.max, f.inv_leaf, &kb, f.box_min_b, f.box_div_b)) { pred = pred0; pred.ok = false; return false; }
    for (int a = 0; a < 3; ++a) {
        if (f.box_div_b[a] >= (1 << 24)) { pred = pred0; return false; }
        f.ext_min[a] = pred.min[a]; f.ext_max[a] = pred.max[a];
    }
    f.box_key_bits = kb;
    f.box_predicted = 1u;
    const uint32_t g = bucket_passes(kb, h.n_valid_k0, v2_extra_passes);
    if (!g) { pred = pred0; return false; }
    pl.measured = true;
    pl.b_grid_mode = 2;
    pl.g = g;
    pl.low = kb > 8 * g ? kb - 8 * g : 0;
    size_fixed_grid(pl, f, n_in);
    return true;
}

void RouteState::adopt(const FramePlan& pl, const CmFrameState& h, const CmFrameDev& f, bool masked) {
    if (h.status != CM_OK) return;
    if (pl.mode == 0 && !masked && (pl.predicted || (!pl.bucket && pl.grid_mode == 0))) {
        float leaf[3];
        for (int a = 0; a < 3; ++a) leaf[a] = 1.0f / f.inv_leaf[a];
        update_predicted_box(h.min_p, h.max_p, leaf);
    }
    last_n_merged = h.n_valid;
    if (pl.writes_splitters() && h.n_valid && !h.spl_incomplete) {
        // the finish left the quantiles of this frame's sorted records: the next frame's splitters (cm_kernels_v4.hip)
        spl_cur ^= 1;
        spl_valid = true;
        spl_n = h.n_valid;
        std::memcpy(spl_min_b, f.box_min_b, sizeof spl_min_b);
        std::memcpy(spl_div_b, f.box_div_b, sizeof spl_div_b);
        std::memcpy(spl_inv_leaf, f.inv_leaf, sizeof spl_inv_leaf);
        if (pl.quant && h.quant_big) quant_big_arm = 16;      // (still needed: stays armed)
        if (pl.quant && !pl.redone) {
            quant_hist = (quant_hist << 1) & 0xFFu;
            if (++quant_good >= 16) quant_rest = 8;
        }
    }
}
