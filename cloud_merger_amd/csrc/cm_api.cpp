// cm_api.cpp — the C-ABI declared in include/cloudmerge.h: entry points and their argument checks. Frames are
// assembled and launched in cm_launch.cpp, routed in cm_route.cpp; the tables computed from a result on request are
// cm_byproducts.cpp's; the context is cm_ctx.hpp, whose buffers own their memory (cm_devbuf.hpp): cm_destroy is `delete`.
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

#include "cm_cost_table.hpp"
#include "cm_ctx.hpp"
#include "cm_match_table.hpp"
#include "cm_cast_math.hpp"
#include "cm_mcl_beam_table.hpp"
#include "cm_mcl_math.hpp"

namespace {

const char* k_status_names(int s) {
    switch (s) {
        case CM_OK: return "CM_OK";
        case CM_EMPTY_INPUT: return "CM_EMPTY_INPUT";
        case CM_GRID_OVERFLOW: return "CM_GRID_OVERFLOW";
        case CM_NOT_READY: return "CM_NOT_READY";
        case CM_SKIPPED: return "CM_SKIPPED";
        case CM_BAD_ARG: return "CM_BAD_ARG";
        case CM_HIP_ERROR: return "CM_HIP_ERROR";
        case CM_NO_DEVICE: return "CM_NO_DEVICE";
        case CM_CAPACITY: return "CM_CAPACITY";
        case CM_INTERNAL: return "CM_INTERNAL";
        default: return "CM_UNKNOWN";
    }
}

// Eigen::Quaternionf(w,x,y,z).toRotationMatrix() in fp32, tf doubles rounded per component
// (reference call site pc_preprocessing_main.cpp:320-322).
void quat_to_rows(const double q[4], const double t[3], float m[12]) {
    const float x = static_cast<float>(q[0]), y = static_cast<float>(q[1]);
    const float z = static_cast<float>(q[2]), w = static_cast<float>(q[3]);
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0] = 1.0f - (tyy + tzz); m[1] = txy - twz;          m[2] = txz + twy;           m[3] = static_cast<float>(t[0]);
    m[4] = txy + twz;          m[5] = 1.0f - (txx + tzz); m[6] = tyz - twx;           m[7] = static_cast<float>(t[1]);
    m[8] = txz - twy;          m[9] = tyz + twx;          m[10] = 1.0f - (txx + tyy); m[11] = static_cast<float>(t[2]);
}

}  // namespace

cm_ctx::~cm_ctx() {
    for (auto& s : slots) {
        if (s.copy_stream) (void)hipStreamDestroy(s.copy_stream);
        if (s.ev_copy) (void)hipEventDestroy(s.ev_copy);
    }
    if (pub_stream) (void)hipStreamDestroy(pub_stream);
    for (auto e : ev_pub) if (e) (void)hipEventDestroy(e);
    for (auto e : prof_ev) (void)hipEventDestroy(e);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

namespace {

int set_slot_cloud(cm_ctx* c, uint32_t sensor, const void* data, bool on_device, uint32_t n,
                   uint32_t step, uint32_t ox, uint32_t oy, uint32_t oz, uint32_t oi, bool wait_copy = true) {
    if (!c) return CM_BAD_ARG;
    if (sensor >= c->max_sensors) return fail(c, CM_BAD_ARG, "sensor index out of range");
    if (n && !data) return fail(c, CM_BAD_ARG, "null payload");
    auto fits = [step](uint32_t off) { return static_cast<uint64_t>(off) + 4u <= step; };   // (no 32-bit wrap-around)
    if (n && (step < 12 || !fits(ox) || !fits(oy) || !fits(oz) || (oi != CM_NO_FIELD && !fits(oi))))
        return fail(c, CM_BAD_ARG, "field offsets do not fit point_step");
    if (n > c->max_points) return fail(c, CM_CAPACITY, "cloud larger than cm_limits.max_points_total");
    HIP_TRY(c, hipSetDevice(c->device));
    Slot& s = c->slots[sensor];
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.fresh && !(c->flags & CM_FLAG_LATEST_WINS)) return CM_SKIPPED;   // first since last fuse wins
    const size_t bytes = static_cast<size_t>(n) * step;
    SlotCloud sc;
    sc.n = n; sc.step = step; sc.ox = ox; sc.oy = oy; sc.oz = oz; sc.oi = oi;
    if (on_device) {
        sc.dptr = data;
        s.bytes_h2d = 0;
    } else {
        // the buffer no enqueued frame reads (a replaced staged cloud lived there too: same copy stream, in order)
        const int w = s.active_buf == 0 ? 1 : 0;
        if (bytes > s.buf[w].capacity() && !s.buf[w].reserve(bytes + bytes / 4 + 256))
            return fail(c, CM_HIP_ERROR, "cannot allocate the sensor's staging buffer");
        if (bytes) {
            HIP_TRY(c, hipMemcpyAsync(s.buf[w], data, bytes, hipMemcpyHostToDevice, s.copy_stream));
            if (wait_copy) {
                HIP_TRY(c, hipStreamSynchronize(s.copy_stream));     // the caller may release `data` when this returns
                s.copy_pending = false;
            } else {
                HIP_TRY(c, hipEventRecord(s.ev_copy, s.copy_stream));  // the frame that consumes the cloud waits for it
                s.copy_pending = true;
            }
        }
        sc.dptr = s.buf[w];
        s.bytes_h2d = bytes;
    }
    s.staged = sc;
    s.has_data = true;
    s.fresh = true;
    ++s.gen;
    return CM_OK;
}

// The refusals the tables computed from the last result's centroids share: CM_OK when there is such a result at rest.
// Caller holds merge_mu, as for every check below.
int centroid_result_check(cm_ctx* c) {
    if (c->pending) return fail(c, CM_BAD_ARG, "a frame is in flight (cm_wait first)");
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    if (c->last_mode != 0) return fail(c, CM_BAD_ARG, "the last result is a partial or merged table (cm_merge_partial / cm_merge_tables)");
    if (c->result.status != CM_OK) return fail(c, CM_BAD_ARG, std::string("last frame has no voxel grid (") + k_status_names(c->result.status) + ")");
    return CM_OK;
}

// The refusals of cm_result_voxel_cov*: CM_OK when a table can be computed with *q.
int voxel_cov_check(cm_ctx* c, const cm_cov_params* p, cm_cov_params* q) {
    if (!(c->flags & CM_FLAG_OCCUPANCY)) return fail(c, CM_BAD_ARG, "context created without CM_FLAG_OCCUPANCY");
    if (const int e = centroid_result_check(c)) return e;
    *q = p ? *p : cm_cov_params{6u, 0.01f};
    if (q->min_points < 3) return fail(c, CM_BAD_ARG, "min_points must be at least 3");
    if (!(q->eig_mult >= 0.0f && q->eig_mult <= 1.0f)) return fail(c, CM_BAD_ARG, "eig_mult must lie in [0, 1]");
    return CM_OK;
}

// The refusals of cm_result_clusters*: CM_OK when the last result can be clustered with *p.
int clusters_check(cm_ctx* c, const cm_cluster_params* p) {
    if (!p) return fail(c, CM_BAD_ARG, "no cluster parameters");
    if (const int e = centroid_result_check(c)) return e;
    if (!std::isfinite(p->tolerance) || !(p->tolerance > 0.0f)) return fail(c, CM_BAD_ARG, "tolerance must be finite and > 0");
    const float t2 = p->tolerance * p->tolerance;
    if (!std::isfinite(t2) || !(t2 > 0.0f)) return fail(c, CM_BAD_ARG, "the fp32 square of the tolerance must be finite and > 0");
    if (p->min_cluster_size == 0) return fail(c, CM_BAD_ARG, "min_cluster_size must be at least 1");
    if (p->min_cluster_size > p->max_cluster_size) return fail(c, CM_BAD_ARG, "min_cluster_size exceeds max_cluster_size");
    return CM_OK;
}

// The refusals of cm_result_cluster_boxes*: CM_OK when the last result's clusters can be fitted with *p.
int boxes_check(cm_ctx* c, const cm_box_params* p) {
    if (!p) return fail(c, CM_BAD_ARG, "no box parameters");
    if (const int e = clusters_check(c, &p->cluster)) return e;
    if (p->n_angles == 0 || p->n_angles > CM_BOX_MAX_ANGLES) return fail(c, CM_BAD_ARG, "n_angles must be in 1..CM_BOX_MAX_ANGLES");
    if (p->criterion != CM_BOX_AREA && p->criterion != CM_BOX_CLOSENESS) return fail(c, CM_BAD_ARG, "unknown box criterion");
    if (p->criterion == CM_BOX_CLOSENESS && (!std::isfinite(p->d_min) || !(p->d_min > 0.0f)))
        return fail(c, CM_BAD_ARG, "d_min must be finite and > 0");
    return CM_OK;
}

// The refusals of cm_result_grid_map*: CM_OK when the last frame's grid map can be computed with *p.
int grid_check(cm_ctx* c, const cm_grid_params* p) {
    if (!p) return fail(c, CM_BAD_ARG, "no grid parameters");
    if (const int e = centroid_result_check(c)) return e;
    if (!std::isfinite(p->origin[0]) || !std::isfinite(p->origin[1])) return fail(c, CM_BAD_ARG, "the origin must be finite");
    if (!std::isfinite(p->cell) || !(p->cell > 0.0f)) return fail(c, CM_BAD_ARG, "cell must be finite and > 0");
    const float inv = 1.0f / p->cell;
    if (!std::isfinite(inv) || !(inv > 0.0f)) return fail(c, CM_BAD_ARG, "the fp32 inverse of cell must be finite and > 0");
    if (p->nx == 0 || p->ny == 0) return fail(c, CM_BAD_ARG, "nx and ny must be at least 1");
    if (static_cast<uint64_t>(p->nx) * p->ny > CM_GRID_MAX_CELLS) return fail(c, CM_BAD_ARG, "nx * ny exceeds CM_GRID_MAX_CELLS");
    if (std::isnan(p->z_min) || std::isnan(p->z_max)) return fail(c, CM_BAD_ARG, "a band limit is NaN");
    if (p->z_min > p->z_max) return fail(c, CM_BAD_ARG, "z_min exceeds z_max");
    if (!std::isfinite(p->obstacle_height) || !(p->obstacle_height >= 0.0f)) return fail(c, CM_BAD_ARG, "obstacle_height must be finite and >= 0");
    if (p->min_points == 0) return fail(c, CM_BAD_ARG, "min_points must be at least 1");
    return CM_OK;
}

// The refusals of cm_result_normals*: CM_OK when the last result's normals can be computed with *p.
int normals_check(cm_ctx* c, const cm_normal_params* p) {
    if (!p) return fail(c, CM_BAD_ARG, "no normal parameters");
    if (const int e = centroid_result_check(c)) return e;
    if (p->k < 3 || p->k > CM_NORMAL_MAX_K) return fail(c, CM_BAD_ARG, "k must be in 3..CM_NORMAL_MAX_K");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(p->viewpoint[a])) return fail(c, CM_BAD_ARG, "the viewpoint must be finite");
    if (!std::isfinite(p->search_cell) || p->search_cell < 0.0f) return fail(c, CM_BAD_ARG, "search_cell must be finite and >= 0");
    return CM_OK;
}

// The refusals the two registrations share, behind those of their own parameters: the loop's limits, the guess, the source.
int registration_check(cm_ctx* c, uint32_t max_iterations, uint32_t iter_cap, const char* iter_text, uint32_t min_correspondences,
                       double trans_eps, double rot_eps, const double guess[12], const void* src, uint64_t n_src) {
    if (max_iterations > iter_cap) return fail(c, CM_BAD_ARG, iter_text);
    if (min_correspondences < 6) return fail(c, CM_BAD_ARG, "min_correspondences must be at least 6");
    if (!(trans_eps >= 0.0) || !(rot_eps >= 0.0)) return fail(c, CM_BAD_ARG, "trans_eps and rot_eps must be >= 0");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(guess[k])) return fail(c, CM_BAD_ARG, "the guess must be finite");
    if (n_src >= (1ull << 30)) return fail(c, CM_BAD_ARG, "the source must hold fewer than 2^30 records");
    if (n_src && !src) return fail(c, CM_BAD_ARG, "null source");
    return CM_OK;
}

// The refusals of cm_result_align*: CM_OK when n_src records at src can be aligned to the last result with *p.
int align_check(cm_ctx* c, const cm_align_params* p, const void* src, uint64_t n_src, const cm_align_result* out) {
    if (!p) return fail(c, CM_BAD_ARG, "no alignment parameters");
    if (!out) return fail(c, CM_BAD_ARG, "no place for the alignment's outcome");
    if (const int e = centroid_result_check(c)) return e;
    if (!std::isfinite(p->max_corr_dist) || !(p->max_corr_dist > 0.0f)) return fail(c, CM_BAD_ARG, "max_corr_dist must be finite and > 0");
    const float r2 = p->max_corr_dist * p->max_corr_dist;
    if (!std::isfinite(r2) || !(r2 > 0.0f)) return fail(c, CM_BAD_ARG, "the fp32 square of max_corr_dist must be finite and > 0");
    if (p->normals_k < 3 || p->normals_k > CM_NORMAL_MAX_K) return fail(c, CM_BAD_ARG, "normals_k must be in 3..CM_NORMAL_MAX_K");
    return registration_check(c, p->max_iterations, CM_ALIGN_MAX_ITER, "max_iterations must be in 0..CM_ALIGN_MAX_ITER",
                              p->min_correspondences, p->trans_eps, p->rot_eps, p->guess, src, n_src);
}

// The refusals of cm_result_ndt_align*: CM_OK when n_src records at src can be aligned to the last result's covariance table
// with *p; *cov: the table's parameters, the default for {0, 0}.
int ndt_check(cm_ctx* c, const cm_ndt_params* p, const void* src, uint64_t n_src, const cm_ndt_result* out, cm_cov_params* cov) {
    if (!p) return fail(c, CM_BAD_ARG, "no NDT parameters");
    if (!out) return fail(c, CM_BAD_ARG, "no place for the NDT registration's outcome");
    const bool dflt = p->cov.min_points == 0 && p->cov.eig_mult == 0.0f;
    if (const int e = voxel_cov_check(c, dflt ? nullptr : &p->cov, cov)) return e;
    if (!std::isfinite(p->outlier_ratio) || !(p->outlier_ratio > 0.0f && p->outlier_ratio < 1.0f))
        return fail(c, CM_BAD_ARG, "outlier_ratio must be finite and in (0, 1)");
    if (p->neighborhood != 1 && p->neighborhood != 7) return fail(c, CM_BAD_ARG, "neighborhood must be 1 or 7");
    return registration_check(c, p->max_iterations, CM_NDT_MAX_ITER, "max_iterations must be in 0..CM_NDT_MAX_ITER",
                              p->min_correspondences, p->trans_eps, p->rot_eps, p->guess, src, n_src);
}

// A registration's host source into fit.src, grown on demand: *src_dev is where the n_src records of 16 bytes then lie.
// what: the error text of a failure to grow.
int stage_source(cm_ctx* c, PoseFit& fit, const void* src_host, uint64_t n_src, const char* what, const void** src_dev) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!fit.src.reserve(n_src * 16)) return fail(c, CM_HIP_ERROR, what);
    if (n_src) {
        HIP_TRY(c, hipMemcpyAsync(fit.src, src_host, n_src * 16, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *src_dev = fit.src;
    return CM_OK;
}

// cm_*_correspondences_copy: the entries of `bytes` each that fit's last call left. what: the error text without such a call.
int copy_correspondences(cm_ctx* c, const PoseFit& fit, size_t bytes, const char* what, void* host_dst, uint64_t capacity, uint64_t* n) {
    if (!fit.have) return fail(c, CM_BAD_ARG, what);
    *n = fit.n_src;
    if (fit.n_src > capacity) return fail(c, CM_CAPACITY, "correspondence destination too small");
    if (fit.n_src == 0) return CM_OK;
    if (!host_dst) return fail(c, CM_BAD_ARG, "null destination");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host_dst, fit.corr, fit.n_src * bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += fit.n_src * bytes;
    return CM_OK;
}

// cm_merged_copy / cm_ground_copy: the frame's points that `mask` keeps, fused into `merged`, then to the host.
// counted: their bytes go into bytes_d2h (cm_frame_stats).
int copy_fused(cm_ctx* c, const unsigned char* mask, void* host_dst, uint64_t capacity, uint64_t* n_points, bool counted) {
    if (c->frame.n_padded == 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!ensure_merged(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the fused cloud's buffer");
    // (seg_counts holds this frame's output offsets in its first cap_seg_tiles words: the tail takes the tile counts)
    uint32_t total = 0;
    const int e = fuse_points(c, c->seg_counts + c->cap_seg_tiles, c->merged, mask, &total);
    if (e != CM_OK) return e;
    *n_points = total;
    if (total > capacity) return fail(c, CM_CAPACITY, "destination too small");
    if (total && host_dst) {
        HIP_TRY(c, hipMemcpyAsync(host_dst, c->merged, static_cast<size_t>(total) * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (counted) c->bytes_d2h += static_cast<uint64_t>(total) * 16;
    }
    return CM_OK;
}

// A frame enqueued and waited for in one call: a refused frame still leaves its status in *res.
int merge_and_wait(cm_ctx* c, const cm_params* p, int mode, const float* bounds, cm_result* res) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    const int e = enqueue(c, p, mode, bounds);
    if (e != CM_OK) {
        if (res) { std::memset(res, 0, sizeof *res); res->status = e; }
        return e;
    }
    return wait_frame(c, res);
}

}  // namespace

extern "C" {

int cm_version(void) { return CM_VERSION; }
const char* cm_status_string(int status) { return k_status_names(status); }
const char* cm_last_error(cm_ctx* ctx) {
    if (!ctx) return "null context";
    static thread_local std::string copy;              // valid until the calling thread asks again
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    copy = ctx->err;
    return copy.c_str();
}

int cm_create(cm_ctx** out, int device, const cm_limits* lim) {
    if (!out || !lim) return CM_BAD_ARG;
    *out = nullptr;
    if (lim->max_sensors < 1 || lim->max_sensors > CM_MAX_SENSORS) return CM_BAD_ARG;
    if (lim->max_points_total < 1 || lim->max_points_total >= (1ull << 30)) return CM_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CM_NO_DEVICE;
    if (device < 0 || device >= ndev) return CM_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return CM_HIP_ERROR;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CM_HIP_ERROR;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CM_NO_DEVICE;   // kernels are gfx950-only

    cm_ctx* c = new (std::nothrow) cm_ctx();
    if (!c) return CM_INTERNAL;
    c->device = device;
    c->flags = lim->flags;
    c->max_sensors = lim->max_sensors;
    c->max_points = lim->max_points_total;
    const uint64_t padded = static_cast<uint64_t>(round_up(static_cast<uint32_t>(lim->max_points_total), CM_TILE)) +
                            static_cast<uint64_t>(lim->max_sensors) * CM_TILE;
    c->cap_padded = static_cast<uint32_t>(padded);
    c->cap_tiles = c->cap_padded / CM_TILE;
    c->cap_seg_tiles = c->cap_padded / CM_SEG_TILE;

    const size_t npad = c->cap_padded, nt = c->cap_tiles, nseg = c->cap_seg_tiles;
    bool ok = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) == hipSuccess;
    c->stream = c->own_stream;
    ok = ok && hipEventCreate(&c->ev_done) == hipSuccess;
    ok = ok && c->keys_a.once(npad) && c->keys_b.once(npad) && c->vals_a.once(npad) && c->vals_b.once(npad);
    ok = ok && c->hist.once(nt * CM_RADIX);
    c->cap_groups = (c->cap_tiles + CM_GROUP - 1) / CM_GROUP;
    {
        const size_t gwords = static_cast<size_t>(c->cap_groups) * CM_RADIX * 5;
        ok = ok && c->grp.once(gwords) && hipMemset(c->grp, 0, gwords * 4) == hipSuccess;
    }
    ok = ok && c->seg_tile_counts.once(nseg + 1) && c->seg_groups.once((nseg / CM_SEG_GROUP + 2) * 32);
    ok = ok && c->partials.once(CM_MINMAX_BLOCKS * 8) && c->totals.once(CM_RADIX) && c->seg_counts.once(nseg + nt);
    ok = ok && c->merged_total.once(256 / 4) && c->out.once(npad * 16);
    if (c->flags & CM_FLAG_OCCUPANCY) ok = ok && c->out_key.once(npad) && c->out_cnt.once(npad);
    ok = ok && c->d_frame.once(1) && c->d_tiles.once(nt);
    ok = ok && c->h_tile_kept.once(nt);
    ok = ok && hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_tile_kept), c->h_tile_kept, 0) == hipSuccess;
    ok = ok && c->d_state[0].once(1) && c->d_state[1].once(1) && c->h_state.once(1);
    ok = ok && hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_state_dev), c->h_state, 0) == hipSuccess;
    for (uint32_t s = 0; ok && s < c->max_sensors; ++s)
        ok = hipStreamCreateWithFlags(&c->slots[s].copy_stream, hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&c->slots[s].ev_copy, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMemset(c->d_state[0], 0, sizeof(CmFrameState)) == hipSuccess;
    ok = ok && hipMemset(c->d_state[1], 0, sizeof(CmFrameState)) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    // The environment switches, read once here.
    RouteState& rt = c->route;
    if (const char* pm = getenv("CM_PATH")) rt.classic_only = std::strcmp(pm, "classic") == 0;
    if (ok) {
        // Probe the device once: lane-ordered returning LDS adds allow the cheap stable ranking.
        // CM_LDS_RANK=0 forces the ballot-match ranking, CM_LDS_RANK=1 skips the probe.
        const char* env = getenv("CM_LDS_RANK");
        if (env && env[0] == '0') rt.lds_rank = false;
        else if (env && env[0] == '1') rt.lds_rank = true;
        else {
            uint32_t violations = 1;
            ok = hipMemset(c->merged_total, 0, 4) == hipSuccess;
            if (ok) {
                cmk_probe_lds_order(c->stream, c->merged_total, 64);
                ok = hipMemcpyAsync(&violations, c->merged_total, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                     hipStreamSynchronize(c->stream) == hipSuccess;
            }
            rt.lds_rank = ok && violations == 0;
        }
    }
    if (const char* fm = getenv("CM_FINISH")) rt.finish_v2 = std::strcmp(fm, "v2") == 0;
#ifdef CM_TEST_HOOKS                     // (the test build only: python -m cloud_merger_amd.build --test-hooks; never the shipped library)
    if (const char* dm = getenv("CM_DEBUG_MISRANK")) rt.debug_misrank = dm[0] == '1' ? 1 : 0;
#endif
    if (const char* qm = getenv("CM_QUANT")) rt.quant_never = qm[0] == '0';     // CM_QUANT=0: fixed-grid passes only
    if (const char* qs = getenv("CM_QUANT_SUB")) rt.quant_sub = qs[0] != '0';
    rt.verbose = getenv("CM_VERBOSE") != nullptr;
    // CM_BOX_SPLIT=<members>: where the box fit hands a cluster to the chunk-wise launches (a measurement's switch; the
    // table is the same bytes at every value)
    if (const char* bs = getenv("CM_BOX_SPLIT")) {
        const unsigned long v = std::strtoul(bs, nullptr, 10);
        if (v >= 1 && v < 0xFFFFFFFFul) c->box_split = static_cast<uint32_t>(v);
    }
    // CM_MCL_BEAM_WALKS=<1|2|4>: how many rays a lane of k_mcl_beam keeps in flight (a measurement's switch; the tables are
    // the same bytes at every value)
    if (const char* bw = getenv("CM_MCL_BEAM_WALKS")) {
        const unsigned long v = std::strtoul(bw, nullptr, 10);
        if (v == 1 || v == 2 || v == 4) c->mcl_beam_walks = static_cast<uint32_t>(v);
    }
    // CM_MCL_HYP_NO_AGG=1: the lanes of a wave send their own atomics in k_mcl_hyp_sums and k_mcl_hyp_spread (a measurement's
    // switch; the hypotheses are the same bytes either way)
    if (const char* na = getenv("CM_MCL_HYP_NO_AGG"))
        if (na[0] == '1' && na[1] == 0) c->mcl_hyp_agg = 0;
    if (!ok) {
        delete c;
        return CM_HIP_ERROR;
    }
    std::memset(&c->result, 0, sizeof c->result);
    std::memset(&c->stage_times, 0, sizeof c->stage_times);
    *out = c;
    return CM_OK;
}

int cm_destroy(cm_ctx* c) {
    if (!c) return CM_BAD_ARG;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    delete c;
    return CM_OK;
}

int cm_set_stream(cm_ctx* c, void* hip_stream) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (c->pending) return fail(c, CM_BAD_ARG, "cannot change stream with a frame in flight");
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    return CM_OK;
}

int cm_set_sensor_transform(cm_ctx* c, uint32_t sensor, const double q[4], const double t[3]) {
    if (!q || !t) return CM_BAD_ARG;
    float m[12];
    quat_to_rows(q, t, m);
    return cm_set_sensor_matrix(c, sensor, m);
}

int cm_set_sensor_matrix(cm_ctx* c, uint32_t sensor, const float m[12]) {
    if (!c || !m) return CM_BAD_ARG;
    if (sensor >= c->max_sensors) return fail(c, CM_BAD_ARG, "sensor index out of range");
    std::lock_guard<std::mutex> lk(c->slots[sensor].mu);
    std::memcpy(c->slots[sensor].m, m, 12 * sizeof(float));
    return CM_OK;
}

int cm_get_sensor_matrix(cm_ctx* c, uint32_t sensor, float m[12]) {
    if (!c || !m) return CM_BAD_ARG;
    if (sensor >= c->max_sensors) return fail(c, CM_BAD_ARG, "sensor index out of range");
    std::lock_guard<std::mutex> lk(c->slots[sensor].mu);
    std::memcpy(m, c->slots[sensor].m, 12 * sizeof(float));
    return CM_OK;
}

int cm_submit_cloud(cm_ctx* c, uint32_t sensor, const void* host_data, uint32_t n, uint32_t point_step,
                    uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i) {
    return set_slot_cloud(c, sensor, host_data, false, n, point_step, off_x, off_y, off_z, off_i);
}

int cm_submit_cloud_async(cm_ctx* c, uint32_t sensor, const void* host_data, uint32_t n, uint32_t point_step,
                          uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i) {
    return set_slot_cloud(c, sensor, host_data, false, n, point_step, off_x, off_y, off_z, off_i, false);
}

int cm_submit_cloud_device(cm_ctx* c, uint32_t sensor, const void* dev_data, uint32_t n, uint32_t point_step,
                           uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_i) {
    return set_slot_cloud(c, sensor, dev_data, true, n, point_step, off_x, off_y, off_z, off_i);
}

int cm_clear_sensor(cm_ctx* c, uint32_t sensor) {
    if (!c) return CM_BAD_ARG;
    if (sensor >= c->max_sensors) return fail(c, CM_BAD_ARG, "sensor index out of range");
    std::lock_guard<std::mutex> lk(c->slots[sensor].mu);
    c->slots[sensor].has_data = false;
    c->slots[sensor].fresh = false;
    c->slots[sensor].staged = SlotCloud();       // (the buffers stay: a frame in flight may still read the active one)
    return CM_OK;
}

int cm_merge_voxelize_async(cm_ctx* c, const cm_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return enqueue(c, p);
}

int cm_wait(cm_ctx* c, cm_result* res) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return wait_frame(c, res);
}

int cm_merge_voxelize(cm_ctx* c, const cm_params* p, cm_result* res) { return merge_and_wait(c, p, 0, nullptr, res); }

int cm_result_device(cm_ctx* c, const void** dev_ptr, uint64_t* n_points) {
    if (!c || !dev_ptr || !n_points) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    *dev_ptr = c->out;
    *n_points = c->result.n_out;
    return CM_OK;
}

int cm_result_copy(cm_ctx* c, void* host_dst, uint64_t capacity_points, uint32_t step_out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    if (step_out == 0) step_out = 16;
    if (step_out != 16 && step_out != 32) return fail(c, CM_BAD_ARG, "point_step_out must be 16 or 32");
    const uint64_t n = c->result.n_out;
    if (n > capacity_points) return fail(c, CM_CAPACITY, "destination too small");
    if (n == 0) return CM_OK;
    if (!host_dst) return CM_BAD_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    c->bytes_d2h += n * 16;
    if (step_out == 16) {
        HIP_TRY(c, hipMemcpyAsync(host_dst, c->out, n * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return CM_OK;
    }
    // pcl::PointXYZI images (A.0) are laid out on the device and cross PCIe as they go on the wire
    if (!ensure_out32(c)) return fail(c, CM_HIP_ERROR, "cannot allocate the 32-byte result buffers");
    cmk_to_pcl32(c->stream, c->out, c->out32, static_cast<uint32_t>(n));
    HIP_TRY(c, hipMemcpyAsync(host_dst, c->out32, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += n * 16;
    return CM_OK;
}

int cm_result_copy_async(cm_ctx* c, void* host_dst, uint64_t capacity_points) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    const uint64_t n = c->result.n_out;
    if (n > capacity_points) return fail(c, CM_CAPACITY, "destination too small");
    if (n == 0) return CM_OK;
    if (!host_dst) return CM_BAD_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host_dst, c->out, n * 16, hipMemcpyDeviceToHost, c->stream));
    c->bytes_d2h += n * 16;
    return CM_OK;
}

int cm_result_publish_async(cm_ctx* c, void* host_dst, uint64_t capacity_points, uint32_t step_out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    if (c->pending) return fail(c, CM_BAD_ARG, "a frame is in flight: publish its predecessor before enqueueing it");
    if (step_out == 0) step_out = 16;
    if (step_out != 16 && step_out != 32) return fail(c, CM_BAD_ARG, "point_step_out must be 16 or 32");
    const uint64_t n = c->result.n_out;
    if (n > capacity_points) return fail(c, CM_CAPACITY, "destination too small");
    if (n == 0) return CM_OK;
    if (!host_dst) return CM_BAD_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->pub_stream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->pub_stream, hipStreamNonBlocking));
        for (auto& e : c->ev_pub) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (!c->out_other.once(static_cast<size_t>(c->cap_padded) * 16)) return fail(c, CM_HIP_ERROR, "cannot allocate the second result buffer");
    }
    // (the frame has been waited for — cm_wait returned its counts — so its result is complete; an overflow fallback's
    // merged cloud was written on c->stream and synchronised as well)
    if (step_out == 16) {
        HIP_TRY(c, hipMemcpyAsync(host_dst, c->out, n * 16, hipMemcpyDeviceToHost, c->pub_stream));
    } else {
        if (!ensure_out32(c) || !c->out32_other.once(static_cast<size_t>(c->cap_padded) * 32))
            return fail(c, CM_HIP_ERROR, "cannot allocate the 32-byte result buffers");
        cmk_to_pcl32(c->pub_stream, c->out, c->out32, static_cast<uint32_t>(n));
        HIP_TRY(c, hipMemcpyAsync(host_dst, c->out32, n * 32, hipMemcpyDeviceToHost, c->pub_stream));
    }
    HIP_TRY(c, hipEventRecord(c->ev_pub[0], c->pub_stream));
    c->pub_pending[0] = true;
    c->bytes_d2h += n * step_out;
    return CM_OK;
}

int cm_publish_wait(cm_ctx* c) {
    if (!c) return CM_BAD_ARG;
    if (!c->pub_stream) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->pub_stream));
    // (pub_pending stays as it is: it steers which buffers the next frame writes, and a finished event costs nothing to wait for)
    return CM_OK;
}

int cm_sync(cm_ctx* c) {
    if (!c) return CM_BAD_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->pub_stream) HIP_TRY(c, hipStreamSynchronize(c->pub_stream));
    return CM_OK;
}

int cm_get_frame_stats(cm_ctx* c, cm_frame_stats* out) {
    if (!c || !out) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    std::memset(out, 0, sizeof *out);
    out->n_sensors = c->stats_n_sensors;
    const uint32_t* kept = c->h_tile_kept;                 // (written by the frame's first scatter; the frame has been waited for)
    const bool have_kept = c->result.status == CM_OK && c->frame.n_tiles && c->last_mode != 2;
    for (uint32_t k = 0; k < c->stats_n_sensors; ++k) {
        out->sensor[k] = c->stats_sensor[k];
        out->n_in[k] = c->stats_n[k];
        out->fresh[k] = c->stats_fresh[k];
        out->bytes_h2d[k] = c->stats_bytes[k];
        out->generation[k] = c->stats_gen[k];
        out->bytes_h2d_total += c->stats_bytes[k];
        if (have_kept) {
            const uint32_t t0 = c->frame.s[k].base / CM_TILE, t1 = t0 + (c->frame.s[k].n + CM_TILE - 1) / CM_TILE;
            uint64_t sum = 0;
            for (uint32_t t = t0; t < t1 && t < c->frame.n_tiles; ++t) sum += kept[t];
            out->n_kept[k] = static_cast<uint32_t>(sum);
        }
    }
    out->bytes_d2h_total = c->bytes_d2h;
    out->bytes_algorithmic = 16ull * c->result.n_in + 16ull * c->result.n_out;
    return CM_OK;
}

int cm_result_copy_cells(cm_ctx* c, int32_t* ijk, uint32_t* counts, uint64_t capacity) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    if (!(c->flags & CM_FLAG_OCCUPANCY)) return fail(c, CM_BAD_ARG, "context created without CM_FLAG_OCCUPANCY");
    if (c->result.status != CM_OK) return fail(c, CM_BAD_ARG, "last frame has no voxel grid");
    const uint64_t n = c->result.n_out;
    if (n > capacity) return fail(c, CM_CAPACITY, "destination too small");
    if (n == 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (counts) HIP_TRY(c, hipMemcpyAsync(counts, c->out_cnt, n * 4, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint32_t> keys;
    if (ijk) {
        keys.resize(n);
        HIP_TRY(c, hipMemcpyAsync(keys.data(), c->out_key, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ijk) {
        // out_key holds linear indices in the grid the frame was sorted in (the crop box, the predicted
        // box or the cloud's own bounds); the caller gets absolute cells floor(p / leaf).
        const uint32_t d0 = static_cast<uint32_t>(c->cell_div_b[0]), d1 = static_cast<uint32_t>(c->cell_div_b[1]);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t k = keys[i];
            ijk[3 * i + 0] = static_cast<int32_t>(k % d0) + c->cell_min_b[0];
            ijk[3 * i + 1] = static_cast<int32_t>((k / d0) % d1) + c->cell_min_b[1];
            ijk[3 * i + 2] = static_cast<int32_t>(k / (d0 * d1)) + c->cell_min_b[2];
        }
    }
    return CM_OK;
}

int cm_merged_copy(cm_ctx* c, void* host_dst, uint64_t capacity, uint64_t* n_points) {
    if (!c || !n_points) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    *n_points = 0;
    return copy_fused(c, c->frame_mask, host_dst, capacity, n_points, true);
}

// How a call hands n elements of `elem` bytes at src (HBM) to the caller: the capacity refusal with the call's own text, the
// missing destination (after an empty result's CM_OK where the call answers an empty result without one), the copy, the wait.
static int copy_out(cm_ctx* c, void* host_dst, const void* src, uint64_t n, size_t elem, uint64_t capacity, const char* too_small,
                    bool empty_is_ok = false) {
    if (n > capacity) return fail(c, CM_CAPACITY, too_small);
    if (empty_is_ok && n == 0) return CM_OK;
    if (!host_dst) return fail(c, CM_BAD_ARG, "no destination");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host_dst, src, n * elem, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += n * elem;
    return CM_OK;
}

// The same for a table the context keeps on the host (the cost table, the field table).
static int table_out(cm_ctx* c, uint8_t* host_dst, const std::vector<unsigned char>& table, uint64_t capacity, uint64_t* n, const char* too_small) {
    if (n) *n = table.size();
    if (table.size() > capacity) return fail(c, CM_CAPACITY, too_small);
    if (!host_dst) return fail(c, CM_BAD_ARG, "no destination");
    std::memcpy(host_dst, table.data(), table.size());
    return CM_OK;
}

static_assert(sizeof(cm_voxel_cov) == 80 && sizeof(CmVoxelCovDev) == sizeof(cm_voxel_cov), "cm_voxel_cov is 80 bytes");
static_assert(CM_COV_VALID == CM_COV_VALID_DEV && CM_COV_INFLATED == CM_COV_INFLATED_DEV, "flags mirror the header");

int cm_result_voxel_cov(cm_ctx* c, const cm_cov_params* p, cm_voxel_cov* host_dst, uint64_t capacity) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_cov_params q;
    int e = voxel_cov_check(c, p, &q);
    if (e != CM_OK) return e;
    if (c->result.n_out > capacity) return fail(c, CM_CAPACITY, "destination too small");
    if (c->result.n_out && !host_dst) return fail(c, CM_BAD_ARG, "no destination");
    e = voxel_cov(c, q);
    if (e != CM_OK) return e;
    return copy_out(c, host_dst, c->cov_entries, c->result.n_out, sizeof(cm_voxel_cov), capacity, "destination too small", true);
}

int cm_result_voxel_cov_device(cm_ctx* c, const cm_cov_params* p, const void** dev_ptr, uint64_t* n) {
    if (!c || !dev_ptr || !n) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_cov_params q;
    int e = voxel_cov_check(c, p, &q);
    if (e == CM_OK) e = voxel_cov(c, q);
    if (e != CM_OK) return e;
    *dev_ptr = c->cov_entries;
    *n = c->result.n_out;
    return CM_OK;
}

static_assert(sizeof(cm_cluster) == 40 && sizeof(CmClusterDev) == sizeof(cm_cluster), "cm_cluster is 40 bytes");
static_assert(sizeof(cm_cluster_params) == 16, "cm_cluster_params is 16 bytes");
static_assert(CM_CLUSTER_NONE == CM_INVALID_KEY, "the radix sort drops the unclustered voxels as invalid keys");

int cm_result_clusters(cm_ctx* c, const cm_cluster_params* p, uint32_t* labels_host, uint64_t labels_capacity,
                       cm_cluster* clusters_host, uint64_t clusters_capacity, uint32_t* indices_host, uint64_t indices_capacity,
                       uint64_t* n_clusters, uint64_t* n_clustered) {
    if (!c || !n_clusters || !n_clustered) return CM_BAD_ARG;
    *n_clusters = 0;
    *n_clustered = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = clusters_check(c, p);
    if (e != CM_OK) return e;
    if ((!labels_host && labels_capacity) || (!clusters_host && clusters_capacity) || (!indices_host && indices_capacity))
        return fail(c, CM_BAD_ARG, "a destination with a capacity but no pointer");
    e = clusters(c, *p);
    if (e != CM_OK) return e;
    *n_clusters = c->cl_n_clusters;
    *n_clustered = c->cl_n_clustered;
    if (labels_host && c->result.n_out > labels_capacity) return fail(c, CM_CAPACITY, "labels destination too small");
    if (clusters_host && c->cl_n_clusters > clusters_capacity) return fail(c, CM_CAPACITY, "clusters destination too small");
    if (indices_host && c->cl_n_clustered > indices_capacity) return fail(c, CM_CAPACITY, "indices destination too small");
    const uint64_t n = c->result.n_out;
    uint64_t bytes = 0;
    if (labels_host && n) {
        HIP_TRY(c, hipMemcpyAsync(labels_host, c->cl_labels, n * 4, hipMemcpyDeviceToHost, c->stream));
        bytes += n * 4;
    }
    if (clusters_host && c->cl_n_clusters) {
        HIP_TRY(c, hipMemcpyAsync(clusters_host, c->cl_clusters, c->cl_n_clusters * sizeof(cm_cluster), hipMemcpyDeviceToHost, c->stream));
        bytes += c->cl_n_clusters * sizeof(cm_cluster);
    }
    if (indices_host && c->cl_n_clustered) {
        HIP_TRY(c, hipMemcpyAsync(indices_host, c->cl_indices, c->cl_n_clustered * 4, hipMemcpyDeviceToHost, c->stream));
        bytes += c->cl_n_clustered * 4;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += bytes;
    return CM_OK;
}

int cm_result_clusters_device(cm_ctx* c, const cm_cluster_params* p, const void** labels, const void** clusters_dev,
                              const void** indices, uint64_t* n_clusters, uint64_t* n_clustered) {
    if (!c || !labels || !clusters_dev || !indices || !n_clusters || !n_clustered) return CM_BAD_ARG;
    *n_clusters = 0;
    *n_clustered = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = clusters_check(c, p);
    if (e == CM_OK) e = clusters(c, *p);
    if (e != CM_OK) return e;
    *labels = c->result.n_out ? c->cl_labels : nullptr;
    *clusters_dev = c->cl_n_clusters ? c->cl_clusters : nullptr;
    *indices = c->cl_n_clustered ? c->cl_indices : nullptr;
    *n_clusters = c->cl_n_clusters;
    *n_clustered = c->cl_n_clustered;
    return CM_OK;
}

static_assert(sizeof(cm_cluster_box) == 48 && sizeof(CmBoxDev) == sizeof(cm_cluster_box) && sizeof(cm_box_params) == 32,
              "cm_cluster_box is 48 bytes, its parameters 32");
static_assert(offsetof(cm_cluster_box, score) == offsetof(CmBoxDev, score) && offsetof(cm_cluster_box, flags) == offsetof(CmBoxDev, flags),
              "the kernels' entry");
static_assert(CM_BOX_CHUNK == CM_BOX_CHUNK_DEV && CM_BOX_MAX_ANGLES == CM_BOX_MAX_ANGLES_DEV && CM_BOX_MAX_EXTENT == CM_BOX_MAX_EXTENT_DEV &&
                  CM_BOX_CLOSENESS == CM_BOX_CLOSENESS_DEV && CM_BOX_VALID == CM_BOX_VALID_DEV,
              "the kernels' constants");

int cm_box_directions(uint32_t n_angles, float* cos_sin, uint64_t capacity_pairs) {
    if (!cos_sin || n_angles == 0 || n_angles > CM_BOX_MAX_ANGLES) return CM_BAD_ARG;
    if (capacity_pairs < n_angles) return CM_CAPACITY;
    box_direction_table(n_angles, cos_sin);
    return CM_OK;
}

int cm_result_cluster_boxes(cm_ctx* c, const cm_box_params* p, cm_cluster_box* host_dst, uint64_t capacity, uint64_t* n_boxes) {
    if (!c || !n_boxes) return CM_BAD_ARG;
    *n_boxes = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = boxes_check(c, p);
    if (e != CM_OK) return e;
    if (!host_dst && capacity) return fail(c, CM_BAD_ARG, "a destination with a capacity but no pointer");
    e = cluster_boxes(c, *p);
    if (e != CM_OK) return e;
    const uint64_t n = c->box_n;
    *n_boxes = n;
    if (n > capacity) return fail(c, CM_CAPACITY, "boxes destination too small");
    if (n == 0) return CM_OK;
    HIP_TRY(c, hipMemcpyAsync(host_dst, c->box_entries, n * sizeof(cm_cluster_box), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += n * sizeof(cm_cluster_box);
    return CM_OK;
}

int cm_result_cluster_boxes_device(cm_ctx* c, const cm_box_params* p, const void** dev_ptr, uint64_t* n_boxes) {
    if (!c || !dev_ptr || !n_boxes) return CM_BAD_ARG;
    *dev_ptr = nullptr;
    *n_boxes = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = boxes_check(c, p);
    if (e == CM_OK) e = cluster_boxes(c, *p);
    if (e != CM_OK) return e;
    *dev_ptr = c->box_n ? c->box_entries : nullptr;
    *n_boxes = c->box_n;
    return CM_OK;
}

static_assert(sizeof(cm_grid_cell) == 32 && sizeof(cm_grid_cell) == CM_GRID_WORDS * 4 && sizeof(cm_grid_params) == 36 &&
                  sizeof(CmGridDev) == sizeof(cm_grid_params),
              "cm_grid_cell is 32 bytes, its parameters 36");
static_assert(offsetof(cm_grid_cell, z_lo) == 8 && offsetof(cm_grid_cell, g_lo) == 16 && offsetof(cm_grid_cell, i_max) == 24 &&
                  offsetof(cm_grid_cell, state) == 28,
              "the kernels' record");
static_assert(CM_GRID_UNKNOWN == CM_GRID_UNKNOWN_DEV && CM_GRID_FREE == CM_GRID_FREE_DEV && CM_GRID_OCCUPIED == CM_GRID_OCCUPIED_DEV,
              "the kernels' states");

int cm_result_grid_map(cm_ctx* c, const cm_grid_params* p, cm_grid_cell* host_dst, uint64_t capacity_cells) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = grid_check(c, p);
    if (e != CM_OK) return e;
    e = grid_map(c, *p);
    if (e != CM_OK) return e;
    const uint64_t n = c->grid_n;
    return copy_out(c, host_dst, c->grid_cells, n, sizeof(cm_grid_cell), capacity_cells, "grid destination too small");
}

int cm_result_grid_map_device(cm_ctx* c, const cm_grid_params* p, const void** dev_ptr, uint64_t* n_cells) {
    if (!c || !dev_ptr || !n_cells) return CM_BAD_ARG;
    *dev_ptr = nullptr;
    *n_cells = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = grid_check(c, p);
    if (e == CM_OK) e = grid_map(c, *p);
    if (e != CM_OK) return e;
    *dev_ptr = c->grid_cells;
    *n_cells = c->grid_n;
    return CM_OK;
}

int cm_grid_occupancy_copy(cm_ctx* c, int8_t* host_dst, uint64_t capacity_cells, uint64_t* n_cells) {
    if (!c || !n_cells) return CM_BAD_ARG;
    *n_cells = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (c->pending) return fail(c, CM_BAD_ARG, "a frame is in flight (cm_wait first)");
    if (!c->grid_have) return fail(c, CM_BAD_ARG, "no grid map of the last result (cm_result_grid_map first)");
    const uint64_t n = c->grid_n;
    *n_cells = n;
    return copy_out(c, host_dst, c->grid_image, n, 1, capacity_cells, "occupancy destination too small");
}

static_assert(sizeof(cm_grid_ray_cell) == 8 && offsetof(cm_grid_ray_cell, n_end) == 4 && sizeof(cm_ray_params) == 8,
              "cm_grid_ray_cell is 8 bytes (the kernels' two words), its parameters 8");

// The refusals of cm_result_grid_rays*: grid_check's, and a min_pass of 0. *r: the parameters in force (NULL: {1, 0}).
static int rays_check(cm_ctx* c, const cm_grid_params* p, const cm_ray_params* in, cm_ray_params* r) {
    if (const int e = grid_check(c, p)) return e;
    *r = in ? *in : cm_ray_params{1u, 0u};
    if (r->min_pass == 0) return fail(c, CM_BAD_ARG, "min_pass must be at least 1");
    return CM_OK;
}

int cm_result_grid_rays(cm_ctx* c, const cm_grid_params* p, const cm_ray_params* r, cm_grid_ray_cell* host_dst, uint64_t capacity_cells) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_ray_params rr;
    int e = rays_check(c, p, r, &rr);
    if (e != CM_OK) return e;
    e = grid_rays(c, *p, rr);
    if (e != CM_OK) return e;
    const uint64_t n = c->ray_n;
    return copy_out(c, host_dst, c->ray_cells, n, sizeof(cm_grid_ray_cell), capacity_cells, "ray destination too small");
}

int cm_result_grid_rays_device(cm_ctx* c, const cm_grid_params* p, const cm_ray_params* r, const void** dev_ptr, uint64_t* n_cells) {
    if (!c || !dev_ptr || !n_cells) return CM_BAD_ARG;
    *dev_ptr = nullptr;
    *n_cells = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_ray_params rr;
    int e = rays_check(c, p, r, &rr);
    if (e == CM_OK) e = grid_rays(c, *p, rr);
    if (e != CM_OK) return e;
    *dev_ptr = c->ray_cells;
    *n_cells = c->ray_n;
    return CM_OK;
}

int cm_grid_ray_occupancy_copy(cm_ctx* c, int8_t* host_dst, uint64_t capacity_cells, uint64_t* n_cells) {
    if (!c || !n_cells) return CM_BAD_ARG;
    *n_cells = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (c->pending) return fail(c, CM_BAD_ARG, "a frame is in flight (cm_wait first)");
    if (!c->ray_have) return fail(c, CM_BAD_ARG, "no rays of the last result (cm_result_grid_rays first)");
    const uint64_t n = c->ray_n;
    *n_cells = n;
    return copy_out(c, host_dst, c->ray_image, n, 1, capacity_cells, "cleared occupancy destination too small");
}

static_assert(sizeof(cm_map_params) == 48 && offsetof(cm_map_params, max_range_cells) == 44 && sizeof(cm_map_cell) == 8 &&
                  offsetof(cm_map_cell, n_obs) == 4 && sizeof(cm_map_info) == 32 && offsetof(cm_map_info, n_frames) == 16,
              "cm_map_params is 48 bytes, cm_map_cell 8 (the kernels' two words), cm_map_info 32");

// What every call on a layer of the map refuses first (cm_map_layers.hpp): a frame in flight, a missing ancestor, the missing
// layer, and for a read a stale result. layer_fresh_check is the last part alone.
static int layer_check(cm_ctx* c, int layer, bool read) {
    const std::string why = layer_refusal(c->layers, c->pending, c->frame_serial, layer, read, c->map.info.n_frames != 0);
    return why.empty() ? CM_OK : fail(c, CM_BAD_ARG, why);
}
static int layer_fresh_check(cm_ctx* c, int layer) {
    const std::string why = layer_stale(c->layers, c->frame_serial, layer, c->map.info.n_frames != 0);
    return why.empty() ? CM_OK : fail(c, CM_BAD_ARG, why);
}
// What a layer's configure call refuses first: a frame in flight and, where p is there, a missing ancestor.
static int configure_check(cm_ctx* c, int layer, const void* p) {
    const std::string why = layer_configure_refusal(c->layers, c->pending, layer, p == nullptr);
    return why.empty() ? CM_OK : fail(c, CM_BAD_ARG, why);
}
// What the producers behind the cost layer refuse about its tables, in their own wording.
static int cost_fresh_check(cm_ctx* c) { return c->layers[LAYER_COST].fresh() ? CM_OK : fail(c, CM_BAD_ARG, cost_stale_text()); }

// What cm_map_integrate and the two matchers refuse about a pose; v: the vehicle's cell.
static int pose_check(cm_ctx* c, const float pose[12], int v[2]) {
    if (!pose) return fail(c, CM_BAD_ARG, "no pose");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(pose[k])) return fail(c, CM_BAD_ARG, "the pose must be finite");
    if (!map_vehicle_cell(c, pose, v)) return fail(c, CM_BAD_ARG, "the vehicle's cell does not exist (beyond 2^30 cells from the world origin)");
    return CM_OK;
}

// The refusals of cm_map_configure about *p.
static int map_params_check(cm_ctx* c, const cm_map_params* p) {
    if (!std::isfinite(p->cell) || !(p->cell > 0.0f)) return fail(c, CM_BAD_ARG, "cell must be finite and > 0");
    const float inv = 1.0f / p->cell;
    if (!std::isfinite(inv) || !(inv > 0.0f)) return fail(c, CM_BAD_ARG, "the fp32 inverse of cell must be finite and > 0");
    if (p->nx == 0 || p->ny == 0) return fail(c, CM_BAD_ARG, "nx and ny must be at least 1");
    if (static_cast<uint64_t>(p->nx) * p->ny > CM_GRID_MAX_CELLS) return fail(c, CM_BAD_ARG, "nx * ny exceeds CM_GRID_MAX_CELLS");
    if (std::isnan(p->z_min) || std::isnan(p->z_max)) return fail(c, CM_BAD_ARG, "a band limit is NaN");
    if (p->z_min > p->z_max) return fail(c, CM_BAD_ARG, "z_min exceeds z_max");
    if (p->l_hit < 1 || p->l_miss < 1) return fail(c, CM_BAD_ARG, "l_hit and l_miss must be at least 1");
    for (const int32_t l : {p->l_hit, p->l_miss, p->l_min, p->l_max, p->l_free, p->l_occ})
        if (l > CM_MAP_MAX_LOGODDS || l < -CM_MAP_MAX_LOGODDS) return fail(c, CM_BAD_ARG, "a log-odds parameter exceeds 2^20 in magnitude");
    if (!(p->l_min <= p->l_free && p->l_free < p->l_occ && p->l_occ <= p->l_max))
        return fail(c, CM_BAD_ARG, "the thresholds must satisfy l_min <= l_free < l_occ <= l_max");
    if (!(p->l_min <= 0 && 0 <= p->l_max)) return fail(c, CM_BAD_ARG, "the clamp limits must satisfy l_min <= 0 <= l_max");
    return CM_OK;
}

int cm_map_configure(cm_ctx* c, const cm_map_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_MAP, p)) return e;
    if (p)
        if (const int e = map_params_check(c, p)) return e;
    return map_configure(c, p);
}

int cm_map_integrate(cm_ctx* c, const float pose[12], cm_map_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = centroid_result_check(c)) return e;
    if (!c->layers[LAYER_MAP].on) return fail(c, CM_BAD_ARG, LAYER_TABLE[LAYER_MAP].absent);
    int v[2];
    if (const int e = pose_check(c, pose, v)) return e;
    if (c->map.serial == c->frame_serial) return fail(c, CM_BAD_ARG, "the last frame was already integrated");
    if (const int e = map_integrate(c, pose, v)) return e;
    if (out) *out = c->map.info;
    return CM_OK;
}

int cm_map_copy(cm_ctx* c, cm_map_cell* host_dst, uint64_t capacity_cells, cm_map_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MAP, true)) return e;
    if (info) *info = c->map.info;
    const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    return copy_out(c, host_dst, c->map.state[c->map.cur], n, sizeof(cm_map_cell), capacity_cells, "map destination too small");
}

int cm_map_device(cm_ctx* c, const void** dev_ptr, cm_map_info* info) {
    if (!c || !dev_ptr) return CM_BAD_ARG;
    *dev_ptr = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MAP, true)) return e;
    if (info) *info = c->map.info;
    *dev_ptr = c->map.state[c->map.cur];
    return CM_OK;
}

int cm_map_occupancy_copy(cm_ctx* c, int8_t* host_dst, uint64_t capacity_cells, cm_map_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MAP, true)) return e;
    if (info) *info = c->map.info;
    const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    return copy_out(c, host_dst, c->map.image, n, 1, capacity_cells, "map image destination too small");
}

int cm_map_load(cm_ctx* c, const cm_map_cell* host_src, uint64_t n_cells, const int32_t anchor[2], cm_map_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MAP, true)) return e;
    if (!host_src) return fail(c, CM_BAD_ARG, "no state table");
    if (!anchor) return fail(c, CM_BAD_ARG, "no anchor");
    if (n_cells != static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny) return fail(c, CM_BAD_ARG, "n_cells is not nx * ny");
    for (int k = 0; k < 2; ++k)
        if (anchor[k] <= -(1 << 30) || anchor[k] >= (1 << 30)) return fail(c, CM_BAD_ARG, "the anchor lies 2^30 cells or more from the world origin");
    for (uint64_t i = 0; i < n_cells; ++i)
        if (host_src[i].logodds < c->map.params.l_min || host_src[i].logodds > c->map.params.l_max)
            return fail(c, CM_BAD_ARG, "a logodds lies outside [l_min, l_max]");
    if (const int e = map_load(c, host_src, anchor)) return e;
    if (out) *out = c->map.info;
    return CM_OK;
}

static_assert(sizeof(cm_cost_params) == 16 && offsetof(cm_cost_params, flags) == 12, "cm_cost_params is 16 bytes");
static_assert(CM_COST_MAX_AXIS == CM_COST_MAX_AXIS_DEV && CM_COST_MAX_RADIUS_CELLS == 256, "the row pass's LDS row and the largest table");

int cm_map_cost_configure(cm_ctx* c, const cm_cost_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_COST, p)) return e;
    uint32_t R = 0;
    if (p) {
        if (const char* why = cm_cost_refusal(c->map.params.cell, p->inscribed_radius, p->inflation_radius, p->cost_scaling,
                                              CM_COST_MAX_RADIUS_CELLS, &R))
            return fail(c, CM_BAD_ARG, why);
        if (p->flags & ~CM_COST_INFLATE_UNKNOWN) return fail(c, CM_BAD_ARG, "unknown flag bits");
        if (c->map.info.nx > CM_COST_MAX_AXIS || c->map.info.ny > CM_COST_MAX_AXIS)
            return fail(c, CM_BAD_ARG, "the map is wider or taller than CM_COST_MAX_AXIS cells");
    }
    return map_cost_configure(c, p, R);
}

int cm_map_cost_update(cm_ctx* c, cm_map_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_COST, false)) return e;
    if (const int e = map_cost_update(c)) return e;
    if (out) *out = c->map.info;
    return CM_OK;
}

// One of the two tables to the host: `bytes` per cell from src.
static int cost_table_to_host(cm_ctx* c, void* host_dst, const void* src, size_t bytes, uint64_t capacity_cells, cm_map_info* info, const char* what) {
    if (const int e = layer_check(c, LAYER_COST, true)) return e;
    if (info) *info = c->map.info;
    const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    return copy_out(c, host_dst, src, n, bytes, capacity_cells, what);
}

int cm_map_cost_copy(cm_ctx* c, uint8_t* host_dst, uint64_t capacity_cells, cm_map_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return cost_table_to_host(c, host_dst, c->cost.cells, 1, capacity_cells, info, "cost destination too small");
}

int cm_map_dist_copy(cm_ctx* c, uint32_t* host_dst, uint64_t capacity_cells, cm_map_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return cost_table_to_host(c, host_dst, c->cost.dist2, sizeof(uint32_t), capacity_cells, info, "distance destination too small");
}

int cm_map_cost_device(cm_ctx* c, const void** cost, const void** dist2, cm_map_info* info) {
    if (!c) return CM_BAD_ARG;
    if (cost) *cost = nullptr;
    if (dist2) *dist2 = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_COST, true)) return e;
    if (info) *info = c->map.info;
    if (cost) *cost = c->cost.cells;
    if (dist2) *dist2 = c->cost.dist2;
    return CM_OK;
}

int cm_map_cost_table_copy(cm_ctx* c, uint8_t* host_dst, uint64_t capacity, uint64_t* n) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_COST, false)) return e;
    return table_out(c, host_dst, c->cost.lut_host, capacity, n, "cost table destination too small");
}

static_assert(sizeof(cm_plan_params) == 16 && sizeof(cm_plan_info) == 16 && sizeof(cm_path_info) == 32, "the plan layer's three structs");
static_assert(CM_PATH_FOUND == CM_PLAN_PATH_FOUND_DEV && CM_PATH_UNREACHABLE == CM_PLAN_PATH_UNREACHABLE_DEV &&
              CM_PATH_TRUNCATED == CM_PLAN_PATH_TRUNCATED_DEV, "k_plan_path writes cm_path_info's status values");

int cm_map_plan_configure(cm_ctx* c, const cm_plan_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_PLAN, p)) return e;
    if (p) {
        if (p->neutral < 1u || p->neutral > 255u) return fail(c, CM_BAD_ARG, "neutral must lie in 1..255");
        if (p->cost_factor_q8 > 256u) return fail(c, CM_BAD_ARG, "cost_factor_q8 must lie in 0..256");
        if (p->flags & ~CM_PLAN_ALLOW_UNKNOWN) return fail(c, CM_BAD_ARG, "unknown flag bits");
        const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
        if (p->max_path_cells < 1u || p->max_path_cells > n) return fail(c, CM_BAD_ARG, "max_path_cells must lie in 1..nx * ny");
        const uint64_t w_max = p->neutral + ((252u * p->cost_factor_q8) >> 8);
        if (7u * w_max * (n - 1u) > 0xFFFFFFFEull)
            return fail(c, CM_BAD_ARG, "the window is too large for these weights: 7 * w_max * (nx * ny - 1) exceeds 0xFFFFFFFE");
    }
    return map_plan_configure(c, p);
}

int cm_map_plan_update(cm_ctx* c, float gx, float gy, cm_plan_info* out, cm_map_info* map) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_PLAN, false)) return e;
    if (const int e = layer_fresh_check(c, LAYER_COST)) return e;
    uint32_t goal[2];
    if (!map_window_cell(c, gx, gy, goal)) return fail(c, CM_BAD_ARG, "the goal is not finite or lies outside the map's window");
    if (const int e = map_plan_update(c, goal)) return e;
    if (out) *out = c->plan_layer.info;
    if (map) *map = c->map.info;
    return CM_OK;
}

int cm_map_plan_copy(cm_ctx* c, uint32_t* host_dst, uint64_t capacity_cells, cm_plan_info* info, cm_map_info* map) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_PLAN, true)) return e;
    if (info) *info = c->plan_layer.info;
    if (map) *map = c->map.info;
    const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    return copy_out(c, host_dst, c->plan_layer.pot, n, sizeof(uint32_t), capacity_cells, "potential destination too small");
}

int cm_map_plan_device(cm_ctx* c, const void** pot, cm_plan_info* info, cm_map_info* map) {
    if (!c) return CM_BAD_ARG;
    if (pot) *pot = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_PLAN, true)) return e;
    if (info) *info = c->plan_layer.info;
    if (map) *map = c->map.info;
    if (pot) *pot = c->plan_layer.pot;
    return CM_OK;
}

int cm_map_plan_path(cm_ctx* c, float sx, float sy, uint32_t* host_dst, uint64_t capacity, cm_path_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_PLAN, true)) return e;
    uint32_t start[2], head[CM_PLAN_PATH_HEAD];
    if (!map_window_cell(c, sx, sy, start)) return fail(c, CM_BAD_ARG, "the start is not finite or lies outside the map's window");
    if (const int e = map_plan_path(c, start, head)) return e;
    const uint64_t n = head[0];
    if (info) *info = cm_path_info{{start[0], start[1]}, {c->plan_layer.info.goal[0], c->plan_layer.info.goal[1]}, head[0], head[1], head[2], 0u};
    return copy_out(c, host_dst, c->plan_layer.path + CM_PLAN_PATH_HEAD, n, sizeof(uint32_t), capacity, "path destination too small", true);
}

static_assert(sizeof(cm_traj_params) == 24 && sizeof(cm_traj_window) == 32 && sizeof(cm_traj_score) == 32 && sizeof(cm_traj_info) == 24,
              "the rollout layer's four structs");
static_assert(sizeof(CmTrajScoreDev) == sizeof(cm_traj_score) && offsetof(cm_traj_score, total) == offsetof(CmTrajScoreDev, total) &&
                  offsetof(cm_traj_score, end_x) == offsetof(CmTrajScoreDev, end_x), "k_traj_roll writes cm_traj_score");
static_assert(CM_TRAJ_VALID == CM_TRAJ_VALID_DEV && CM_TRAJ_COLLISION == CM_TRAJ_COLLISION_DEV && CM_TRAJ_OFF_MAP == CM_TRAJ_OFF_MAP_DEV &&
                  CM_TRAJ_NO_POTENTIAL == CM_TRAJ_NO_POTENTIAL_DEV && CM_TRAJ_HEADINGS == CM_TRAJ_HEADINGS_DEV &&
                  CM_TRAJ_MAX_SAMPLES == CM_TRAJ_MAX_SAMPLES_DEV && CM_TRAJ_MAX_STEPS == CM_TRAJ_MAX_STEPS_DEV && CM_TRAJ_MAX_FOOT == CM_TRAJ_MAX_FOOT_DEV,
              "the kernels' constants");

int cm_traj_directions(float* cos_sin, uint64_t capacity_pairs) {
    if (!cos_sin) return CM_BAD_ARG;
    if (capacity_pairs < CM_TRAJ_HEADINGS) return CM_CAPACITY;
    std::memcpy(cos_sin, traj_direction_table(), 2 * CM_TRAJ_HEADINGS * sizeof(float));
    return CM_OK;
}

int cm_map_traj_configure(cm_ctx* c, const cm_traj_params* p, const float* foot_xy, uint32_t n_foot) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_TRAJ, p)) return e;
    if (!p) return map_traj_configure(c, nullptr, nullptr, 0);
    if (p->nv < 1u || p->nw < 1u || static_cast<uint64_t>(p->nv) * p->nw > CM_TRAJ_MAX_SAMPLES)
        return fail(c, CM_BAD_ARG, "nv and nw must be at least 1 and nv * nw at most CM_TRAJ_MAX_SAMPLES");
    if (p->n_steps < 1u || p->n_steps > CM_TRAJ_MAX_STEPS) return fail(c, CM_BAD_ARG, "n_steps must lie in 1..CM_TRAJ_MAX_STEPS");
    if (p->flags & ~CM_TRAJ_ALLOW_UNKNOWN) return fail(c, CM_BAD_ARG, "unknown flag bits");
    if (n_foot < 1u || n_foot > CM_TRAJ_MAX_FOOT) return fail(c, CM_BAD_ARG, "n_foot must lie in 1..CM_TRAJ_MAX_FOOT");
    if (!foot_xy) return fail(c, CM_BAD_ARG, "no footprint");
    for (uint32_t i = 0; i < 2u * n_foot; ++i)
        if (!std::isfinite(foot_xy[i])) return fail(c, CM_BAD_ARG, "a footprint coordinate is not finite");
    return map_traj_configure(c, p, foot_xy, n_foot);
}

int cm_map_traj_evaluate(cm_ctx* c, const cm_traj_window* w, cm_traj_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_TRAJ, false)) return e;
    if (const int e = layer_fresh_check(c, LAYER_PLAN)) return e;
    if (!w) return fail(c, CM_BAD_ARG, "no window");
    for (const float v : {w->x, w->y, w->yaw, w->v_lo, w->v_hi, w->w_lo, w->w_hi, w->dt})
        if (!std::isfinite(v)) return fail(c, CM_BAD_ARG, "a window value is not finite");
    if (w->v_hi < w->v_lo) return fail(c, CM_BAD_ARG, "v_hi is below v_lo");
    if (w->w_hi < w->w_lo) return fail(c, CM_BAD_ARG, "w_hi is below w_lo");
    if (!(w->dt > 0.0f)) return fail(c, CM_BAD_ARG, "dt must be above 0");
    if (std::fabs(w->yaw) > 1024.0f) return fail(c, CM_BAD_ARG, "|yaw| is above 1024");
    uint32_t start[2];
    if (!map_window_cell(c, w->x, w->y, start)) return fail(c, CM_BAD_ARG, "the start's cell does not exist or lies outside the map's window");
    // (traj_info holds the last command by value: a refusal below leaves the fresh scores and their info alone)
    std::vector<float>& sv = c->traj.v;
    std::vector<float>& sw = c->traj.w;
    traj_samples(w->v_lo, w->v_hi, c->traj.params.nv, sv.data());
    traj_samples(w->w_lo, w->w_hi, c->traj.params.nw, sw.data());
    for (const float v : sv)
        if (!std::isfinite(v) || !std::isfinite(static_cast<float>(v * w->dt))) return fail(c, CM_BAD_ARG, "a sample or its step length is not finite");
    for (const float wj : sw)
        if (!std::isfinite(wj) || std::fabs(static_cast<double>(wj) * static_cast<double>(w->dt)) >= 3.141592653589793)
            return fail(c, CM_BAD_ARG, "a turn of pi or more per step: |w_j * dt| must stay below pi");
    if (const int e = map_traj_evaluate(c, *w, start)) return e;
    if (out) *out = c->traj.info;
    return CM_OK;
}

int cm_map_traj_copy(cm_ctx* c, cm_traj_score* host_dst, uint64_t capacity, cm_traj_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_TRAJ, true)) return e;
    if (info) *info = c->traj.info;
    const uint64_t n = static_cast<uint64_t>(c->traj.params.nv) * c->traj.params.nw;
    return copy_out(c, host_dst, c->traj.scores, n, sizeof(cm_traj_score), capacity, "score destination too small");
}

int cm_map_traj_device(cm_ctx* c, const void** scores, cm_traj_info* info) {
    if (!c) return CM_BAD_ARG;
    if (scores) *scores = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_TRAJ, true)) return e;
    if (info) *info = c->traj.info;
    if (scores) *scores = c->traj.scores;
    return CM_OK;
}

static_assert(sizeof(cm_frontier_params) == 20 && sizeof(cm_frontier) == 40 && sizeof(cm_frontier_info) == 32 && offsetof(cm_frontier_info, best_score) == 24,
              "the frontier layer's three structs");
static_assert(sizeof(CmFrontEntryDev) == sizeof(cm_frontier) && offsetof(cm_frontier, sum_x) == offsetof(CmFrontEntryDev, sum_x) &&
                  offsetof(cm_frontier, min_pot) == offsetof(CmFrontEntryDev, key) && offsetof(cm_frontier, x0) == offsetof(CmFrontEntryDev, box01),
              "k_front_best writes cm_frontier");
static_assert(CM_FRONTIER_NONE == CM_FRONT_NONE_DEV && CM_FRONTIER_MAX_TABLE == CM_FRONT_MAX_TABLE_DEV && CM_FRONTIER_NONE == CM_PLAN_UNREACHABLE,
              "the kernels' constants");

int cm_map_frontier_configure(cm_ctx* c, const cm_frontier_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_FRONT, p)) return e;
    if (!p) return map_frontier_configure(c, nullptr);
    if (p->min_cells < 1u) return fail(c, CM_BAD_ARG, "min_cells must be at least 1");
    if (p->max_frontiers < 1u || p->max_frontiers > CM_FRONTIER_MAX_TABLE) return fail(c, CM_BAD_ARG, "max_frontiers must lie in 1..CM_FRONTIER_MAX_TABLE");
    if (p->max_cost > 252u) return fail(c, CM_BAD_ARG, "max_cost must lie in 0..252");
    if (c->map.info.nx > 0xFFFFu || c->map.info.ny > 0xFFFFu) return fail(c, CM_BAD_ARG, "the window is too large for a 16-bit box");
    return map_frontier_configure(c, p);
}

int cm_map_frontier_update(cm_ctx* c, cm_frontier_info* out, cm_map_info* map) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_FRONT, false)) return e;
    if (const int e = layer_fresh_check(c, LAYER_PLAN)) return e;
    if (const int e = map_frontier_update(c)) return e;
    if (out) *out = c->front.info;
    if (map) *map = c->map.info;
    return CM_OK;
}

int cm_map_frontier_copy(cm_ctx* c, cm_frontier* host_dst, uint64_t capacity, cm_frontier_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_FRONT, true)) return e;
    if (info) *info = c->front.info;
    const uint64_t n = c->front.info.n_written;
    return copy_out(c, host_dst, c->front.table, n, sizeof(cm_frontier), capacity, "frontier destination too small", true);
}

int cm_map_frontier_labels_copy(cm_ctx* c, uint32_t* host_dst, uint64_t capacity_cells, cm_frontier_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_FRONT, true)) return e;
    if (info) *info = c->front.info;
    const uint64_t n = static_cast<uint64_t>(c->map.info.nx) * c->map.info.ny;
    return copy_out(c, host_dst, c->front.labels, n, sizeof(uint32_t), capacity_cells, "label destination too small");
}

int cm_map_frontier_device(cm_ctx* c, const void** labels, const void** table, cm_frontier_info* info) {
    if (!c) return CM_BAD_ARG;
    if (labels) *labels = nullptr;
    if (table) *table = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_FRONT, true)) return e;
    if (info) *info = c->front.info;
    if (labels) *labels = c->front.labels;
    if (table) *table = c->front.table;
    return CM_OK;
}

static_assert(sizeof(cm_match_params) == 28 && sizeof(cm_match_result) == 96 && offsetof(cm_match_result, sub) == 32 &&
                  offsetof(cm_match_result, pose) == 48, "the matching layer's two structs");
static_assert(CM_MATCH_MAX_SHIFT == CM_MATCH_MAX_SHIFT_DEV && 2 * CM_MATCH_MAX_ANGLES + 1 == CM_MATCH_MAX_ANGLES_DEV &&
                  CM_MATCH_MAX_CANDIDATES == CM_GRID_MAX_CELLS, "the kernels' constants");

int cm_match_table(float cell, float sigma, float max_dist, uint8_t* dst, uint64_t capacity, uint64_t* n) {
    uint32_t R = 0;
    if (!dst || cm_match_refusal(cell, sigma, max_dist, CM_MATCH_MAX_RADIUS_CELLS, &R)) return CM_BAD_ARG;
    const uint64_t n_lut = static_cast<uint64_t>(R) * R + 1;
    if (n) *n = n_lut;
    if (n_lut > capacity) return CM_CAPACITY;
    cm_match_table_build(cell, sigma, max_dist, R, dst);
    return CM_OK;
}

// What the two matchers' configure calls refuse in the same words: the field, then the angle candidates; the flag bits come
// last in both (match_flags_check), behind the refusals each has of its own.
static int match_field_check(cm_ctx* c, float sigma, float max_dist, uint32_t n_a, uint32_t a_stride, uint32_t* R) {
    if (const char* why = cm_match_refusal(c->map.params.cell, sigma, max_dist, CM_MATCH_MAX_RADIUS_CELLS, R)) return fail(c, CM_BAD_ARG, why);
    if (n_a > CM_MATCH_MAX_ANGLES) return fail(c, CM_BAD_ARG, "n_a exceeds CM_MATCH_MAX_ANGLES");
    if (a_stride == 0u) return fail(c, CM_BAD_ARG, "a_stride must be at least 1");
    if (static_cast<uint64_t>(n_a) * a_stride > 1024u) return fail(c, CM_BAD_ARG, "n_a * a_stride exceeds 1024 (a quarter turn)");
    return CM_OK;
}
static int match_flags_check(cm_ctx* c, uint32_t flags) {
    return (flags & ~CM_MATCH_SUBCELL) ? fail(c, CM_BAD_ARG, "unknown flag bits") : CM_OK;
}

int cm_map_match_configure(cm_ctx* c, const cm_match_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_MATCH, p)) return e;
    uint32_t R = 0;
    if (p) {
        if (const int e = match_field_check(c, p->sigma, p->max_dist, p->n_a, p->a_stride, &R)) return e;
        if (p->wx > CM_MATCH_MAX_SHIFT || p->wy > CM_MATCH_MAX_SHIFT) return fail(c, CM_BAD_ARG, "wx or wy exceeds CM_MATCH_MAX_SHIFT");
        if ((2ull * p->n_a + 1u) * (2ull * p->wx + 1u) * (2ull * p->wy + 1u) > CM_MATCH_MAX_CANDIDATES)
            return fail(c, CM_BAD_ARG, "more than CM_MATCH_MAX_CANDIDATES candidates");
        if (const int e = match_flags_check(c, p->flags)) return e;
    }
    return map_match_configure(c, p, R);
}

int cm_map_match_evaluate(cm_ctx* c, const float pose[12], cm_match_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MATCH, false)) return e;
    if (const int e = centroid_result_check(c)) return e;
    if (c->map.info.n_frames == 0) return fail(c, CM_BAD_ARG, "the map holds no frame (cm_map_integrate first)");
    if (const int e = cost_fresh_check(c)) return e;
    int v[2];
    if (const int e = pose_check(c, pose, v)) return e;
    if (const int e = map_match_evaluate(c, pose)) return e;
    if (out) *out = c->match.result;
    return CM_OK;
}

static uint64_t match_entries(const cm_ctx* c) {
    const cm_match_params& q = c->match.params;
    return (2ull * q.n_a + 1u) * (2ull * q.wx + 1u) * (2ull * q.wy + 1u);
}

int cm_map_match_copy(cm_ctx* c, uint32_t* host_dst, uint64_t capacity, cm_match_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MATCH, true)) return e;
    if (out) *out = c->match.result;
    const uint64_t n = match_entries(c);
    return copy_out(c, host_dst, c->match.vol, n, sizeof(uint32_t), capacity, "score destination too small");
}

int cm_map_match_device(cm_ctx* c, const void** scores, cm_match_result* out) {
    if (!c) return CM_BAD_ARG;
    if (scores) *scores = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MATCH, true)) return e;
    if (out) *out = c->match.result;
    if (scores) *scores = c->match.vol;
    return CM_OK;
}

int cm_map_match_table_copy(cm_ctx* c, uint8_t* host_dst, uint64_t capacity, uint64_t* n) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MATCH, false)) return e;
    return table_out(c, host_dst, c->match.lut_host, capacity, n, "field table destination too small");
}

static_assert(sizeof(cm_mcl_params) == 40 && offsetof(cm_mcl_params, seed) == 32 && sizeof(cm_mcl_particle) == 24 && sizeof(cm_mcl_weight) == 8 &&
                  sizeof(cm_mcl_info) == 176 && offsetof(cm_mcl_info, gen) == 16 && offsetof(cm_mcl_info, sum_w) == 48 && offsetof(cm_mcl_info, n_eff) == 120,
              "the localisation layer's four structs");
static_assert(sizeof(CmMclParticleDev) == sizeof(cm_mcl_particle) && offsetof(cm_mcl_particle, acc) == offsetof(CmMclParticleDev, acc) &&
                  offsetof(cm_mcl_particle, parent) == offsetof(CmMclParticleDev, parent) && sizeof(CmMclWeightDev) == sizeof(cm_mcl_weight) &&
                  offsetof(cm_mcl_weight, weight) == offsetof(CmMclWeightDev, weight),
              "the kernels write cm_mcl_particle and cm_mcl_weight");
static_assert(CM_MCL_MAX_PARTICLES == CM_MCL_MAX_PARTICLES_DEV && CM_MCL_MAX_BEAMS == CM_MCL_MAX_BEAMS_DEV && CM_MCL_MAX_RANGE_CELLS == CM_MCL_MAX_RANGE_DEV &&
                  CM_MCL_MAX_BEAMS * 8 <= 65536 && CM_MCL_MAX_PARTICLES <= 64 * CM_MCL_ONE_BLOCK &&
                  ((2ull * CM_MCL_MAX_RANGE_CELLS + 1) * (2ull * CM_MCL_MAX_RANGE_CELLS + 1) + 31) / 32 <= 1ull * CM_MCL_BLOCK * CM_MCL_ONE_BLOCK &&
                  (CM_GRID_MAX_CELLS + 31) / 32 <= CM_MCL_BLOCK * CM_MCL_ONE_BLOCK,
              "the kernels' constants; the staged beams fit 64 KiB of LDS; a bitmap's block counts fit one workgroup's scan");

int cm_mcl_draws(uint64_t seed, uint64_t gen, uint32_t first_p, uint32_t n_p, uint32_t i, uint64_t* dst) {
    if (!dst || i >= 256u || static_cast<uint64_t>(first_p) + n_p > (1ull << 32)) return CM_BAD_ARG;
    const unsigned long long base = cm_mcl_base(seed, gen);
    for (uint32_t k = 0; k < n_p; ++k) dst[k] = cm_mcl_draw(base, first_p + k, i);
    return CM_OK;
}

int cm_map_mcl_configure(cm_ctx* c, const cm_mcl_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_MCL, p)) return e;
    uint32_t R = 0;
    if (p) {
        if (p->n_particles < 1u || p->n_particles > CM_MCL_MAX_PARTICLES) return fail(c, CM_BAD_ARG, "n_particles must lie in 1..CM_MCL_MAX_PARTICLES");
        if (p->max_beams < 1u || p->max_beams > CM_MCL_MAX_BEAMS) return fail(c, CM_BAD_ARG, "max_beams must lie in 1..CM_MCL_MAX_BEAMS");
        if (p->range_cells < 1u || p->range_cells > CM_MCL_MAX_RANGE_CELLS) return fail(c, CM_BAD_ARG, "range_cells must lie in 1..CM_MCL_MAX_RANGE_CELLS");
        if (const char* why = cm_match_refusal(c->map.params.cell, p->sigma, p->max_dist, CM_MATCH_MAX_RADIUS_CELLS, &R)) return fail(c, CM_BAD_ARG, why);
        if (!std::isfinite(p->tau) || !(p->tau > 0.0f)) return fail(c, CM_BAD_ARG, "tau must be finite and > 0");
        if (!std::isfinite(p->resample_frac) || !(p->resample_frac >= 0.0f && p->resample_frac <= 1.0f))
            return fail(c, CM_BAD_ARG, "resample_frac must be finite and lie in 0..1");
        if (p->flags & ~CM_MCL_RESAMPLE_ALWAYS) return fail(c, CM_BAD_ARG, "unknown flag bits");
    }
    return map_mcl_configure(c, p, R);
}

static int particles_check(cm_ctx* c) {
    return c->mcl.init ? CM_OK : fail(c, CM_BAD_ARG, "the particles are not initialised (cm_map_mcl_init_pose or cm_map_mcl_init_uniform first)");
}

// The refusals every call on a configured localisation layer shares: the particles come before the stale weights.
static int mcl_check(cm_ctx* c, bool need_particles, bool read) {
    if (const int e = layer_check(c, LAYER_MCL, false)) return e;
    if (need_particles)
        if (const int e = particles_check(c)) return e;
    return read ? layer_fresh_check(c, LAYER_MCL) : CM_OK;
}

// A centre or a motion (x, y, yaw) and its three standard deviations: what init_pose and predict refuse about them.
static int mcl_values_check(cm_ctx* c, const float v[6]) {
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(v[k])) return fail(c, CM_BAD_ARG, "a value is not finite");
    if (std::fabs(v[2]) > 1024.0f) return fail(c, CM_BAD_ARG, "|yaw| is above 1024");
    for (int k = 3; k < 6; ++k)
        if (v[k] < 0.0f || v[k] > 1024.0f) return fail(c, CM_BAD_ARG, "a standard deviation must lie in 0..1024");
    return CM_OK;
}

int cm_map_mcl_init_pose(cm_ctx* c, float x0, float y0, float yaw0, float sd_x, float sd_y, float sd_yaw) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, false, false)) return e;
    const float v[6] = {x0, y0, yaw0, sd_x, sd_y, sd_yaw};
    if (const int e = mcl_values_check(c, v)) return e;
    return map_mcl_init_pose(c, v);
}

int cm_map_mcl_init_uniform(cm_ctx* c) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, false, false)) return e;
    if (c->map.info.n_frames == 0) return fail(c, CM_BAD_ARG, "the map holds no frame (cm_map_integrate or cm_map_load first)");
    return map_mcl_init_uniform(c);
}

int cm_map_mcl_predict(cm_ctx* c, float d_fwd, float d_left, float d_yaw, float sd_fwd, float sd_left, float sd_yaw) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, false)) return e;
    const float v[6] = {d_fwd, d_left, d_yaw, sd_fwd, sd_left, sd_yaw};
    if (const int e = mcl_values_check(c, v)) return e;
    return map_mcl_predict(c, v);
}

int cm_map_mcl_update(cm_ctx* c, cm_mcl_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, false, false)) return e;
    if (const int e = centroid_result_check(c)) return e;
    if (c->map.info.n_frames == 0) return fail(c, CM_BAD_ARG, "the map holds no frame (cm_map_integrate first)");
    if (const int e = cost_fresh_check(c)) return e;
    if (const int e = particles_check(c)) return e;
    if (const int e = map_mcl_update(c)) return e;
    if (out) *out = c->mcl.info;
    return CM_OK;
}

int cm_map_mcl_copy(cm_ctx* c, cm_mcl_particle* host_dst, uint64_t capacity) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, false)) return e;
    const uint64_t n = c->mcl.params.n_particles;
    return copy_out(c, host_dst, c->mcl.parts[c->mcl.cur], n, sizeof(cm_mcl_particle), capacity, "particle destination too small");
}

int cm_map_mcl_weights_copy(cm_ctx* c, cm_mcl_weight* host_dst, uint64_t capacity, cm_mcl_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, true)) return e;
    if (info) *info = c->mcl.info;
    const uint64_t n = c->mcl.params.n_particles;
    return copy_out(c, host_dst, c->mcl.wts, n, sizeof(cm_mcl_weight), capacity, "weight destination too small");
}

int cm_map_mcl_device(cm_ctx* c, const void** particles, const void** weights, cm_mcl_info* info) {
    if (!c) return CM_BAD_ARG;
    if (particles) *particles = nullptr;
    if (weights) *weights = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, true)) return e;
    if (info) *info = c->mcl.info;
    if (particles) *particles = c->mcl.parts[c->mcl.cur];
    if (weights) *weights = c->mcl.wts;
    return CM_OK;
}

static_assert(sizeof(cm_mcl_beam_params) == 24 && offsetof(cm_mcl_beam_params, flags) == 20 && sizeof(cm_mcl_beam_info) == 56 &&
                  offsetof(cm_mcl_beam_info, n_skipped) == 48 && CM_MCL_BEAM_MAX_OVER == CM_MCL_BEAM_MAX_OVER_DEV && CM_MCL_BEAM_MAX_OVER == CM_CAST_MAX_OVER && CM_MCL_BEAM_MAX_D == CM_CAST_MAX_D,
              "the beam model's two structs; the kernel's constant");

int cm_mcl_beam_table(const cm_mcl_beam_params* p, float cell, uint8_t* dst, uint64_t capacity) {
    if (!p || !dst || cm_mcl_beam_refusal(*p, cell)) return CM_BAD_ARG;
    if (capacity < 2ull * p->over_cells + 3u) return CM_CAPACITY;
    cm_mcl_beam_table_build(*p, cell, dst);
    return CM_OK;
}

int cm_map_mcl_beam_configure(cm_ctx* c, const cm_mcl_beam_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MCL, false)) return e;
    if (p)
        if (const char* why = cm_mcl_beam_refusal(*p, c->map.params.cell)) return fail(c, CM_BAD_ARG, why);
    return map_mcl_beam_configure(c, p);
}

int cm_map_mcl_beam_info_copy(cm_ctx* c, cm_mcl_beam_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, true)) return e;
    if (!c->mcl.beam_info_have) return fail(c, CM_BAD_ARG, "the last cm_map_mcl_update ran without the beam model (cm_map_mcl_beam_configure first)");
    if (!out) return fail(c, CM_BAD_ARG, "no destination");
    *out = c->mcl.beam_info;
    return CM_OK;
}

static_assert(sizeof(cm_mcl_hyp_params) == 40 && offsetof(cm_mcl_hyp_params, flags) == 32 && sizeof(cm_mcl_hyp) == 136 && offsetof(cm_mcl_hyp, sum_w) == 16 &&
                  offsetof(cm_mcl_hyp, share) == 80 && sizeof(cm_mcl_hyp_info) == 72 && offsetof(cm_mcl_hyp_info, sum_s) == 32 &&
                  CM_MCL_HYP_MAX == CM_MCL_HYP_MAX_DEV && sizeof(CmMclHypRecDev) == 88,
              "the three structs of the hypotheses; the kernels' constant and record");

int cm_mcl_kld_bound(uint32_t k, float err, float z, uint32_t* out) {
    if (!out || !std::isfinite(err) || !(err > 0.0f && err <= 1.0f) || !std::isfinite(z) || !(z > 0.0f)) return CM_BAD_ARG;
    if (k <= 1u) {
        *out = 1u;
        return CM_OK;
    }
    const double k1 = static_cast<double>(k - 1u);
    const double a = 2.0 / (9.0 * k1);
    const double b = (1.0 - a) + std::sqrt(a) * static_cast<double>(z);
    const double n = std::ceil((k1 / (2.0 * static_cast<double>(err))) * ((b * b) * b));
    *out = !(n <= 4294967295.0) ? 0xFFFFFFFFu : n < 1.0 ? 1u : static_cast<uint32_t>(n);
    return CM_OK;
}

int cm_map_mcl_hyp_configure(cm_ctx* c, const cm_mcl_hyp_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_MCL, false)) return e;
    if (p) {
        if (p->bin_q < 64u || p->bin_q > 1048576u) return fail(c, CM_BAD_ARG, "bin_q must lie in 64..1048576");
        if (p->heading_bits > 8u) return fail(c, CM_BAD_ARG, "heading_bits must lie in 0..8");
        if (p->max_hyp < 1u || p->max_hyp > CM_MCL_HYP_MAX) return fail(c, CM_BAD_ARG, "max_hyp must lie in 1..CM_MCL_HYP_MAX");
        if (p->inject_max > c->mcl.params.n_particles - 1u) return fail(c, CM_BAD_ARG, "inject_max is above n_particles - 1");
        if (!std::isfinite(p->alpha_slow) || !std::isfinite(p->alpha_fast) || !(0.0f <= p->alpha_slow && p->alpha_slow <= p->alpha_fast && p->alpha_fast <= 1.0f))
            return fail(c, CM_BAD_ARG, "the alphas must be finite with 0 <= alpha_slow <= alpha_fast <= 1");
        if (!std::isfinite(p->kld_err) || !(p->kld_err > 0.0f && p->kld_err <= 1.0f)) return fail(c, CM_BAD_ARG, "kld_err must be finite and lie in 0 < kld_err <= 1");
        if (!std::isfinite(p->kld_z) || !(p->kld_z > 0.0f)) return fail(c, CM_BAD_ARG, "kld_z must be finite and > 0");
        if (p->flags || p->_pad) return fail(c, CM_BAD_ARG, "unknown flag bits");
    }
    return map_mcl_hyp_configure(c, p);
}

int cm_map_mcl_hyp_copy(cm_ctx* c, cm_mcl_hyp* host_dst, uint64_t capacity, cm_mcl_hyp_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = mcl_check(c, true, true)) return e;
    if (!c->mcl.hyp_have) return fail(c, CM_BAD_ARG, "the last cm_map_mcl_update ran without the hypotheses (cm_map_mcl_hyp_configure first)");
    if (info) *info = c->mcl.hyp_info;
    const uint64_t n = c->mcl.hyp_out.size();
    if (capacity < n) return fail(c, CM_CAPACITY, "hypothesis destination too small");
    if (!host_dst) return fail(c, CM_BAD_ARG, "no destination");
    std::memcpy(host_dst, c->mcl.hyp_out.data(), n * sizeof(cm_mcl_hyp));
    return CM_OK;
}

static_assert(sizeof(cm_cast_params) == 16 && sizeof(cm_cast_pose) == 12 && offsetof(cm_cast_pose, h) == 8 && sizeof(cm_cast_ray) == 8 &&
                  offsetof(cm_cast_ray, status) == 2 && offsetof(cm_cast_ray, jx) == 4 && sizeof(cm_cast_info) == 24 && offsetof(cm_cast_info, n_max) == 8,
              "the cast layer's four structs");
static_assert(sizeof(CmCastRayDev) == sizeof(cm_cast_ray) && offsetof(CmCastRayDev, jy) == offsetof(cm_cast_ray, jy) && sizeof(CmMclParticleDev) % 4 == 0 &&
                  offsetof(CmMclParticleDev, x) == 0 && offsetof(CmMclParticleDev, y) == 4 && offsetof(CmMclParticleDev, h) == 8,
              "the kernel writes cm_cast_ray and reads a particle's x, y, h as a pose's");
static_assert(CM_CAST_MAX_POSES == CM_CAST_MAX_POSES_DEV && CM_CAST_MAX_BEARINGS == CM_CAST_MAX_BEARINGS_DEV && CM_CAST_MAX_RANGE_CELLS == CM_CAST_MAX_RANGE_DEV &&
                  CM_CAST_MAX_RAYS == CM_CAST_MAX_RAYS_DEV && CM_CAST_DIRS == CM_TRAJ_HEADINGS && CM_CAST_NO_ORIGIN == 3 && CM_CAST_WORDS == 4 &&
                  CM_MCL_MAX_PARTICLES <= CM_CAST_MAX_POSES,
              "the kernels' constants; the count words are indexed by status");

int cm_cast_directions(uint32_t range_cells, int16_t* dst, uint64_t capacity_pairs) {
    if (!dst || range_cells < 1u || range_cells > CM_CAST_MAX_RANGE_CELLS) return CM_BAD_ARG;
    if (capacity_pairs < CM_CAST_DIRS) return CM_CAPACITY;
    cast_direction_table(range_cells, dst);
    return CM_OK;
}

int cm_map_cast_configure(cm_ctx* c, const cm_cast_params* p, const uint32_t* bearings) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_CAST, p)) return e;
    if (p) {
        if (p->max_poses < 1u || p->max_poses > CM_CAST_MAX_POSES) return fail(c, CM_BAD_ARG, "max_poses must lie in 1..CM_CAST_MAX_POSES");
        if (p->n_bearings < 1u || p->n_bearings > CM_CAST_MAX_BEARINGS) return fail(c, CM_BAD_ARG, "n_bearings must lie in 1..CM_CAST_MAX_BEARINGS");
        if (p->range_cells < 1u || p->range_cells > CM_CAST_MAX_RANGE_CELLS) return fail(c, CM_BAD_ARG, "range_cells must lie in 1..CM_CAST_MAX_RANGE_CELLS");
        if (static_cast<uint64_t>(p->max_poses) * p->n_bearings > CM_CAST_MAX_RAYS) return fail(c, CM_BAD_ARG, "max_poses * n_bearings is above CM_CAST_MAX_RAYS");
        if (p->flags & ~CM_CAST_PLAIN) return fail(c, CM_BAD_ARG, "unknown flag bits");
    }
    return map_cast_configure(c, p, bearings);
}

// The refusals every call on a configured cast layer shares: a read wants fresh rays, an evaluate a fresh cost table.
static int cast_check(cm_ctx* c, bool read) {
    if (const int e = layer_check(c, LAYER_CAST, read)) return e;
    return read ? CM_OK : cost_fresh_check(c);
}

int cm_map_cast_evaluate(cm_ctx* c, const cm_cast_pose* host_poses, uint32_t n, cm_cast_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = cast_check(c, false)) return e;
    if (n < 1u || n > c->cast.params.max_poses) return fail(c, CM_BAD_ARG, "n must lie in 1..max_poses");
    if (!host_poses) return fail(c, CM_BAD_ARG, "no poses");
    if (const int e = map_cast_evaluate(c, host_poses, n)) return e;
    if (out) *out = c->cast.info;
    return CM_OK;
}

int cm_map_cast_evaluate_mcl(cm_ctx* c, cm_cast_info* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = cast_check(c, false)) return e;
    if (!c->layers[LAYER_MCL].on) return fail(c, CM_BAD_ARG, LAYER_TABLE[LAYER_MCL].absent);
    if (const int e = particles_check(c)) return e;
    if (c->mcl.params.n_particles > c->cast.params.max_poses) return fail(c, CM_BAD_ARG, "n_particles is above max_poses");
    if (const int e = map_cast_evaluate(c, nullptr, c->mcl.params.n_particles)) return e;
    if (out) *out = c->cast.info;
    return CM_OK;
}

int cm_map_cast_copy(cm_ctx* c, cm_cast_ray* host_dst, uint64_t capacity, cm_cast_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = cast_check(c, true)) return e;
    if (info) *info = c->cast.info;
    const uint64_t n = static_cast<uint64_t>(c->cast.info.n_poses) * c->cast.info.n_bearings;
    return copy_out(c, host_dst, c->cast.rays, n, sizeof(cm_cast_ray), capacity, "ray destination too small");
}

int cm_map_cast_device(cm_ctx* c, const void** rays, cm_cast_info* info) {
    if (!c) return CM_BAD_ARG;
    if (rays) *rays = nullptr;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = cast_check(c, true)) return e;
    if (info) *info = c->cast.info;
    if (rays) *rays = c->cast.rays;
    return CM_OK;
}

static_assert(sizeof(cm_match_search_params) == 40 && sizeof(cm_match_search_info) == 84 && offsetof(cm_match_search_info, scored) == 12 &&
                  offsetof(cm_match_search_info, live) == 44 && offsetof(cm_match_search_info, overflow_level) == 80, "the search layer's two structs");
static_assert(CM_MATCH_SEARCH_MAX_SHIFT == CM_MSEARCH_MAX_SHIFT_DEV && CM_MATCH_SEARCH_MAX_DEPTH == CM_MSEARCH_MAX_DEPTH_DEV &&
                  2 * CM_MATCH_SEARCH_MAX_SHIFT < 4096 && 2 * CM_MATCH_MAX_ANGLES + 1 < 256 && CM_MATCH_SEARCH_MAX_NODES == CM_GRID_MAX_CELLS,
              "the kernels' constants; a node is 8 + 12 + 12 bits");

int cm_map_match_search_configure(cm_ctx* c, const cm_match_search_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = configure_check(c, LAYER_SEARCH, p)) return e;
    uint32_t R = 0;
    if (p) {
        if (const int e = match_field_check(c, p->sigma, p->max_dist, p->n_a, p->a_stride, &R)) return e;
        if (p->wx > CM_MATCH_SEARCH_MAX_SHIFT || p->wy > CM_MATCH_SEARCH_MAX_SHIFT) return fail(c, CM_BAD_ARG, "wx or wy exceeds CM_MATCH_SEARCH_MAX_SHIFT");
        if (p->depth > CM_MATCH_SEARCH_MAX_DEPTH) return fail(c, CM_BAD_ARG, "depth exceeds CM_MATCH_SEARCH_MAX_DEPTH");
        if (p->max_nodes == 0u || p->max_nodes > CM_MATCH_SEARCH_MAX_NODES) return fail(c, CM_BAD_ARG, "max_nodes must be 1 .. CM_MATCH_SEARCH_MAX_NODES");
        if (p->max_cells == 0u || p->max_cells > CM_MATCH_SEARCH_MAX_NODES) return fail(c, CM_BAD_ARG, "max_cells must be 1 .. CM_MATCH_SEARCH_MAX_NODES");
        const uint64_t rx = (2ull * p->wx + (1ull << p->depth)) >> p->depth, ry = (2ull * p->wy + (1ull << p->depth)) >> p->depth;
        if ((2ull * p->n_a + 1u) * rx * ry > p->max_nodes) return fail(c, CM_BAD_ARG, "more roots than max_nodes");
        if (c->map.info.nx > 65535u || c->map.info.ny > 65535u) return fail(c, CM_BAD_ARG, "the map's window has more than 65535 cells along an axis");
        if (const int e = match_flags_check(c, p->flags)) return e;
    }
    return map_msearch_configure(c, p, R);
}

int cm_map_match_search(cm_ctx* c, const float pose[12], cm_match_result* out, cm_match_search_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_SEARCH, false)) return e;
    if (const int e = centroid_result_check(c)) return e;
    if (c->map.info.n_frames == 0) return fail(c, CM_BAD_ARG, "the map holds no frame (cm_map_integrate first)");
    if (const int e = cost_fresh_check(c)) return e;
    int v[2];
    if (const int e = pose_check(c, pose, v)) return e;
    const int e = map_msearch_evaluate(c, pose);
    if (e == CM_CAPACITY && info) *info = c->msearch.info;
    if (e) return e;
    if (out) *out = c->msearch.result;
    if (info) *info = c->msearch.info;
    return CM_OK;
}

int cm_map_match_search_result(cm_ctx* c, cm_match_result* out, cm_match_search_info* info) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_SEARCH, true)) return e;
    if (out) *out = c->msearch.result;
    if (info) *info = c->msearch.info;
    return CM_OK;
}

int cm_map_match_search_level_copy(cm_ctx* c, uint32_t h, uint8_t* host_dst, uint64_t capacity, uint32_t dims[2]) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = layer_check(c, LAYER_SEARCH, true)) return e;
    if (h > c->msearch.params.depth) return fail(c, CM_BAD_ARG, "no such level (h exceeds depth)");
    const uint32_t pw = c->map.info.nx + (1u << h) - 1u, ph = c->map.info.ny + (1u << h) - 1u;
    if (dims) {
        dims[0] = pw;
        dims[1] = ph;
    }
    const uint64_t n = static_cast<uint64_t>(pw) * ph;
    return copy_out(c, host_dst, c->msearch.pyr + msearch_level_offset(c->map.info.nx, c->map.info.ny, h), n, 1, capacity, "level destination too small");
}

static_assert(sizeof(cm_voxel_normal) == 32 && sizeof(cm_normal_params) == 24, "cm_voxel_normal is 32 bytes, its parameters 24");
static_assert(CM_NORMAL_VALID == CM_NORMAL_VALID_DEV && CM_NORMAL_MAX_K == 64, "the kernels' flag and largest list");

int cm_result_normals(cm_ctx* c, const cm_normal_params* p, cm_voxel_normal* host_dst, uint64_t capacity) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = normals_check(c, p);
    if (e != CM_OK) return e;
    const uint64_t n = c->result.n_out;
    if (n > capacity) return fail(c, CM_CAPACITY, "normals destination too small");
    if (n && !host_dst) return fail(c, CM_BAD_ARG, "null destination");
    e = normals(c, *p);
    if (e != CM_OK || n == 0) return e;
    HIP_TRY(c, hipMemcpyAsync(host_dst, c->nrm_entries, n * sizeof(cm_voxel_normal), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->bytes_d2h += n * sizeof(cm_voxel_normal);
    return CM_OK;
}

int cm_result_normals_device(cm_ctx* c, const cm_normal_params* p, const void** dev_ptr, uint64_t* n) {
    if (!c || !dev_ptr || !n) return CM_BAD_ARG;
    *dev_ptr = nullptr;
    *n = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    int e = normals_check(c, p);
    if (e == CM_OK) e = normals(c, *p);
    if (e != CM_OK) return e;
    *dev_ptr = c->result.n_out ? c->nrm_entries : nullptr;
    *n = c->result.n_out;
    return CM_OK;
}

static_assert(sizeof(cm_align_params) == 128 && sizeof(cm_align_result) == 368 && sizeof(cm_align_corr) == 8,
              "cm_align_params is 128 bytes, cm_align_result 368, a correspondence 8");
static_assert(CM_ALIGN_NONE == CM_ALIGN_NONE_DEV && offsetof(cm_align_result, H) == 96 && offsetof(cm_align_result, n_corr) == 352,
              "the kernels' mark of no match; the outcome's layout");

int cm_result_align(cm_ctx* c, const cm_align_params* p, const void* src_host, uint64_t n_src, cm_align_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    const void* src_dev = nullptr;
    if (const int e = align_check(c, p, src_host, n_src, out)) return e;
    if (const int e = stage_source(c, c->aln_fit, src_host, n_src, "cannot allocate the registration's source", &src_dev)) return e;
    return align(c, *p, src_dev, n_src, out);
}

int cm_result_align_device(cm_ctx* c, const cm_align_params* p, const void* src_dev, uint64_t n_src, cm_align_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (const int e = align_check(c, p, src_dev, n_src, out)) return e;
    return align(c, *p, src_dev, n_src, out);
}

int cm_align_correspondences_copy(cm_ctx* c, cm_align_corr* host_dst, uint64_t capacity, uint64_t* n) {
    if (!c || !n) return CM_BAD_ARG;
    *n = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return copy_correspondences(c, c->aln_fit, sizeof(cm_align_corr), "no alignment since the last merge", host_dst, capacity, n);
}

static_assert(sizeof(cm_ndt_params) == 136 && sizeof(cm_ndt_result) == 376 && sizeof(cm_ndt_corr) == 16,
              "cm_ndt_params is 136 bytes, cm_ndt_result 376, a correspondence 16");
static_assert(CM_NDT_NONE == CM_NDT_NONE_DEV && offsetof(cm_ndt_params, trans_eps) == 24 && offsetof(cm_ndt_result, H) == 96 &&
                  offsetof(cm_ndt_result, n_corr) == 360 && offsetof(cm_ndt_corr, score) == 8,
              "the kernels' mark of no voxel; the layouts");
static_assert(CM_NDT_CONVERGED == CM_ALIGN_CONVERGED && CM_NDT_MAX_ITER_HIT == CM_ALIGN_MAX_ITER_HIT && CM_NDT_FEW == CM_ALIGN_FEW &&
                  CM_NDT_SINGULAR == CM_ALIGN_SINGULAR, "the same four meanings as CM_ALIGN_*");

int cm_result_ndt_align(cm_ctx* c, const cm_ndt_params* p, const void* src_host, uint64_t n_src, cm_ndt_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_cov_params cov;
    const void* src_dev = nullptr;
    if (const int e = ndt_check(c, p, src_host, n_src, out, &cov)) return e;
    if (const int e = stage_source(c, c->ndt_fit, src_host, n_src, "cannot allocate the NDT registration's source", &src_dev)) return e;
    return ndt(c, *p, cov, src_dev, n_src, out);
}

int cm_result_ndt_align_device(cm_ctx* c, const cm_ndt_params* p, const void* src_dev, uint64_t n_src, cm_ndt_result* out) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    cm_cov_params cov;
    if (const int e = ndt_check(c, p, src_dev, n_src, out, &cov)) return e;
    return ndt(c, *p, cov, src_dev, n_src, out);
}

int cm_ndt_correspondences_copy(cm_ctx* c, cm_ndt_corr* host_dst, uint64_t capacity, uint64_t* n) {
    if (!c || !n) return CM_BAD_ARG;
    *n = 0;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    return copy_correspondences(c, c->ndt_fit, sizeof(cm_ndt_corr), "no NDT registration since the last merge", host_dst, capacity, n);
}

int cm_set_ground_removal(cm_ctx* c, const cm_ground_params* g) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (c->pending) return fail(c, CM_BAD_ARG, "cannot change ground removal with a frame in flight");
    if (!g) { c->ground_on = false; return CM_OK; }
    if (g->max_iterations < 1 || g->max_iterations > 100000) return fail(c, CM_BAD_ARG, "max_iterations must be in 1..100000");
    if (!(g->distance_threshold > 0.0f) || !std::isfinite(g->distance_threshold)) return fail(c, CM_BAD_ARG, "distance_threshold must be > 0");
    if (!(g->probability > 0.0f && g->probability < 1.0f)) return fail(c, CM_BAD_ARG, "probability must be in (0, 1)");
    if (g->outlier_radius < 0.0f || !std::isfinite(g->outlier_radius)) return fail(c, CM_BAD_ARG, "outlier_radius must be >= 0");
    CmGroundDev d;
    std::memset(&d, 0, sizeof d);
    for (uint32_t s = 0; s < CM_MAX_SENSORS; ++s) {
        if (g->n_zones[s] > CM_MAX_ZONES) return fail(c, CM_BAD_ARG, "more than CM_MAX_ZONES zones for a sensor");
        d.n_zones[s] = g->n_zones[s];
        for (uint32_t z = 0; z < g->n_zones[s]; ++z) {
            const cm_zone& zn = g->zones[s][z];
            if (!std::isfinite(zn.x_min) || !(zn.x_length >= 0.0f) || !std::isfinite(zn.x_length) || !std::isfinite(zn.z_max_ground))
                return fail(c, CM_BAD_ARG, "zone limits must be finite, x_length >= 0");
            d.x0[s][z] = zn.x_min;
            d.x1[s][z] = zn.x_min + zn.x_length;                          // setFilterLimits(deviation, deviation + length), :57
            d.zmax[s][z] = zn.z_max_ground;
            d.zlo[s][z] = static_cast<float>(static_cast<double>(zn.z_max_ground) + 0.01);   // z_max_ground + 0.01, :91
        }
    }
    d.z_keep_max = g->z_keep_max;
    d.threshold = g->distance_threshold;
    d.probability = g->probability;
    d.max_iterations = g->max_iterations;
    d.optimize = g->optimize_coefficients ? 1u : 0u;
    d.seed = g->seed;
    c->ground = d;
    c->ground_outlier_radius = g->outlier_radius;
    c->ground_outlier_min_nb = g->outlier_min_neighbors;
    c->ground_uploaded = false;
    c->ground_on = true;
    return CM_OK;
}

int cm_ground_copy(cm_ctx* c, void* host_dst, uint64_t capacity, uint64_t* n_points) {
    if (!c || !n_points) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result) return fail(c, CM_BAD_ARG, "no result");
    *n_points = 0;
    if (!c->frame_had_ground) return fail(c, CM_BAD_ARG, "the last frame ran without ground removal");
    return copy_fused(c, c->gmask, host_dst, capacity, n_points, false);
}

int cm_ground_planes(cm_ctx* c, cm_ground_plane* planes, uint32_t capacity) {
    if (!c || !planes) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result || !c->frame_had_ground) return fail(c, CM_BAD_ARG, "the last frame ran without ground removal");
    static_assert(sizeof(cm_ground_plane) == sizeof(CmGroundPlaneDev), "plane record layout");
    const uint32_t n = std::min<uint32_t>(capacity, CM_DEV_MAX_SENSORS * CM_DEV_MAX_ZONES);
    if (c->frame.n_padded == 0) {                      // an empty frame: no band points anywhere
        std::memset(planes, 0, static_cast<size_t>(n) * sizeof(cm_ground_plane));
        return CM_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(planes, c->d_planes, static_cast<size_t>(n) * sizeof(cm_ground_plane), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CM_OK;
}

int cm_local_bounds(cm_ctx* c, const cm_params* p, float min_xyz[3], float max_xyz[3], uint64_t* n_valid) {
    if (!c || !p || !min_xyz || !max_xyz) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) return fail(c, CM_BAD_ARG, "previous frame not waited for (cm_wait)");
    if (c->motion_on) return fail(c, CM_BAD_ARG, "ego-motion compensation is not combined with cm_local_bounds (cm_set_ego_motion(NULL) first)");
    if (c->sor_on) return fail(c, CM_BAD_ARG, "statistical outlier removal is not combined with cm_local_bounds (cm_set_statistical_outlier(NULL) first)");
    for (int a = 0; a < 3; ++a)
        if (!(p->leaf[a] > 0.0f)) return fail(c, CM_BAD_ARG, "leaf must be > 0");
    std::vector<std::unique_lock<std::mutex>> locks;
    // a peek: the clouds stay fresh, and c->frame stays the last frame's. HBM holds the peek's descriptor afterwards, which
    // frame_uploaded records: the merge that follows skips its upload when it builds the same one, and a by-product call
    // that comes first puts c->frame back (frame_on_device).
    CmFrameDev f;
    const int bf = build_frame(c, p, &f, locks);
    if (bf != CM_OK) return bf;
    const float inf = std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; ++a) { min_xyz[a] = inf; max_xyz[a] = -inf; }
    if (n_valid) *n_valid = 0;
    if (f.n_padded == 0) return CM_OK;
    cmk_setup(c->stream, f, c->d_frame, c->d_tiles);
    c->frame_uploaded = f;
    c->frame_uploaded_valid = true;
    uint64_t cnt = 0;
    const int e = measure_bounds(c, f.n_tiles, min_xyz, max_xyz, &cnt);
    if (e != CM_OK) return e;
    if (n_valid) *n_valid = cnt;
    return CM_OK;
}

int cm_merge_partial(cm_ctx* c, const cm_params* p, const float* global_min_max, cm_result* res) {
    return merge_and_wait(c, p, 1, global_min_max, res);
}

int cm_partial_device(cm_ctx* c, const void** dev_entries, uint64_t* n_entries) {
    if (!c || !dev_entries || !n_entries) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result || c->last_mode != 1) return fail(c, CM_BAD_ARG, "no partial table (cm_merge_partial)");
    *dev_entries = c->partial;
    *n_entries = c->result.status == CM_OK ? c->result.n_out : 0;
    return CM_OK;
}

int cm_partial_copy(cm_ctx* c, cm_partial_entry* host_dst, uint64_t capacity) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!c->have_result || c->last_mode != 1) return fail(c, CM_BAD_ARG, "no partial table (cm_merge_partial)");
    const uint64_t n = c->result.status == CM_OK ? c->result.n_out : 0;
    if (n > capacity) return fail(c, CM_CAPACITY, "destination too small");
    if (n == 0) return CM_OK;
    if (!host_dst) return CM_BAD_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(host_dst, c->partial, n * 32, hipMemcpyDefault, c->stream));   // host or device destination
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return CM_OK;
}

int cm_merge_tables(cm_ctx* c, const void* const* dev_tables, const uint64_t* n_entries, uint32_t n_tables,
                    const cm_params* p, cm_result* res) {
    if (!c || !p || !dev_tables || !n_entries || n_tables < 1 || n_tables > CM_MAX_SENSORS) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->pending) return fail(c, CM_BAD_ARG, "previous frame not waited for (cm_wait)");
    return merge_tables(c, dev_tables, n_entries, n_tables, p, res);
}

int cm_set_sensor_time_field(cm_ctx* c, uint32_t sensor, uint32_t offset, uint32_t type) {
    if (!c) return CM_BAD_ARG;
    if (sensor >= c->max_sensors) return fail(c, CM_BAD_ARG, "sensor index out of range");
    if (type != CM_TIME_NONE && type != CM_TIME_F32_S && type != CM_TIME_U32_NS) return fail(c, CM_BAD_ARG, "unknown time field type");
    std::lock_guard<std::mutex> lk(c->slots[sensor].mu);
    c->slots[sensor].time_off = offset;
    c->slots[sensor].time_type = type;
    return CM_OK;
}

int cm_set_ego_motion(cm_ctx* c, const cm_motion* m) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!m) { c->motion_on = false; return CM_OK; }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(m->v[a]) || !std::isfinite(m->w[a])) return fail(c, CM_BAD_ARG, "ego velocity must be finite");
    if (!c->motion_buf) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (!c->motion_buf.once(static_cast<size_t>(c->cap_padded) * 16))
            return fail(c, CM_HIP_ERROR, "could not allocate the compensated clouds' buffer");
    }
    c->motion = *m;
    c->motion_on = true;
    return CM_OK;
}

int cm_set_statistical_outlier(cm_ctx* c, const cm_sor_params* p) {
    if (!c) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!p) { c->sor_on = false; return CM_OK; }
    if (p->mean_k < 1 || p->mean_k > CM_SOR_MAX_K) return fail(c, CM_BAD_ARG, "mean_k must be 1..64");
    if (!std::isfinite(p->std_mul)) return fail(c, CM_BAD_ARG, "std_mul must be finite");
    if (!(p->search_cell >= 0.0f) || !std::isfinite(p->search_cell)) return fail(c, CM_BAD_ARG, "search_cell must be finite and >= 0");
    const size_t npad = c->cap_padded;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!(c->sor_d.once(npad) && c->sor_list.once(npad * 8) && c->sor_words.once(CM_SOR_WORDS) && ensure_mask(c) && ensure_cell_sort(c)))
        return fail(c, CM_HIP_ERROR, "could not allocate the statistical outlier stage's buffers");
    c->sor = *p;
    c->sor_on = true;
    return CM_OK;
}

int cm_get_sor_stats(cm_ctx* c, cm_sor_stats* out) {
    if (!c || !out) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    std::memset(out, 0, sizeof *out);
    if (c->have_result && c->last_sor) *out = c->sor_stats;
    return CM_OK;
}

int cm_sor_distances_copy(cm_ctx* c, float* host_dst, uint64_t capacity, uint64_t* n) {
    if (!c || !n) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    *n = 0;
    if (c->pending) return fail(c, CM_BAD_ARG, "frame in flight (cm_wait first)");
    if (!c->have_result || !c->last_sor) return fail(c, CM_BAD_ARG, "the last frame did not run statistical outlier removal");
    const uint32_t np = c->frame.n_padded;
    if (c->pending_trivial || np == 0 || c->result.status < 0) return CM_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> all(np);
    HIP_TRY(c, hipMemcpyAsync(all.data(), c->sor_d, static_cast<size_t>(np) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t m = 0;
    for (uint32_t v : all) m += v != 0xFFFFFFFFu;
    *n = m;
    if (m > capacity) return fail(c, CM_CAPACITY, "destination too small");
    if (m && !host_dst) return CM_BAD_ARG;
    uint64_t o = 0;
    for (uint32_t v : all)
        if (v != 0xFFFFFFFFu) std::memcpy(host_dst + o++, &v, 4);
    return CM_OK;
}

int cm_get_stage_times(cm_ctx* c, cm_stage_times* out) {
    if (!c || !out) return CM_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->merge_mu);
    if (!(c->flags & CM_FLAG_PROFILE)) return fail(c, CM_BAD_ARG, "context created without CM_FLAG_PROFILE");
    *out = c->stage_times;
    return CM_OK;
}

#ifdef CM_TEST_HOOKS                     // (the test build only: cm_devbuf.hpp's counts of the process)
CM_API int cm_test_device_allocations(uint64_t* live, uint64_t* total) {
    if (!live || !total) return CM_BAD_ARG;
    *live = cm_allocations_live.load();
    *total = cm_allocations_total.load();
    return CM_OK;
}
#endif

int cm_host_alloc(void** ptr, size_t bytes) {
    if (!ptr) return CM_BAD_ARG;
    return hipHostMalloc(ptr, bytes, hipHostMallocDefault) == hipSuccess ? CM_OK : CM_HIP_ERROR;
}

int cm_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return CM_BAD_ARG;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? CM_OK : CM_INTERNAL;
}
int cm_host_unregister(void* ptr) {
    if (!ptr) return CM_BAD_ARG;
    return hipHostUnregister(ptr) == hipSuccess ? CM_OK : CM_INTERNAL;
}
int cm_host_free(void* ptr) {
    return hipHostFree(ptr) == hipSuccess ? CM_OK : CM_HIP_ERROR;
}

}  // extern "C"
