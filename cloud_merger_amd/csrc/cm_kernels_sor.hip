// cm_kernels_sor.hip — statistical outlier removal (pcl::StatisticalOutlierRemoval) on the fused cloud before the voxel
// grid, for gfx950. The stage's input is sorted by a grid of cells `search_cell` wide with the radius stage's
// sort (cm_launch.cpp sor_filter): sorted_pts holds the points in cell order (x, y, z, padded index), the sorted keys lie
// beside them and the (y,z)-row table gives each row's range.
//
//   k_sor_knn<KMAX>(first)  exact k nearest neighbours, one lane per point, the k smallest squared distances kept ascending
//                           in LDS (KMAX floats per lane, lane-interleaved). First launch: the 3x3x3 cells around the point;
//                           it is finished when its k-th distance is no larger than the distance to the nearest face of that
//                           block. The others go onto a list with that k-th distance as a bound. Second launch: the listed
//                           points search row ring by row ring ((y,z) Chebyshev rings), skipping empty rows through the
//                           table and rows beyond the bound, scanning in every row only the cells within the bound in x,
//                           until the next ring lies beyond the k-th distance. Writes d_i per padded index.
//   k_sor_bins              per-exponent bins of d_i and fp32(d_i * d_i): LDS then global 64-bit integer adds (exact)
//   k_sor_threshold         one lane: the exact sums (cm_sor_sum.hpp), mean, stddev, threshold -> the stats record
//   k_sor_mask              keep-mask: double(d_i) > threshold removes the point
// Every kernel leaves at once when the sort's state is not CM_DEV_OK.
// The walks (for_row_cells, for_rows_3x3, for_row_ring), d2_of and kRel are cm_search.hpp's, shared with k_nrm_knn; the
// pruning bounds (axis_gap), x_range, the list and the "finished after the first launch" test are this kernel's own.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"
#include "cm_sor_sum.hpp"

namespace {

// sqrtf correctly rounded: the fp64 root of an fp32 value rounded to fp32 (53 >= 2 * 24 + 2 bits: no double-rounding error).
// (HIP's __fsqrt_rn is the 1-ulp hardware root unless OCML's rounded operations are enabled.)
__device__ __forceinline__ float sqrt_rn(float x) { return static_cast<float>(__dsqrt_rn(static_cast<double>(x))); }

// A lower bound (m) on the distance from the point to any point s or more cells away along one axis: the cell
// assignment floor(x * inv) may round either way by |x| 2^-23.
__device__ __forceinline__ float axis_gap(float s, float cell, float coord) {
    return fmaxf(__fsub_rn(__fmul_rn(__fmul_rn(s, cell), kRel), __fmul_rn(fabsf(coord), 1.0f / (1 << 21))), 0.0f);
}

template <int KMAX>
__global__ __launch_bounds__(CM_BLOCK) void k_sor_knn(const CmFrameDev* __restrict__ fd, const CmFrameState* __restrict__ st,
                                                      const uint32_t* __restrict__ keys_a, const uint32_t* __restrict__ keys_b,
                                                      const float4* __restrict__ pts, const uint2* __restrict__ rows,
                                                      float* __restrict__ dist, uint2* __restrict__ list,
                                                      unsigned int* __restrict__ list_n, uint32_t k, int first) {
    __shared__ float lst[KMAX * CM_BLOCK];
    if (st->status != CM_DEV_OK) return;
    const uint32_t n = st->n_valid;
    const uint32_t n_items = first ? n : *list_n;
    const uint32_t* __restrict__ keys = (st->n_passes & 1u) ? keys_b : keys_a;
    const uint32_t dx = static_cast<uint32_t>(st->div_b[0]), dy = static_cast<uint32_t>(st->div_b[1]),
                   dz = static_cast<uint32_t>(st->div_b[2]);
    const float inv_x = fd->inv_cell[0];
    const float cx = 1.0f / fd->inv_cell[0], cy = 1.0f / fd->inv_cell[1], cz = 1.0f / fd->inv_cell[2];
    const float fbx = static_cast<float>(st->min_b[0]);
    float* my = lst + threadIdx.x;                       // my[j * CM_BLOCK]: the j-th smallest d2 so far
    const float inf = __builtin_inff();
    for (uint32_t t = blockIdx.x * CM_BLOCK + threadIdx.x; t < n_items; t += gridDim.x * CM_BLOCK) {
        const uint2 item = first ? make_uint2(t, __float_as_uint(inf)) : list[t];
        const uint32_t p = item.x;
        const float4 me = pts[p];
        const uint32_t idx = __float_as_uint(me.w);
        if (n <= k) {                                    // degenerate frame: no k neighbours
            dist[idx] = __uint_as_float(0x7FC00000u);
            continue;
        }
        const uint32_t key = keys[p];
        const uint32_t jk = key / dx, i = key - jk * dx, kk = jk / dy, j = jk - kk * dy;
        const float bound0 = __uint_as_float(item.y);   // an upper bound on the k-th d2 (the first launch's), or +inf
        uint32_t cnt = 0;
        auto eff = [&]() { return cnt == k ? my[(k - 1) * CM_BLOCK] : bound0; };
        auto offer = [&](float d2) {
            if (cnt < k) {
                if (!(d2 <= bound0)) return;
                uint32_t q = cnt++;
                for (; q > 0 && my[(q - 1) * CM_BLOCK] > d2; --q) my[q * CM_BLOCK] = my[(q - 1) * CM_BLOCK];
                my[q * CM_BLOCK] = d2;
            } else if (d2 < my[(k - 1) * CM_BLOCK]) {
                uint32_t q = k - 1;
                for (; q > 0 && my[(q - 1) * CM_BLOCK] > d2; --q) my[q * CM_BLOCK] = my[(q - 1) * CM_BLOCK];
                my[q * CM_BLOCK] = d2;
            }
        };
        // one row: the points of cells il..ih (clipped to the grid), the point itself left out
        auto scan_row = [&](uint32_t row, uint32_t il, uint32_t ih) {
            const uint2 r = rows[row];
            for_row_cells(keys, r.x, r.y, row, dx, il, ih, [&](uint32_t q) {
                if (q != p) offer(d2_of(me, pts[q]));
            });
        };
        // the cells of a row within the current bound in x (the whole row while there is none)
        auto x_range = [&](uint32_t& il, uint32_t& ih) {
            const float e = eff();
            il = 0; ih = dx - 1;
            if (e == inf) return;
            const float rr = __fadd_rn(__fmul_rn(__fsqrt_rn(e), 1.0f + 1.0f / (1 << 20)), __fmul_rn(fabsf(me.x), 1.0f / (1 << 21)));
            const float lo = __fsub_rn(__fsub_rn(floorf(__fmul_rn(__fsub_rn(me.x, rr), inv_x)), fbx), 1.0f);
            const float hi = __fadd_rn(__fsub_rn(floorf(__fmul_rn(__fadd_rn(me.x, rr), inv_x)), fbx), 1.0f);
            if (lo > 0.0f) il = lo >= static_cast<float>(dx - 1) ? dx - 1 : static_cast<uint32_t>(lo);
            if (hi < static_cast<float>(dx - 1)) ih = hi < 0.0f ? 0u : static_cast<uint32_t>(hi);
        };
        bool done = false;
        if (first) {
            const uint32_t il = i ? i - 1 : 0u, ih = i + 1 < dx ? i + 1 : dx - 1;
            for_rows_3x3(j, kk, dy, dz, [&](uint32_t row) { scan_row(row, il, ih); });
            if (cnt == k) {
                // the nearest face of the 3x3x3 block, per axis (an axis the block covers whole has none)
                float g = inf;
                if (i >= 2 || i + 2 < dx) g = fminf(g, axis_gap(1.0f, cx, me.x));
                if (j >= 2 || j + 2 < dy) g = fminf(g, axis_gap(1.0f, cy, me.y));
                if (kk >= 2 || kk + 2 < dz) g = fminf(g, axis_gap(1.0f, cz, me.z));
                done = g == inf || my[(k - 1) * CM_BLOCK] <= __fmul_rn(__fmul_rn(g, g), kRel);
            }
            if (!done) {
                const unsigned int slot = atomicAdd(list_n, 1u);
                list[slot] = make_uint2(p, __float_as_uint(cnt == k ? my[(k - 1) * CM_BLOCK] : inf));
                continue;
            }
        } else {
            const uint32_t s_max = max(max(j, dy - 1 - j), max(kk, dz - 1 - kk));
            for (uint32_t s = 0; s <= s_max; ++s) {
                if (s >= 2 && cnt == k) {
                    // rows of ring s and beyond are (s - 1) cells away in y or z
                    const float sf = static_cast<float>(s - 1);
                    const float g = fminf(axis_gap(sf, cy, me.y), axis_gap(sf, cz, me.z));
                    if (my[(k - 1) * CM_BLOCK] <= __fmul_rn(__fmul_rn(g, g), kRel)) break;
                }
                for_row_ring(s, j, kk, dy, dz, [&](uint32_t row, int dj, int dk) {
                    // skip a row wholly beyond the bound: every point of it is (|dj|-1, |dk|-1) cells away at least
                    const float e = eff();
                    if (e != inf) {
                        const float gy = axis_gap(static_cast<float>(max(abs(dj) - 1, 0)), cy, me.y);
                        const float gz = axis_gap(static_cast<float>(max(abs(dk) - 1, 0)), cz, me.z);
                        if (e < __fmul_rn(__fadd_rn(__fmul_rn(gy, gy), __fmul_rn(gz, gz)), kRel)) return;
                    }
                    uint32_t il, ih;
                    x_range(il, ih);
                    scan_row(row, il, ih);
                });
            }
        }
        // d_i: the square roots, correctly rounded, added in ascending order in fp64 from 0, divided by k, rounded to fp32
        double sum = 0.0;
        for (uint32_t q = 0; q < k; ++q) sum = __dadd_rn(sum, static_cast<double>(sqrt_rn(my[q * CM_BLOCK])));
        dist[idx] = static_cast<float>(__ddiv_rn(sum, static_cast<double>(k)));
    }
}

// bins[0..255]: d_i, bins[256..511]: fp32(d_i * d_i). Slots outside the stage's input hold the sentinel 0xFFFFFFFF.
__global__ __launch_bounds__(CM_BLOCK) void k_sor_bins(const CmFrameState* __restrict__ st, const float* __restrict__ dist,
                                                       unsigned long long* __restrict__ bins, uint32_t n_padded) {
    __shared__ unsigned long long lb[2 * CM_SOR_BINS];
    for (uint32_t q = threadIdx.x; q < 2 * CM_SOR_BINS; q += CM_BLOCK) lb[q] = 0ull;
    __syncthreads();
    if (st->status != CM_DEV_OK) return;
    for (uint32_t t = blockIdx.x * CM_BLOCK + threadIdx.x; t < n_padded; t += gridDim.x * CM_BLOCK) {
        const float d = dist[t];
        if (__float_as_uint(d) == 0xFFFFFFFFu || d != d) continue;
        uint32_t e, m;
        cm_sor_split(d, &e, &m);
        atomicAdd(&lb[e], static_cast<unsigned long long>(m));
        cm_sor_split(__fmul_rn(d, d), &e, &m);
        atomicAdd(&lb[CM_SOR_BINS + e], static_cast<unsigned long long>(m));
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < 2 * CM_SOR_BINS; q += CM_BLOCK)
        if (lb[q]) atomicAdd(&bins[q], lb[q]);
}

__global__ void k_sor_threshold(const CmFrameState* __restrict__ st, const unsigned long long* __restrict__ bins,
                                CmSorStatsDev* __restrict__ out, uint32_t k, float std_mul) {
    if (threadIdx.x != 0) return;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const uint32_t n = st->status == CM_DEV_OK ? st->n_valid : 0u;
    CmSorStatsDev r;
    r.n_valid = n;
    r.n_removed = 0;
    r.mean = nan; r.stddev = nan; r.threshold = inf;
    if (n > k) {
        const double S = cm_sor_bins_to_double(bins), Q = cm_sor_bins_to_double(bins + CM_SOR_BINS);
        const double dn = static_cast<double>(n);
        const double mean = __ddiv_rn(S, dn);
        const double var = __ddiv_rn(__dsub_rn(Q, __ddiv_rn(__dmul_rn(S, S), dn)), __dsub_rn(dn, 1.0));
        const double sd = __dsqrt_rn(var);
        r.mean = mean;
        r.stddev = sd;
        r.threshold = __dadd_rn(mean, __dmul_rn(static_cast<double>(std_mul), sd));
    }
    *out = r;
}

__global__ __launch_bounds__(CM_BLOCK) void k_sor_mask(const CmFrameState* __restrict__ st, const float* __restrict__ dist,
                                                       CmSorStatsDev* __restrict__ stats, unsigned char* __restrict__ mask,
                                                       uint32_t n_padded) {
    __shared__ unsigned long long s_removed;
    if (threadIdx.x == 0) s_removed = 0ull;
    __syncthreads();
    if (st->status != CM_DEV_OK) return;
    const double thr = stats->threshold;
    unsigned long long removed = 0;
    for (uint32_t t = blockIdx.x * CM_BLOCK + threadIdx.x; t < n_padded; t += gridDim.x * CM_BLOCK) {
        const float d = dist[t];
        if (__float_as_uint(d) == 0xFFFFFFFFu) continue;
        if (static_cast<double>(d) > thr) ++removed;     // (false for a NaN threshold or d_i: kept, as in PCL)
        else mask[t] = 1;
    }
    if (removed) atomicAdd(&s_removed, removed);
    __syncthreads();
    if (threadIdx.x == 0 && s_removed) atomicAdd(&stats->n_removed, s_removed);
}

}  // namespace

// cm_launch.cpp sor_filter: words = CM_SOR_WORDS u64 (bins, list count, stats record), zeroed up to CM_SOR_WORD_STATS before
// the first launch; dist = n_padded floats set to 0xFFFFFFFF before it; list = n_padded uint2.
void cmk_sor_knn(hipStream_t s, const CmFrameDev* fd, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b,
                 const void* sorted_pts, const void* rows, float* dist, void* list, unsigned long long* words, uint32_t n_padded,
                 uint32_t k, bool first) {
    const float4* sp = reinterpret_cast<const float4*>(sorted_pts);
    const uint2* rw = reinterpret_cast<const uint2*>(rows);
    uint2* ls = reinterpret_cast<uint2*>(list);
    unsigned int* list_n = reinterpret_cast<unsigned int*>(words + CM_SOR_WORD_LIST);
    const uint32_t blocks = (n_padded + CM_BLOCK - 1) / CM_BLOCK;
    const int f = first ? 1 : 0;
    if (k <= 16) CM_LAUNCH(k_sor_knn<16>, blocks, CM_BLOCK, s, fd, st, keys_a, keys_b, sp, rw, dist, ls, list_n, k, f);
    else if (k <= 32) CM_LAUNCH(k_sor_knn<32>, blocks, CM_BLOCK, s, fd, st, keys_a, keys_b, sp, rw, dist, ls, list_n, k, f);
    else CM_LAUNCH(k_sor_knn<64>, blocks, CM_BLOCK, s, fd, st, keys_a, keys_b, sp, rw, dist, ls, list_n, k, f);
}
void cmk_sor_bins(hipStream_t s, const CmFrameState* st, const float* dist, unsigned long long* words, uint32_t n_padded) {
    CM_LAUNCH(k_sor_bins, (n_padded + CM_BLOCK * 16 - 1) / (CM_BLOCK * 16), CM_BLOCK, s, st, dist, words, n_padded);
}
void cmk_sor_threshold(hipStream_t s, const CmFrameState* st, unsigned long long* words, uint32_t k, float std_mul) {
    CM_LAUNCH(k_sor_threshold, 1, 64, s, st, words, reinterpret_cast<CmSorStatsDev*>(words + CM_SOR_WORD_STATS), k, std_mul);
}
void cmk_sor_mask(hipStream_t s, const CmFrameState* st, const float* dist, unsigned long long* words, unsigned char* mask,
                  uint32_t n_padded) {
    CM_LAUNCH(k_sor_mask, (n_padded + CM_BLOCK * 16 - 1) / (CM_BLOCK * 16), CM_BLOCK, s, st, dist,
              reinterpret_cast<CmSorStatsDev*>(words + CM_SOR_WORD_STATS), mask, n_padded);
}
