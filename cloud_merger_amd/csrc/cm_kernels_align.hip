// cm_kernels_align.hip — point-to-plane ICP registration of a source cloud against the last frame's result, for gfx950
// (cm_result_align).
//
// A by-product computed on request after a frame, never part of one. The result's centroids are sorted by a search grid of
// their own with the cluster call's front end (k_cl_bounds, k_cl_keys, the radix passes, k_cl_gather, the (y,z)-row table),
// once per call: pts holds them in cell order (x, y, z, result index), the sorted keys lie beside them; the cell is at least
// 1.0039 r (cluster_grid, cm_route.cpp). One evaluation of a pose is two launches:
//
//   k_aln_eval   one lane per source point, one workgroup per aligned block of 256 source indices.
//                Transform: q64 = ((r00 x + r01 y) + r02 z) + t0 ... in fp64, qf = float(q64). Match: the 9 rows x 3 cells
//                around qf's cell (grid_cell, for_row_cells, d2_of: cm_search.hpp, the cell, the search and
//                the distance of k_cl_hook), the smallest (d2, result index) pair with d2 < r2 kept; its 8-byte correspondence is written at the source index. Terms: the matched
//                centroid and its normal gathered by result index, the 28 fp64 products about the pivot. Reduction: inside
//                a wave v[l] += v[l + s] for s = 32 .. 1 by shuffles, the four wave sums through LDS as ((w0 + w1) + w2) + w3,
//                and one vector store of the block's 28 sums and its count (29 lanes, 8 bytes each).
//   k_aln_sum    one lane per sum: the block partials added one after the other in ascending block order from 0.0.
//
// No floating-point atomics anywhere: the sums depend on the inputs alone, not on the launch or on timing.
//
// Why the 27 cells are enough, also for a point outside the grid. The cell of a coordinate (grid_cell) is
// clamp(floor(fl(fl(x - min) * inv)), 0, dims - 1): every step is monotone in x, so the whole is. A centroid c with
// d2(qf, c) < r2 is within r (1 + 2^-22) of qf along every axis, and two coordinates that close are never two cells apart
// (cell >= 1.0039 r; tests/test_cluster.py checks that premise in this arithmetic) — before the clamp, and the clamp, being
// monotone and 1-Lipschitz on integers, can only bring the two cells closer. So a point beyond the bounds lands in a border
// cell, the cells around it hold every centroid it could match, and the predicate alone decides: a point farther out than r
// matches nothing. This is the argument of the cluster stage, whose points all lie inside the grid.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

__global__ __launch_bounds__(CM_BLOCK) void k_aln_eval(const CmFrameState* __restrict__ st, const uint32_t* __restrict__ keys_a,
                                                       const uint32_t* __restrict__ keys_b, const float4* __restrict__ pts,
                                                       const uint2* __restrict__ rows, const float4* __restrict__ recs,
                                                       const uint4* __restrict__ normals, const float4* __restrict__ src,
                                                       uint32_t n_src, uint32_t n_tgt, CmClusterGridDev g, float r2,
                                                       CmAlignPoseDev P, uint2* __restrict__ corr,
                                                       double* __restrict__ partials) {
    __shared__ double wsum[CM_WAVES][CM_ALIGN_SUMS];
    const uint32_t i = blockIdx.x * CM_BLOCK + threadIdx.x;
    const bool has = i < n_src;

    // 1. transform
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
    if (has) {
        const float4 s = src[i];
        const double x = s.x, y = s.y, z = s.z;
        q0 = dadd(dadd(dadd(dmul(P.m[0], x), dmul(P.m[1], y)), dmul(P.m[2], z)), P.m[3]);
        q1 = dadd(dadd(dadd(dmul(P.m[4], x), dmul(P.m[5], y)), dmul(P.m[6], z)), P.m[7]);
        q2 = dadd(dadd(dadd(dmul(P.m[8], x), dmul(P.m[9], y)), dmul(P.m[10], z)), P.m[11]);
        f0 = static_cast<float>(q0); f1 = static_cast<float>(q1); f2 = static_cast<float>(q2);
    }

    // 2. match: the smallest (d2, result index) among the centroids with d2 < r2
    uint32_t best_j = CM_ALIGN_NONE_DEV;
    float best_d = 0.0f;
    if (has && n_tgt != 0u && isfinite(f0) && isfinite(f1) && isfinite(f2) && st->status == CM_DEV_OK) {
        const uint32_t* __restrict__ keys = pick(st, keys_a, keys_b);
        const uint32_t dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
        const uint32_t cx = grid_cell(f0, g.min[0], g.inv, dx), cy = grid_cell(f1, g.min[1], g.inv, dy),
                       cz = grid_cell(f2, g.min[2], g.inv, dz);
        const uint32_t x_lo = cx ? cx - 1u : 0u, x_hi = (cx + 1u < dx) ? cx + 1u : dx - 1u;
        const float4 qf = make_float4(f0, f1, f2, 0.0f);
        // (the 3 x 3 rows in for_rows_3x3's order, in this kernel's own rolled loop: through the template the kernel measured
        // 1 % slower per iteration at a 50 cm leaf, profiles/device_helpers_cost.txt)
#pragma unroll 1
        for (int q = 0; q < 9; ++q) {
            const int oz = q / 3 - 1, oy = q % 3 - 1;
            if ((oz < 0 && cz == 0u) || (oz > 0 && cz + 1u >= dz) || (oy < 0 && cy == 0u) || (oy > 0 && cy + 1u >= dy)) continue;
            const uint32_t r = (cy + static_cast<uint32_t>(oy)) + dy * (cz + static_cast<uint32_t>(oz));
            const uint2 rg = rows[r];
            for_row_cells(keys, rg.x, rg.y, r, dx, x_lo, x_hi, [&](uint32_t t) {
                const float4 p = pts[t];
                const float d2 = d2_of(qf, p);
                const uint32_t j = __float_as_uint(p.w);
                if (d2 < r2 && (best_j == CM_ALIGN_NONE_DEV || d2 < best_d || (d2 == best_d && j < best_j))) {
                    best_d = d2;
                    best_j = j;
                }
            });
        }
    }
    if (has) corr[i] = make_uint2(best_j, __float_as_uint(best_d));

    // 3. terms: +0.0 for a lane without a match or without a valid normal
    double v[CM_ALIGN_TERMS];
#pragma unroll
    for (int t = 0; t < CM_ALIGN_TERMS; ++t) v[t] = 0.0;
    bool counted = false;
    if (best_j != CM_ALIGN_NONE_DEV) {
        const uint4 n4 = normals[2 * static_cast<size_t>(best_j)];
        const uint4 m4 = normals[2 * static_cast<size_t>(best_j) + 1];
        if (m4.w & CM_NORMAL_VALID_DEV) {
            counted = true;
            const float4 c = recs[best_j];
            const double a0 = dsub(q0, P.p0[0]), a1 = dsub(q1, P.p0[1]), a2 = dsub(q2, P.p0[2]);
            const double b0 = dsub(static_cast<double>(c.x), P.p0[0]), b1 = dsub(static_cast<double>(c.y), P.p0[1]),
                         b2 = dsub(static_cast<double>(c.z), P.p0[2]);
            const double n0 = __uint_as_float(n4.x), n1 = __uint_as_float(n4.y), n2 = __uint_as_float(n4.z);
            const double res = dadd(dadd(dmul(n0, dsub(a0, b0)), dmul(n1, dsub(a1, b1))), dmul(n2, dsub(a2, b2)));
            const double J[6] = {dsub(dmul(a1, n2), dmul(a2, n1)), dsub(dmul(a2, n0), dmul(a0, n2)),
                                 dsub(dmul(a0, n1), dmul(a1, n0)), n0, n1, n2};
            int t = 0;
#pragma unroll
            for (int u = 0; u < 6; ++u)
#pragma unroll
                for (int w = 0; w <= u; ++w) v[t++] = dmul(J[u], J[w]);
#pragma unroll
            for (int u = 0; u < 6; ++u) v[21 + u] = dmul(J[u], res);
            v[27] = dmul(res, res);
        }
    }

    // 4. the wave's sums in lane 0, the block's in lanes 0..28 of wave 0
    const uint32_t cnt = static_cast<uint32_t>(__popcll(__ballot(counted)));
#pragma unroll
    for (int t = 0; t < CM_ALIGN_TERMS; ++t) {
        double a = v[t];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) a = dadd(a, __shfl_down(a, s));
        v[t] = a;
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int t = 0; t < CM_ALIGN_TERMS; ++t) wsum[wave][t] = v[t];
        wsum[wave][CM_ALIGN_TERMS] = __longlong_as_double(static_cast<long long>(cnt));
    }
    __syncthreads();
    if (threadIdx.x < CM_ALIGN_SUMS) {
        const uint32_t t = threadIdx.x;
        double s;
        if (t < CM_ALIGN_TERMS) {
            s = dadd(dadd(dadd(wsum[0][t], wsum[1][t]), wsum[2][t]), wsum[3][t]);
        } else {
            s = __longlong_as_double(__double_as_longlong(wsum[0][t]) + __double_as_longlong(wsum[1][t]) +
                                     __double_as_longlong(wsum[2][t]) + __double_as_longlong(wsum[3][t]));
        }
        partials[static_cast<size_t>(blockIdx.x) * CM_ALIGN_STRIDE + t] = s;
    }
}

// sums[0..27]: the 28 sums; sums[28]: the count (an integer in the 8 bytes).
__global__ __launch_bounds__(64) void k_aln_sum(const double* __restrict__ partials, uint32_t n_blocks, double* __restrict__ sums) {
    const uint32_t t = threadIdx.x;
    if (t >= CM_ALIGN_SUMS) return;
    if (t < CM_ALIGN_TERMS) {
        double acc = 0.0;
        for (uint32_t b = 0; b < n_blocks; ++b) acc = dadd(acc, partials[static_cast<size_t>(b) * CM_ALIGN_STRIDE + t]);
        sums[t] = acc;
    } else {
        long long acc = 0;
        for (uint32_t b = 0; b < n_blocks; ++b) acc += __double_as_longlong(partials[static_cast<size_t>(b) * CM_ALIGN_STRIDE + t]);
        sums[t] = __longlong_as_double(acc);
    }
}

}  // namespace

// cm_byproducts.cpp align. corr: n_src entries of 8 bytes; partials: ceil(n_src / 256) * CM_ALIGN_STRIDE doubles; sums:
// CM_ALIGN_SUMS doubles. n_src 0: no launch of k_aln_eval, and the sums are those of no block (zeros).
void cmk_aln_eval(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                  const void* rows, const void* recs, const void* normals, const void* src, uint32_t n_src, uint32_t n_tgt,
                  const CmClusterGridDev& g, float r2, const CmAlignPoseDev& pose, void* corr, double* partials) {
    if (n_src == 0) return;
    CM_LAUNCH(k_aln_eval, (n_src + CM_BLOCK - 1) / CM_BLOCK, CM_BLOCK, s, st, keys_a, keys_b, reinterpret_cast<const float4*>(pts),
              reinterpret_cast<const uint2*>(rows), reinterpret_cast<const float4*>(recs), reinterpret_cast<const uint4*>(normals),
              reinterpret_cast<const float4*>(src), n_src, n_tgt, g, r2, pose, reinterpret_cast<uint2*>(corr), partials);
}

void cmk_aln_sum(hipStream_t s, const double* partials, uint32_t n_blocks, double* sums) {
    CM_LAUNCH(k_aln_sum, 1, 64, s, partials, n_blocks, sums);
}
