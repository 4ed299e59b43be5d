// cm_kernels_ndt.hip — NDT registration of a source cloud against the last frame's per-voxel covariance table, for gfx950
// (cm_result_ndt_align).
//
// A by-product computed on request after a frame, never part of one. It reads the result's sorted voxel keys (out_key) and
// the covariance table (cm_kernels_cov.hip) and writes buffers of its own only. One evaluation of a pose is two launches:
//
//   k_ndt_eval   one lane per source point, one workgroup per aligned block of 256 source indices.
//                Transform: k_aln_eval's, q64 in fp64 and qf = float(q64). Voxels: qf's cell in the grid of out_key with
//                k_cov_keys' fp32 arithmetic, then the cell and (neighbourhood 7) its six face neighbours, each tested per
//                axis as integers against the grid and looked up in out_key by binary search (lower_bound_u32,
//                cm_search.hpp: k_cov_keys' search) — no search grid of its own.
//                Terms: per used voxel the Mahalanobis form m, the weight w = cm_exp_neg(d2h * m) (cm_ndt_math.hpp) and the
//                28 products, added over the point's voxels in candidate order into 28 registers; the voxel loop stays
//                rolled. The 16-byte correspondence goes out in one store. Reduction: k_aln_eval's — shuffles inside a
//                wave, the four wave sums through LDS as ((w0 + w1) + w2) + w3, one vector store of the block's 28 sums and
//                its count, CM_ALIGN_STRIDE doubles per block.
//   k_aln_sum    (cm_kernels_align.hip) the block partials added in ascending block order.
//
// No floating-point atomics anywhere: the sums depend on the inputs alone, not on the launch or on timing.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

// the rounded fp64 operations: cm_ndt_math.hpp's macros, the one spelling of this file too
#define CM_NDT_FN __device__ __forceinline__
#define CM_NDT_MUL(a, b) __dmul_rn((a), (b))
#define CM_NDT_ADD(a, b) __dadd_rn((a), (b))
#define CM_NDT_SUB(a, b) __dsub_rn((a), (b))
#include "cm_ndt_math.hpp"

namespace {

// (x0 y0 + x1 y1) + x2 y2, every operation rounded on its own
__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
    return CM_NDT_ADD(CM_NDT_ADD(CM_NDT_MUL(x0, y0), CM_NDT_MUL(x1, y1)), CM_NDT_MUL(x2, y2));
}
// x0 y0 + x1 y1: the three-term form with an exact zero left out
__device__ __forceinline__ double dot2(double x0, double x1, double y0, double y1) {
    return CM_NDT_ADD(CM_NDT_MUL(x0, y0), CM_NDT_MUL(x1, y1));
}

__global__ __launch_bounds__(CM_BLOCK) void k_ndt_eval(const uint32_t* __restrict__ out_key, uint32_t n_out,
                                                       const CmVoxelCovDev* __restrict__ cov, const float4* __restrict__ src,
                                                       uint32_t n_src, CmCovGridDev g, uint32_t n_cand, double d2h,
                                                       CmAlignPoseDev P, uint4* __restrict__ corr,
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
        q0 = CM_NDT_ADD(CM_NDT_ADD(CM_NDT_ADD(CM_NDT_MUL(P.m[0], x), CM_NDT_MUL(P.m[1], y)), CM_NDT_MUL(P.m[2], z)), P.m[3]);
        q1 = CM_NDT_ADD(CM_NDT_ADD(CM_NDT_ADD(CM_NDT_MUL(P.m[4], x), CM_NDT_MUL(P.m[5], y)), CM_NDT_MUL(P.m[6], z)), P.m[7]);
        q2 = CM_NDT_ADD(CM_NDT_ADD(CM_NDT_ADD(CM_NDT_MUL(P.m[8], x), CM_NDT_MUL(P.m[9], y)), CM_NDT_MUL(P.m[10], z)), P.m[11]);
        f0 = static_cast<float>(q0); f1 = static_cast<float>(q1); f2 = static_cast<float>(q2);
    }

    // 2. the point's cell, tested in float before any cast: within one cell of the grid on every axis, or no voxel at all
    const float v0 = __fsub_rn(floorf(__fmul_rn(f0, g.inv[0])), static_cast<float>(g.min_b[0]));
    const float v1 = __fsub_rn(floorf(__fmul_rn(f1, g.inv[1])), static_cast<float>(g.min_b[1]));
    const float v2 = __fsub_rn(floorf(__fmul_rn(f2, g.inv[2])), static_cast<float>(g.min_b[2]));
    const bool near_grid = has && isfinite(f0) && isfinite(f1) && isfinite(f2) &&
                           v0 >= -1.0f && v0 <= static_cast<float>(g.div_b[0]) && v1 >= -1.0f && v1 <= static_cast<float>(g.div_b[1]) &&
                           v2 >= -1.0f && v2 <= static_cast<float>(g.div_b[2]);

    // 3. terms over the used voxels, in candidate order from +0.0
    double v[CM_ALIGN_TERMS];
#pragma unroll
    for (int t = 0; t < CM_ALIGN_TERMS; ++t) v[t] = 0.0;
    uint32_t idx = CM_NDT_NONE_DEV, n_used = 0;
    if (near_grid) {
        const long long c0 = static_cast<long long>(v0), c1 = static_cast<long long>(v1), c2 = static_cast<long long>(v2);
        const double a0 = CM_NDT_SUB(q0, P.p0[0]), a1 = CM_NDT_SUB(q1, P.p0[1]), a2 = CM_NDT_SUB(q2, P.p0[2]);
#pragma unroll 1
        for (uint32_t j = 0; j < n_cand; ++j) {
            // c, c - e0, c + e0, c - e1, c + e1, c - e2, c + e2
            const long long step = j == 0u ? 0 : ((j & 1u) ? -1 : 1);
            const uint32_t axis = (j + 1u) >> 1;           // 0: none, 1..3: x, y, z
            const long long e0 = c0 + (axis == 1u ? step : 0), e1 = c1 + (axis == 2u ? step : 0), e2 = c2 + (axis == 3u ? step : 0);
            if (e0 < 0 || e0 >= static_cast<long long>(g.div_b[0]) || e1 < 0 || e1 >= static_cast<long long>(g.div_b[1]) ||
                e2 < 0 || e2 >= static_cast<long long>(g.div_b[2]))
                continue;
            const uint32_t key = static_cast<uint32_t>(e0) + static_cast<uint32_t>(e1) * g.div_b[0] +
                                 static_cast<uint32_t>(e2) * (g.div_b[0] * g.div_b[1]);
            const uint32_t k = lower_bound_u32(out_key, 0u, n_out, key);
            if (k >= n_out || out_key[k] != key) continue;
            const CmVoxelCovDev* __restrict__ e = cov + k;
            if (!(e->flags & CM_COV_VALID_DEV)) continue;
            const double r0 = CM_NDT_SUB(a0, CM_NDT_SUB(static_cast<double>(e->mean[0]), P.p0[0]));
            const double r1 = CM_NDT_SUB(a1, CM_NDT_SUB(static_cast<double>(e->mean[1]), P.p0[1]));
            const double r2 = CM_NDT_SUB(a2, CM_NDT_SUB(static_cast<double>(e->mean[2]), P.p0[2]));
            const double B00 = e->icov[0], B10 = e->icov[1], B20 = e->icov[2], B11 = e->icov[3], B21 = e->icov[4], B22 = e->icov[5];
            const double u0 = dot3(B00, B10, B20, r0, r1, r2);
            const double u1 = dot3(B10, B11, B21, r0, r1, r2);
            const double u2 = dot3(B20, B21, B22, r0, r1, r2);
            const double m = dot3(r0, r1, r2, u0, u1, u2);
            if (!(isfinite(m) && m >= 0.0)) continue;
            ++n_used;
            if (j == 0u) idx = k;
            const double w = cm_exp_neg(CM_NDT_MUL(d2h, m));
            // the twist's Jacobian columns about the pivot: c_0 = (0, -a2, a1), c_1 = (a2, 0, -a0), c_2 = (-a1, a0, 0),
            // c_3..5 = e_0..2; y_v = B c_v with the exact zeros left out, so y_3..5 are B's columns
            const double na0 = -a0, na1 = -a1, na2 = -a2;
            const double y00 = dot2(B10, B20, na2, a1), y01 = dot2(B11, B21, na2, a1), y02 = dot2(B21, B22, na2, a1);
            const double y10 = dot2(B00, B20, a2, na0), y11 = dot2(B10, B21, a2, na0), y12 = dot2(B20, B22, a2, na0);
            const double y20 = dot2(B00, B10, na1, a0), y21 = dot2(B10, B11, na1, a0), y22 = dot2(B20, B21, na1, a0);
            // H, the lower triangle row by row: c_u . y_v
            v[0] = CM_NDT_ADD(v[0], CM_NDT_MUL(w, dot2(na2, a1, y01, y02)));
            v[1] = CM_NDT_ADD(v[1], CM_NDT_MUL(w, dot2(a2, na0, y00, y02)));
            v[2] = CM_NDT_ADD(v[2], CM_NDT_MUL(w, dot2(a2, na0, y10, y12)));
            v[3] = CM_NDT_ADD(v[3], CM_NDT_MUL(w, dot2(na1, a0, y00, y01)));
            v[4] = CM_NDT_ADD(v[4], CM_NDT_MUL(w, dot2(na1, a0, y10, y11)));
            v[5] = CM_NDT_ADD(v[5], CM_NDT_MUL(w, dot2(na1, a0, y20, y21)));
            v[6] = CM_NDT_ADD(v[6], CM_NDT_MUL(w, y00));
            v[7] = CM_NDT_ADD(v[7], CM_NDT_MUL(w, y10));
            v[8] = CM_NDT_ADD(v[8], CM_NDT_MUL(w, y20));
            v[9] = CM_NDT_ADD(v[9], CM_NDT_MUL(w, B00));
            v[10] = CM_NDT_ADD(v[10], CM_NDT_MUL(w, y01));
            v[11] = CM_NDT_ADD(v[11], CM_NDT_MUL(w, y11));
            v[12] = CM_NDT_ADD(v[12], CM_NDT_MUL(w, y21));
            v[13] = CM_NDT_ADD(v[13], CM_NDT_MUL(w, B10));
            v[14] = CM_NDT_ADD(v[14], CM_NDT_MUL(w, B11));
            v[15] = CM_NDT_ADD(v[15], CM_NDT_MUL(w, y02));
            v[16] = CM_NDT_ADD(v[16], CM_NDT_MUL(w, y12));
            v[17] = CM_NDT_ADD(v[17], CM_NDT_MUL(w, y22));
            v[18] = CM_NDT_ADD(v[18], CM_NDT_MUL(w, B20));
            v[19] = CM_NDT_ADD(v[19], CM_NDT_MUL(w, B21));
            v[20] = CM_NDT_ADD(v[20], CM_NDT_MUL(w, B22));
            // g: c_u . u
            v[21] = CM_NDT_ADD(v[21], CM_NDT_MUL(w, dot2(na2, a1, u1, u2)));
            v[22] = CM_NDT_ADD(v[22], CM_NDT_MUL(w, dot2(a2, na0, u0, u2)));
            v[23] = CM_NDT_ADD(v[23], CM_NDT_MUL(w, dot2(na1, a0, u0, u1)));
            v[24] = CM_NDT_ADD(v[24], CM_NDT_MUL(w, u0));
            v[25] = CM_NDT_ADD(v[25], CM_NDT_MUL(w, u1));
            v[26] = CM_NDT_ADD(v[26], CM_NDT_MUL(w, u2));
            v[27] = CM_NDT_ADD(v[27], w);
        }
    }
    if (has) {
        const unsigned long long sb = static_cast<unsigned long long>(__double_as_longlong(v[27]));
        corr[i] = make_uint4(idx, n_used, static_cast<uint32_t>(sb), static_cast<uint32_t>(sb >> 32));
    }

    // 4. the wave's sums in lane 0, the block's in lanes 0..28 of wave 0 (k_aln_eval's reduction and layout)
    const uint32_t cnt = static_cast<uint32_t>(__popcll(__ballot(n_used != 0u)));
#pragma unroll
    for (int t = 0; t < CM_ALIGN_TERMS; ++t) {
        double a = v[t];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) a = CM_NDT_ADD(a, __shfl_down(a, s));
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
            s = CM_NDT_ADD(CM_NDT_ADD(CM_NDT_ADD(wsum[0][t], wsum[1][t]), wsum[2][t]), wsum[3][t]);
        } else {
            s = __longlong_as_double(__double_as_longlong(wsum[0][t]) + __double_as_longlong(wsum[1][t]) +
                                     __double_as_longlong(wsum[2][t]) + __double_as_longlong(wsum[3][t]));
        }
        partials[static_cast<size_t>(blockIdx.x) * CM_ALIGN_STRIDE + t] = s;
    }
}

}  // namespace

// cm_byproducts.cpp ndt. corr: n_src entries of 16 bytes; partials: ceil(n_src / 256) * CM_ALIGN_STRIDE doubles, summed by
// cmk_aln_sum. n_src 0: no launch. n_out 0: nothing is looked up, and out_key and cov are not read.
void cmk_ndt_eval(hipStream_t s, const uint32_t* out_key, uint32_t n_out, const void* cov, const void* src, uint32_t n_src,
                  const CmCovGridDev& g, uint32_t neighborhood, double d2h, const CmAlignPoseDev& pose, void* corr,
                  double* partials) {
    if (n_src == 0) return;
    hipLaunchKernelGGL(k_ndt_eval, dim3((n_src + CM_BLOCK - 1) / CM_BLOCK), dim3(CM_BLOCK), 0, s, out_key, n_out,
                       reinterpret_cast<const CmVoxelCovDev*>(cov), reinterpret_cast<const float4*>(src), n_src, g, neighborhood,
                       d2h, pose, reinterpret_cast<uint4*>(corr), partials);
}
