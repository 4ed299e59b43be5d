// cm_kernels_cov.hip — per-voxel covariance of the last frame's result (pcl::VoxelGridCovariance), for gfx950.
//
// A by-product computed on request after a frame (cm_result_voxel_cov), never part of one. It reads what the frame left —
// the kept points (cmk_merged, in (sensor, point) order), the result's sorted voxel keys and counts — and writes into
// buffers of its own only, so no later frame can see whether it ran.
//
//   k_cov_keys    one record per slot of the merged cloud: its cell key in the grid of out_key (the exact fp32 arithmetic of
//                 k_keys), found in out_key by binary search -> the record's voxel number, or CM_INVALID_KEY for a voxel
//                 the frame dropped (min_points_per_voxel); digit-0 counts per tile and per group of tiles, as k_keys
//                 leaves them for the radix sort                                    [16 B/rec read, 4 B/rec write]
//   radix sort    of (voxel number, record index) with the general path's k_hist / k_gscan / k_scatter, ballot-ranked
//                 (stable by construction), ceil(bits(n_out - 1) / 8) passes; pass 0 drops the invalid records
//   k_cov_reduce  one lane per voxel: finds the voxel's run by binary search, checks its length against out_cnt, adds the
//                 fp64 moments point after point in sorted (= merged) order, then the covariance, its eigen-decomposition
//                 (jacobi3), the inflation and the inverse                          [16 B/rec gather, 80 B/voxel write]
// Arithmetic: fp64, every operation rounded on its own (-ffp-contract=off and the _rn intrinsics: dadd, dsub, dmul, ddiv of
// cm_search.hpp), in the order of the header. The binary search is cm_search.hpp's lower_bound_u32.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

__global__ __launch_bounds__(CM_BLOCK) void k_cov_keys(const float4* __restrict__ recs, const uint32_t* __restrict__ total,
                                                       CmCovGridDev g, const uint32_t* __restrict__ out_key, uint32_t n_out,
                                                       uint32_t n_passes, CmFrameState* __restrict__ st,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                       uint32_t* __restrict__ grp) {
    __shared__ uint32_t lh[CM_RADIX];
    const uint32_t tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0) {
        // the sort's own state record: what k_hist / k_scatter read (status, passes); pass 0 writes n_valid
        st->status = CM_DEV_OK;
        st->n_passes = n_passes;
        st->n_valid = 0;
        st->err = 0;
    }
    const uint32_t n = *total;
    const uint32_t mul1 = g.div_b[0], mul2 = g.div_b[0] * g.div_b[1];
    const float fb0 = static_cast<float>(g.min_b[0]), fb1 = static_cast<float>(g.min_b[1]), fb2 = static_cast<float>(g.min_b[2]);
    lh[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        uint32_t v = CM_INVALID_KEY;
        if (i < n) {
            const float4 p = recs[i];
            const int c0 = static_cast<int>(__fsub_rn(floorf(__fmul_rn(p.x, g.inv[0])), fb0));
            const int c1 = static_cast<int>(__fsub_rn(floorf(__fmul_rn(p.y, g.inv[1])), fb1));
            const int c2 = static_cast<int>(__fsub_rn(floorf(__fmul_rn(p.z, g.inv[2])), fb2));
            const bool inside = static_cast<uint32_t>(c0) < g.div_b[0] && static_cast<uint32_t>(c1) < g.div_b[1] &&
                                static_cast<uint32_t>(c2) < g.div_b[2];
            const uint32_t key = static_cast<uint32_t>(c0) + static_cast<uint32_t>(c1) * mul1 + static_cast<uint32_t>(c2) * mul2;
            const uint32_t k = lower_bound_u32(out_key, 0u, n_out, key);
            if (inside && k < n_out && out_key[k] == key) {
                v = k;
                atomicAdd(&lh[v & (CM_RADIX - 1)], 1u);
            }
        }
        keys[i] = v;
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    hist[static_cast<size_t>(tile) * CM_RADIX + threadIdx.x] = c;
    if (c) atomicAdd(&grp[static_cast<size_t>(tile / CM_GROUP) * CM_RADIX + threadIdx.x], c);
}

__global__ __launch_bounds__(CM_BLOCK) void k_cov_reduce(const float4* __restrict__ recs, const CmFrameState* __restrict__ st_sort,
                                                         const uint32_t* __restrict__ keys_a, const uint32_t* __restrict__ vals_a,
                                                         const uint32_t* __restrict__ keys_b, const uint32_t* __restrict__ vals_b,
                                                         const uint32_t* __restrict__ out_cnt, uint32_t n_out, uint32_t min_points,
                                                         float eig_mult, CmVoxelCovDev* __restrict__ out, uint32_t* __restrict__ err) {
    const uint32_t v = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (v >= n_out) return;
    const bool odd = (st_sort->n_passes & 1u) != 0;       // pass p reads A when p is even and writes the other
    const uint32_t* __restrict__ keys = odd ? keys_b : keys_a;
    const uint32_t* __restrict__ vals = odd ? vals_b : vals_a;
    const uint32_t n_sorted = st_sort->n_valid;
    const uint32_t cnt = out_cnt[v];
    const uint32_t lo = lower_bound_u32(keys, 0u, n_sorted, v);
    const uint32_t hi = lo + cnt;
    // the run of voxel v must hold exactly the points the frame counted for it
    if (cnt == 0 || hi > n_sorted || hi < lo || keys[hi - 1] != v || (hi < n_sorted && keys[hi] == v)) {
        atomicOr(err, 1u);
        return;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    double S00 = 0.0, S10 = 0.0, S20 = 0.0, S11 = 0.0, S21 = 0.0, S22 = 0.0;
    for (uint32_t k = lo; k < hi; ++k) {
        const float4 p = recs[vals[k]];
        const double x = p.x, y = p.y, z = p.z;
        s0 = dadd(s0, x); s1 = dadd(s1, y); s2 = dadd(s2, z);
        S00 = dadd(S00, dmul(x, x)); S10 = dadd(S10, dmul(y, x)); S20 = dadd(S20, dmul(z, x));
        S11 = dadd(S11, dmul(y, y)); S21 = dadd(S21, dmul(z, y)); S22 = dadd(S22, dmul(z, z));
    }
    const double n = static_cast<double>(cnt);
    const double m0 = ddiv(s0, n), m1 = ddiv(s1, n), m2 = ddiv(s2, n);
    CmVoxelCovDev e;
    e.mean[0] = static_cast<float>(m0); e.mean[1] = static_cast<float>(m1); e.mean[2] = static_cast<float>(m2);
    e.count = cnt;
    for (int k = 0; k < 6; ++k) { e.cov[k] = 0.f; e.icov[k] = 0.f; }
    e.evals[0] = e.evals[1] = e.evals[2] = 0.f;
    e.flags = 0;
    if (cnt >= min_points) {
        // C_ij = ((S_ij - 2 (s_i m_j)) / n + m_i m_j) ((n - 1) / n), lower triangle (i >= j)
        const double f = ddiv(dsub(n, 1.0), n);
        const double s[3] = {s0, s1, s2}, m[3] = {m0, m1, m2};
        const double S[6] = {S00, S10, S20, S11, S21, S22};
        const int I[6] = {0, 1, 2, 1, 2, 2}, J[6] = {0, 0, 0, 1, 1, 2};
        double c[6];
#pragma unroll
        for (int q = 0; q < 6; ++q)
            c[q] = dmul(dadd(ddiv(dsub(S[q], dmul(2.0, dmul(s[I[q]], m[J[q]]))), n), dmul(m[I[q]], m[J[q]])), f);
        double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
        double V[3][3];
        jacobi3(A, V);
        // ascending eigenvalues, eigenvectors along
        int o[3] = {0, 1, 2};
        double l[3] = {A[0][0], A[1][1], A[2][2]};
        if (l[o[1]] < l[o[0]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
        if (l[o[2]] < l[o[1]]) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
        if (l[o[1]] < l[o[0]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
        double lam[3] = {l[o[0]], l[o[1]], l[o[2]]};
        double E[3][3];                                   // E[i][k]: component i of the k-th eigenvector
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) E[i][k] = V[i][o[k]];
        bool valid = lam[0] >= 0.0 && lam[1] >= 0.0 && lam[2] > 0.0;
        if (valid) {
            const double mu = dmul(static_cast<double>(eig_mult), lam[2]);
            if (lam[0] < mu) {
                lam[0] = mu;
                if (lam[1] < mu) lam[1] = mu;
                e.flags |= CM_COV_INFLATED_DEV;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const int i = I[q], j = J[q];
                    c[q] = dadd(dadd(dmul(dmul(E[i][0], lam[0]), E[j][0]), dmul(dmul(E[i][1], lam[1]), E[j][1])),
                                dmul(dmul(E[i][2], lam[2]), E[j][2]));
                }
            }
            // inverse by cofactors of the symmetric matrix (a b c / b d e / c e f)
            const double a = c[0], b = c[1], cc = c[2], d = c[3], ee = c[4], ff = c[5];
            const double A00 = dsub(dmul(d, ff), dmul(ee, ee)), A10 = dsub(dmul(cc, ee), dmul(b, ff)),
                         A20 = dsub(dmul(b, ee), dmul(cc, d)), A11 = dsub(dmul(a, ff), dmul(cc, cc)),
                         A21 = dsub(dmul(b, cc), dmul(a, ee)), A22 = dsub(dmul(a, d), dmul(b, b));
            const double det = dadd(dadd(dmul(a, A00), dmul(b, A10)), dmul(cc, A20));
            const double inv[6] = {ddiv(A00, det), ddiv(A10, det), ddiv(A20, det), ddiv(A11, det), ddiv(A21, det), ddiv(A22, det)};
#pragma unroll
            for (int q = 0; q < 6; ++q) valid = valid && isfinite(inv[q]);
            if (valid) {
#pragma unroll
                for (int q = 0; q < 6; ++q) e.icov[q] = static_cast<float>(inv[q]);
#pragma unroll
                for (int k = 0; k < 3; ++k) e.evals[k] = static_cast<float>(lam[k]);
                e.flags |= CM_COV_VALID_DEV;
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) e.cov[q] = static_cast<float>(c[q]);
    }
    out[v] = e;
}

}  // namespace

void cmk_cov_keys(hipStream_t s, const void* recs, const uint32_t* total, const CmCovGridDev& g, const uint32_t* out_key,
                  uint32_t n_out, uint32_t n_passes, CmFrameState* st, uint32_t* keys, uint32_t* hist, uint32_t* grp,
                  uint32_t n_tiles) {
    hipLaunchKernelGGL(k_cov_keys, dim3(n_tiles), dim3(CM_BLOCK), 0, s, reinterpret_cast<const float4*>(recs), total, g, out_key,
                       n_out, n_passes, st, keys, hist, grp);
}
void cmk_cov_reduce(hipStream_t s, const void* recs, const CmFrameState* st_sort, const uint32_t* keys_a, const uint32_t* vals_a,
                    const uint32_t* keys_b, const uint32_t* vals_b, const uint32_t* out_cnt, uint32_t n_out, uint32_t min_points,
                    float eig_mult, void* out, uint32_t* err) {
    if (n_out == 0) return;
    hipLaunchKernelGGL(k_cov_reduce, dim3((n_out + CM_BLOCK - 1) / CM_BLOCK), dim3(CM_BLOCK), 0, s,
                       reinterpret_cast<const float4*>(recs), st_sort, keys_a, vals_a, keys_b, vals_b, out_cnt, n_out, min_points,
                       eig_mult, reinterpret_cast<CmVoxelCovDev*>(out), err);
}
