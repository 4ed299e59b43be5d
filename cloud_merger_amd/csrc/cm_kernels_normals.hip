// cm_kernels_normals.hip — surface normals and curvature of the last frame's result (pcl::NormalEstimation, k-nearest
// neighbours), for gfx950.
//
// A by-product computed on request after a frame (cm_result_normals), never part of one. The centroids are sorted by a search
// grid of their own with the cluster call's front end (k_cl_bounds, k_cl_keys, the radix passes, k_cl_gather, the (y,z)-row
// table): pts holds them in cell order (x, y, z, result index), the sorted keys lie beside them.
//
//   k_nrm_knn<KMAX, LANES>(first)  exact k nearest neighbours, one lane per centroid, the k - 1 smallest (d2, result index)
//                           pairs of the OTHER centroids kept ascending in LDS (KMAX pairs per lane, lane-interleaved: 8 B per
//                           slot). First launch: the 3x3x3 cells around the centroid; it is finished when its last pair's d2 is
//                           strictly below the distance to the nearest face of that block. The others go onto a list with that
//                           d2 as a bound. Second launch (only when the list is not empty): the listed centroids search row
//                           ring by row ring, as k_sor_knn does. A finished centroid goes straight on to its plane:
//   nrm_plane               the neighbours in list order: fp64 offsets about the centroid, their sums and products added one
//                           after the other, the covariance, jacobi3, the eigenvector of the smallest eigenvalue turned
//                           towards the viewpoint, and the 32-byte entry in two 16-byte stores.
//
// Ties. The neighbourhood is defined by the lexicographic order of (d2, result index), so that the table is a function of the
// result alone whatever the search grid and the launch geometry. Hence (a) a candidate replaces the last pair iff its pair
// is lexicographically smaller, and (b) every bound that ends or prunes the search rejects only candidates whose d2 is
// STRICTLY larger than the current last d2: a candidate at exactly that distance may still win by its index. Every such
// bound below is "last d2 < lower bound on the d2 of what is skipped".
//
// The geometry of the grid (cm_device.h CmClusterGridDev): cell = floor(fl(fl(p - min) * inv)), at most 4096 cells per axis
// (normals_grid, cm_route.cpp). The two roundings move a centroid by less than 4096 * 2^-23 = 2^-11 of a cell, so two centroids
// whose cell indices differ by D >= 2 along an axis are more than (D - 1 - 2^-10) cells apart along it; cell_gap takes
// (D - 1 - 2^-8), and kRel (cm_search.hpp) covers the rounding of 1 / inv, of the products and of the fp32 d2 itself.
//
// d2_of, kRel and the fp64 operations (dadd ...) are cm_search.hpp's. The walk is NOT: scan_row, the 3 x 3 rows and the ring
// loop below are this kernel's own copy of for_row_cells / for_rows_3x3 / for_row_ring, line for line in the visiting order.
// Through the shared templates the kernel compiled to two to four instructions more (the same registers, LDS and occupancy) and
// measured 2 - 4 % slower at a 50 cm leaf, k = 30, in two sessions (profiles/device_helpers_cost.txt), so its text stays
// byte for byte what it was. A change to the walk in cm_search.hpp is a change here too.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

// A lower bound (m) on the distance along one axis between two centroids whose cell indices differ by D or more.
__device__ __forceinline__ float cell_gap(int D, float cell) {
    return D >= 2 ? __fmul_rn(__fmul_rn(static_cast<float>(D - 1) - 1.0f / 256.0f, cell), kRel) : 0.0f;
}

__device__ __forceinline__ bool pair_less(float d2a, uint32_t ja, float d2b, uint32_t jb) {
    return d2a < d2b || (d2a == d2b && ja < jb);
}

// The entry of centroid `me` (result index me.w) from its kk nearest others, lj[q * LANES] in ascending (d2, index) order.
template <int LANES>
__device__ __forceinline__ void nrm_plane(const float4* __restrict__ recs, const float4& me, const float* ld, const uint32_t* lj,
                                          uint32_t kk, float vx, float vy, float vz, uint4* __restrict__ out) {
    const uint32_t idx = __float_as_uint(me.w);
    const uint32_t m = kk + 1u;
    const double cx = me.x, cy = me.y, cz = me.z;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    double S00 = 0.0, S10 = 0.0, S20 = 0.0, S11 = 0.0, S21 = 0.0, S22 = 0.0;
    for (uint32_t q = 0; q < kk; ++q) {
        const float4 p = recs[lj[q * LANES]];
        const double x = dsub(static_cast<double>(p.x), cx), y = dsub(static_cast<double>(p.y), cy),
                     z = dsub(static_cast<double>(p.z), cz);
        s0 = dadd(s0, x); s1 = dadd(s1, y); s2 = dadd(s2, z);
        S00 = dadd(S00, dmul(x, x)); S10 = dadd(S10, dmul(y, x)); S20 = dadd(S20, dmul(z, x));
        S11 = dadd(S11, dmul(y, y)); S21 = dadd(S21, dmul(z, y)); S22 = dadd(S22, dmul(z, z));
    }
    const float nanf_ = __uint_as_float(0x7FC00000u);
    float nx = nanf_, ny = nanf_, nz = nanf_, curv = nanf_;
    uint32_t flags = 0;
    if (m >= 3u) {
        const double dm = static_cast<double>(m);
        const double m0 = ddiv(s0, dm), m1 = ddiv(s1, dm), m2 = ddiv(s2, dm);
        const double c00 = dsub(ddiv(S00, dm), dmul(m0, m0)), c10 = dsub(ddiv(S10, dm), dmul(m1, m0)),
                     c20 = dsub(ddiv(S20, dm), dmul(m2, m0)), c11 = dsub(ddiv(S11, dm), dmul(m1, m1)),
                     c21 = dsub(ddiv(S21, dm), dmul(m2, m1)), c22 = dsub(ddiv(S22, dm), dmul(m2, m2));
        double A[3][3] = {{c00, c10, c20}, {c10, c11, c21}, {c20, c21, c22}};
        double V[3][3];
        jacobi3(A, V);
        // the smallest eigenvalue and its eigenvector (selects, no indexed registers) and the largest
        const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
        const bool z1 = l1 < l0;
        double lo = z1 ? l1 : l0;
        double e0 = z1 ? V[0][1] : V[0][0], e1 = z1 ? V[1][1] : V[1][0], e2 = z1 ? V[2][1] : V[2][0];
        const bool z2 = l2 < lo;
        lo = z2 ? l2 : lo;
        e0 = z2 ? V[0][2] : e0; e1 = z2 ? V[1][2] : e1; e2 = z2 ? V[2][2] : e2;
        const double hi = fmax(fmax(l0, l1), l2);
        const double len = __dsqrt_rn(dadd(dadd(dmul(e0, e0), dmul(e1, e1)), dmul(e2, e2)));
        e0 = ddiv(e0, len); e1 = ddiv(e1, len); e2 = ddiv(e2, len);
        const double cv = fabs(ddiv(lo, dadd(dadd(l0, l1), l2)));
        const double wx = dsub(static_cast<double>(vx), cx), wy = dsub(static_cast<double>(vy), cy),
                     wz = dsub(static_cast<double>(vz), cz);
        if (dadd(dadd(dmul(e0, wx), dmul(e1, wy)), dmul(e2, wz)) < 0.0) { e0 = -e0; e1 = -e1; e2 = -e2; }
        if (hi > 0.0 && isfinite(hi) && isfinite(lo) && isfinite(e0) && isfinite(e1) && isfinite(e2) && isfinite(cv)) {
            nx = static_cast<float>(e0); ny = static_cast<float>(e1); nz = static_cast<float>(e2);
            curv = static_cast<float>(cv);
            flags = CM_NORMAL_VALID_DEV;
        }
    }
    const float r2 = kk ? ld[(kk - 1u) * LANES] : 0.0f;
    const uint32_t last = kk ? lj[(kk - 1u) * LANES] : idx;
    out[2 * static_cast<size_t>(idx)] = make_uint4(__float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz), __float_as_uint(curv));
    out[2 * static_cast<size_t>(idx) + 1] = make_uint4(__float_as_uint(r2), m, last, flags);
}

template <int KMAX, int LANES>
__global__ __launch_bounds__(LANES) void k_nrm_knn(const CmFrameState* __restrict__ st, const uint32_t* __restrict__ keys_a,
                                                   const uint32_t* __restrict__ keys_b, const float4* __restrict__ pts,
                                                   const uint2* __restrict__ rows, const float4* __restrict__ recs,
                                                   CmClusterGridDev g, uint32_t n, uint32_t k, float vx, float vy, float vz,
                                                   uint4* __restrict__ out, uint2* __restrict__ list,
                                                   unsigned int* __restrict__ list_n, int first) {
    __shared__ float lst_d[KMAX * LANES];
    __shared__ uint32_t lst_j[KMAX * LANES];
    if (st->status != CM_DEV_OK) return;
    const uint32_t n_items = first ? n : *list_n;
    const uint32_t* __restrict__ keys = pick(st, keys_a, keys_b);
    const uint32_t dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    const float cell = 1.0f / g.inv;                      // (+inf for the one-cell grid, which has no faces)
    const uint32_t kk = (k < n ? k : n) - 1u;             // the others wanted: m - 1
    float* myd = lst_d + threadIdx.x;                     // myd[q * LANES], myj[q * LANES]: the q-th smallest pair so far
    uint32_t* myj = lst_j + threadIdx.x;
    const float inf = __builtin_inff();
    for (uint32_t t = blockIdx.x * LANES + threadIdx.x; t < n_items; t += gridDim.x * LANES) {
        const uint2 item = first ? make_uint2(t, __float_as_uint(inf)) : list[t];
        const uint32_t p = item.x;
        const float4 me = pts[p];
        const uint32_t key = keys[p];
        const uint32_t jk = key / dx, i = key - jk * dx, kz0 = jk / dy, j = jk - kz0 * dy;
        const float bound0 = __uint_as_float(item.y);    // an upper bound on the last pair's d2 (the first launch's), or +inf
        uint32_t cnt = 0;
        auto eff = [&]() { return cnt == kk ? myd[(kk - 1) * LANES] : bound0; };
        auto offer = [&](float d2, uint32_t jr) {
            uint32_t q;
            if (cnt < kk) {
                if (!(d2 <= bound0)) return;              // (equal distances are admitted: they may win by their index)
                q = cnt++;
            } else {
                q = kk - 1;
                if (!pair_less(d2, jr, myd[q * LANES], myj[q * LANES])) return;
            }
            for (; q > 0 && pair_less(d2, jr, myd[(q - 1) * LANES], myj[(q - 1) * LANES]); --q) {
                myd[q * LANES] = myd[(q - 1) * LANES];
                myj[q * LANES] = myj[(q - 1) * LANES];
            }
            myd[q * LANES] = d2;
            myj[q * LANES] = jr;
        };
        // one row: the centroids of cells il..ih, the centroid itself left out
        auto scan_row = [&](uint32_t row, uint32_t il, uint32_t ih) {
            const uint2 r = rows[row];
            if (r.x >= r.y) return;
            const uint32_t lo_key = row * dx + il, hi_key = row * dx + ih;
            uint32_t a = r.x, b = r.y;
            while (a < b) {
                const uint32_t mid = (a + b) >> 1;
                if (keys[mid] < lo_key) a = mid + 1; else b = mid;
            }
            for (uint32_t q = a; q < r.y; ++q) {
                if (keys[q] > hi_key) break;
                if (q == p) continue;
                const float4 c = pts[q];
                offer(d2_of(me, c), __float_as_uint(c.w));
            }
        };
        // the cells of a row that can hold a candidate at or within the current bound in x (the whole row while there is none):
        // |dx| <= sqrt(e) (1 + 2^-22) for every such candidate; the margins cover the root, the rounding of me.x -+ rr and a
        // square that underflowed, the cell on either side the rounding of the cell assignment
        auto x_range = [&](uint32_t& il, uint32_t& ih) {
            const float e = eff();
            il = 0; ih = dx - 1;
            if (e == inf || dx == 1u) return;
            const float rr = __fadd_rn(__fadd_rn(__fmul_rn(__fsqrt_rn(e), 1.0f + 1.0f / (1 << 20)),
                                                 __fmul_rn(fabsf(me.x), 1.0f / (1 << 21))), 1e-22f);
            const float lo = __fsub_rn(floorf(__fmul_rn(__fsub_rn(__fsub_rn(me.x, rr), g.min[0]), g.inv)), 1.0f);
            const float hi = __fadd_rn(floorf(__fmul_rn(__fsub_rn(__fadd_rn(me.x, rr), g.min[0]), g.inv)), 1.0f);
            if (lo > 0.0f) il = lo >= static_cast<float>(dx - 1) ? dx - 1 : static_cast<uint32_t>(lo);
            if (hi < static_cast<float>(dx - 1)) ih = hi < 0.0f ? 0u : static_cast<uint32_t>(hi);
        };
        if (kk == 0u) {                                   // a result of one centroid
            nrm_plane<LANES>(recs, me, myd, myj, 0u, vx, vy, vz, out);
            continue;
        }
        if (first) {
            const uint32_t il = i ? i - 1 : 0u, ih = i + 1 < dx ? i + 1 : dx - 1;
            for (int o = 0; o < 9; ++o) {
                const int jj = static_cast<int>(j) + (o % 3) - 1, kz = static_cast<int>(kz0) + (o / 3) - 1;
                if (jj < 0 || jj >= static_cast<int>(dy) || kz < 0 || kz >= static_cast<int>(dz)) continue;
                scan_row(static_cast<uint32_t>(jj) + static_cast<uint32_t>(kz) * dy, il, ih);
            }
            bool done = false;
            if (cnt == kk) {
                // what lies outside the 3x3x3 block differs by two cells or more along an axis the block does not cover whole
                const bool open = i >= 2 || i + 2 < dx || j >= 2 || j + 2 < dy || kz0 >= 2 || kz0 + 2 < dz;
                const float gp = cell_gap(2, cell);
                done = !open || myd[(kk - 1) * LANES] < __fmul_rn(__fmul_rn(gp, gp), kRel);
            }
            if (!done) {
                const unsigned int slot = atomicAdd(list_n, 1u);
                list[slot] = make_uint2(p, __float_as_uint(cnt == kk ? myd[(kk - 1) * LANES] : inf));
                continue;
            }
        } else {
            const uint32_t s_max = max(max(j, dy - 1 - j), max(kz0, dz - 1 - kz0));
            for (uint32_t s = 0; s <= s_max; ++s) {
                const int si = static_cast<int>(s);
                if (s >= 2 && cnt == kk) {
                    // the rows of ring s and beyond differ by s cells or more in y or z
                    const float gp = cell_gap(si, cell);
                    if (myd[(kk - 1) * LANES] < __fmul_rn(__fmul_rn(gp, gp), kRel)) break;
                }
                for (int dk = -si; dk <= si; ++dk) {
                    const int kz = static_cast<int>(kz0) + dk;
                    if (kz < 0 || kz >= static_cast<int>(dz)) continue;
                    const bool edge_k = dk == -si || dk == si;
                    const int step = (edge_k || si == 0) ? 1 : 2 * si;
                    for (int dj = -si; dj <= si; dj += step) {
                        const int jj = static_cast<int>(j) + dj;
                        if (jj < 0 || jj >= static_cast<int>(dy)) continue;
                        // skip a row wholly beyond the bound (strictly: see the head of the file)
                        const float e = eff();
                        if (e != inf) {
                            const float gy = cell_gap(abs(dj), cell), gz = cell_gap(abs(dk), cell);
                            if (e < __fmul_rn(__fadd_rn(__fmul_rn(gy, gy), __fmul_rn(gz, gz)), kRel)) continue;
                        }
                        uint32_t il, ih;
                        x_range(il, ih);
                        scan_row(static_cast<uint32_t>(jj) + static_cast<uint32_t>(kz) * dy, il, ih);
                    }
                }
            }
        }
        nrm_plane<LANES>(recs, me, myd, myj, kk, vx, vy, vz, out);
    }
}

}  // namespace

// cm_byproducts.cpp normals: *list_n zeroed before the first launch; list = n uint2; out = n entries of 32 bytes. n_items: the
// centroids (first) or the length of the list the first launch left.
void cmk_nrm_knn(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                 const void* rows, const void* recs, const CmClusterGridDev& g, uint32_t n, uint32_t k, const float viewpoint[3],
                 void* out, void* list, uint32_t* list_n, uint32_t n_items, bool first) {
    if (n_items == 0) return;
    const float4* sp = reinterpret_cast<const float4*>(pts);
    const uint2* rw = reinterpret_cast<const uint2*>(rows);
    const float4* rc = reinterpret_cast<const float4*>(recs);
    uint4* o = reinterpret_cast<uint4*>(out);
    uint2* ls = reinterpret_cast<uint2*>(list);
    const int f = first ? 1 : 0;
    const float vx = viewpoint[0], vy = viewpoint[1], vz = viewpoint[2];
    // 8 B per slot: 32 KiB (16 x 256), 64 KiB (32 x 256), 64 KiB (64 x 128) of LDS per workgroup
    if (k <= 16)
        CM_LAUNCH((k_nrm_knn<16, 256>), (n_items + 255) / 256, 256, s, st, keys_a, keys_b, sp, rw, rc, g, n, k, vx, vy, vz, o, ls, list_n, f);
    else if (k <= 32)
        CM_LAUNCH((k_nrm_knn<32, 256>), (n_items + 255) / 256, 256, s, st, keys_a, keys_b, sp, rw, rc, g, n, k, vx, vy, vz, o, ls, list_n, f);
    else
        CM_LAUNCH((k_nrm_knn<64, 128>), (n_items + 127) / 128, 128, s, st, keys_a, keys_b, sp, rw, rc, g, n, k, vx, vy, vz, o, ls, list_n, f);
}
