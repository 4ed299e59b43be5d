// cm_search.hpp — device helpers shared by the by-product kernel files (cm_kernels_cluster / box / grid / rays / sor / normals /
// align / cov / ndt .hip): the order-preserving image of a float, the guarded one-way atomics, the uncontracted fp64
// operations, the fp32 squared distance in its one operation order, the lower bound in a sorted key array, the cell of a
// coordinate in a search grid, and the three walks over a search grid's sorted cells. The frame path's
// helpers are cm_common.hpp's; nothing here is used by a frame except d2_of in the radius stage.
//
// Why once. The clusters, the ICP matches, the normals' neighbour lists and the SOR distances are bit-exact against their
// restatements only because every kernel computes the same cell of a coordinate and the same d2 of a pair, and visits every
// candidate a grid holds. A by-product that searches the grid takes all of that from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CM_LAUNCH(kernel, grid, block, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, __VA_ARGS__)

namespace {

// ------------------------------------------------------------------------------------------------
// scalar helpers
// ------------------------------------------------------------------------------------------------
// Order-preserving image of a float (-inf < ... < -0 < +0 < ... < +inf) and back. Host code decodes the images it copies out
// (cm_byproducts.cpp result_bounds) with the same function.
__host__ __device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ float ord2f(uint32_t o) {
    return __builtin_bit_cast(float, o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// A word that other workgroups' atomics move, read past the CU's L1 (relaxed, agent scope).
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// atomicMin / atomicMax that skip the atomic when the word already holds a value at least as good (the word only moves
// one way, so a stale read can only cost an atomic, never lose one).
__device__ __forceinline__ void min_into(uint32_t* p, uint32_t v) { if (v < ld_agent(p)) atomicMin(p, v); }
__device__ __forceinline__ void max_into(uint32_t* p, uint32_t v) { if (v > ld_agent(p)) atomicMax(p, v); }

// The lock-free union-find on 32-bit parent words that the frontier layer's merge and the localisation layer's hypotheses
// share. Every word holds an element of the same tree that is not above it, a root holds itself: a walk strictly decreases
// and ends. No thread waits on another.
__device__ __forceinline__ uint32_t cm_uf_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ uint32_t cm_uf_find(const uint32_t* parent, uint32_t c) {
    uint32_t p = cm_uf_load(parent + c);
    while (p != c) {
        c = p;
        p = cm_uf_load(parent + c);
    }
    return c;
}
// Unites the trees of a and b. The larger root's word falls to the smaller root; if the word was no root any more (another
// thread hung it elsewhere in the meantime), what it held still has to meet the smaller root, and the larger of the two
// elements in hand has strictly fallen.
__device__ __forceinline__ void cm_uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    a = cm_uf_find(parent, a);
    b = cm_uf_find(parent, b);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) break;
        a = cm_uf_find(parent, old);
        b = cm_uf_find(parent, b);
    }
}

// fp64, every operation rounded on its own whatever the contraction setting.
__device__ __forceinline__ double dadd(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double dsub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double dmul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double ddiv(double a, double b) { return __ddiv_rn(a, b); }

// The fp32 squared distance of the radius stage, (ex ex + ey ey) + ez ez with every operation rounded on its own: the one
// d2 of every neighbour predicate and every neighbour order (.w is not read).
__device__ __forceinline__ float d2_of(const float4& a, const float4& b) {
    const float ex = __fsub_rn(a.x, b.x), ey = __fsub_rn(a.y, b.y), ez = __fsub_rn(a.z, b.z);
    return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}

constexpr float kRel = 1.0f - 1.0f / (1 << 20);        // margin of every pruning bound against fp32 rounding

// First index in keys[lo, hi) whose value is >= v (hi where there is none); keys ascending.
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// The cell of a coordinate along one axis of a search grid (CmClusterGridDev: min, inv, dims), clamped into the grid:
// clamp(floor(fl(fl(x - min) * inv)), 0, dim - 1), monotone in x. (fmaxf drops a NaN — an infinite offset times the zero
// inverse of the one-cell grid — onto cell 0.)
__device__ __forceinline__ uint32_t grid_cell(float x, float mn, float inv, uint32_t dim) {
    const float v = floorf(__fmul_rn(__fsub_rn(x, mn), inv));
    return static_cast<uint32_t>(fminf(fmaxf(v, 0.0f), static_cast<float>(dim - 1u)));
}

// The cell coordinate of the 2-D grid map's step 1 on one axis (include/cloudmerge.h): false when the point is outside the
// grid (a t of +-inf or NaN included). The one membership test of k_grid_bin and k_ray_mark.
__device__ __forceinline__ bool grid_axis(float p, float origin, float inv, uint32_t n, uint32_t* i) {
    const float c = floorf(__fmul_rn(__fsub_rn(p, origin), inv));
    if (!(c >= 0.0f && c < static_cast<float>(n))) return false;
    *i = static_cast<uint32_t>(static_cast<int>(c));
    return true;
}

// The absolute cell of a world coordinate on one axis, the occupancy map's step 1 (include/cloudmerge.h): floorf(w * inv),
// false when it is not strictly inside +-2^30 (a w of +-inf or NaN included). No origin is subtracted: the lattice never
// moves. The one cell computation of k_map_mark.
__device__ __forceinline__ bool world_axis(float w, float inv, int* g) {
    const float c = floorf(__fmul_rn(w, inv));
    if (!(c > -1073741824.0f && c < 1073741824.0f)) return false;
    *g = static_cast<int>(c);
    return true;
}

// ------------------------------------------------------------------------------------------------
// walks over the sorted cells of a search grid: keys ascending, key = x + dx * row, row = y + dy * z; the (y,z)-row table
// gives each row's range of sorted positions
// ------------------------------------------------------------------------------------------------
// visit(t) for every sorted position t in [first, end) of row `row` whose cell lies in x_lo..x_hi, ascending. [first, end)
// is the row's range or the head of it.
template <class Visit>
__device__ __forceinline__ void for_row_cells(const uint32_t* __restrict__ keys, uint32_t first, uint32_t end, uint32_t row,
                                              uint32_t dx, uint32_t x_lo, uint32_t x_hi, Visit&& visit) {
    if (first >= end) return;
    const uint32_t k_lo = row * dx + x_lo, k_hi = row * dx + x_hi;
    for (uint32_t t = lower_bound_u32(keys, first, end, k_lo); t < end; ++t) {
        if (keys[t] > k_hi) break;
        visit(t);
    }
}

// visit_row(row) for the up to nine rows around row (j, k) that lie inside the dy x dz grid: z - 1 first, y - 1 first.
template <class VisitRow>
__device__ __forceinline__ void for_rows_3x3(uint32_t j, uint32_t k, uint32_t dy, uint32_t dz, VisitRow&& visit_row) {
    for (int o = 0; o < 9; ++o) {
        const int jj = static_cast<int>(j) + (o % 3) - 1, kz = static_cast<int>(k) + (o / 3) - 1;
        if (jj < 0 || jj >= static_cast<int>(dy) || kz < 0 || kz >= static_cast<int>(dz)) continue;
        visit_row(static_cast<uint32_t>(jj) + static_cast<uint32_t>(kz) * dy);
    }
}

// visit_row(row, dj, dk) for the rows of the Chebyshev ring s around row (j, k) that lie inside the grid (s = 0: the row
// itself): dk ascending, dj ascending inside; the rows with |dk| < s are the two with |dj| = s.
template <class VisitRow>
__device__ __forceinline__ void for_row_ring(uint32_t s, uint32_t j, uint32_t k, uint32_t dy, uint32_t dz, VisitRow&& visit_row) {
    const int si = static_cast<int>(s);
    for (int dk = -si; dk <= si; ++dk) {
        const int kz = static_cast<int>(k) + dk;
        if (kz < 0 || kz >= static_cast<int>(dz)) continue;
        const bool edge_k = dk == -si || dk == si;
        const int step = (edge_k || si == 0) ? 1 : 2 * si;
        for (int dj = -si; dj <= si; dj += step) {
            const int jj = static_cast<int>(j) + dj;
            if (jj < 0 || jj >= static_cast<int>(dy)) continue;
            visit_row(static_cast<uint32_t>(jj) + static_cast<uint32_t>(kz) * dy, dj, dk);
        }
    }
}

}  // namespace
