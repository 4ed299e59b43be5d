// cm_kernels_cost.hip — the cost layer over the occupancy map: the exact squared Euclidean distance of every window cell to
// the nearest occupied cell, and costmap_2d's inflated cost from it, for gfx950 (wave64).
//
// Computed on request (cm_map_cost_update) from the map's three-valued image; it writes buffers of the cost layer only
// (the semantics are in include/cloudmerge.h). The transform is separable: dist2(x, y) is the minimum over x'
// of (x - x')^2 + g(x', y)^2, g the vertical distance to the nearest obstacle of column x'. Everything is an integer, so the
// order of evaluation cannot show in the bytes.
//
//   k_cost_colmask   one thread per column and block of CM_COST_ROWS rows: the obstacle bits of its 32 cells as one word.
//                    Lanes run along x, so every one of the 32 loads of a wave reads 64 neighbouring bytes; the loads do
//                    not depend on one another.
//   k_cost_colcarry  one thread per word of that table: the nearest obstacle row above and below its block, found by walking
//                    the column's words outwards until one is not zero (at most ny / 32 of them, 4 bytes each, from L2).
//                    With the block's own word these two rows give g of every cell of the block without a scan: the
//                    highest set bit at or below the row, the lowest at or above it. No thread walks 2048 rows.
//   k_cost_rows      one workgroup per row. g^2 of the row from the two tables into LDS (nx words, at most 8 KB), then
//                    each lane scans outwards from its cell, dx = 1, 2, ..., and stops once dx^2 reaches its best:
//                    neighbouring lanes read neighbouring words, so no bank conflict, and the work follows the distances
//                    that are present, not nx. The same thread writes dist2 and, from the image byte and the table
//                    (read through the cache: the entries a row needs are few and shared by every row), the cost.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_device.h"
#include "cm_kernels.h"

namespace {

constexpr uint32_t kNoDist = 0xFFFFFFFFu;          // CM_MAP_DIST_NONE

__global__ __launch_bounds__(CM_COST_BLOCK) void k_cost_colmask(const signed char* __restrict__ image, CmCostDev g,
                                                                uint32_t* __restrict__ masks) {
    const uint32_t x = blockIdx.x * CM_COST_BLOCK + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (x >= g.nx) return;
    const uint32_t y0 = b * CM_COST_ROWS;
    // (a row beyond the window reads the last row instead and counts for nothing: 32 loads with no branch between them)
    signed char v[CM_COST_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < CM_COST_ROWS; ++r) {
        const uint32_t y = y0 + r < g.ny ? y0 + r : g.ny - 1u;
        v[r] = image[y * g.nx + x];
    }
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t r = 0; r < CM_COST_ROWS; ++r)
        m |= (y0 + r < g.ny && v[r] == 100 ? 1u : 0u) << r;
    masks[b * g.nx + x] = m;
}

__global__ __launch_bounds__(CM_COST_BLOCK) void k_cost_colcarry(const uint32_t* __restrict__ masks, CmCostDev g,
                                                                 uint32_t* __restrict__ carry) {
    const uint32_t x = blockIdx.x * CM_COST_BLOCK + threadIdx.x;
    const uint32_t b = blockIdx.y;
    if (x >= g.nx) return;
    const uint32_t nb = (g.ny + CM_COST_ROWS - 1) / CM_COST_ROWS;
    uint32_t up = CM_COST_NO_ROW, dn = CM_COST_NO_ROW;
    for (uint32_t k = b; k-- > 0;) {
        const uint32_t m = masks[k * g.nx + x];
        if (m) { up = k * CM_COST_ROWS + 31u - static_cast<uint32_t>(__clz(m)); break; }
    }
    for (uint32_t k = b + 1; k < nb; ++k) {
        const uint32_t m = masks[k * g.nx + x];
        if (m) { dn = k * CM_COST_ROWS + static_cast<uint32_t>(__ffs(m)) - 1u; break; }
    }
    carry[b * g.nx + x] = up | (dn << 16);
}

__global__ __launch_bounds__(CM_COST_BLOCK) void k_cost_rows(const signed char* __restrict__ image,
                                                             const uint32_t* __restrict__ masks,
                                                             const uint32_t* __restrict__ carry,
                                                             const unsigned char* __restrict__ lut, CmCostDev g,
                                                             uint32_t* __restrict__ dist2, unsigned char* __restrict__ cost) {
    __shared__ uint32_t g2[CM_COST_MAX_AXIS_DEV];
    const uint32_t y = blockIdx.x;
    const uint32_t b = y / CM_COST_ROWS, r = y % CM_COST_ROWS;
    for (uint32_t x = threadIdx.x; x < g.nx; x += CM_COST_BLOCK) {
        const uint32_t m = masks[b * g.nx + x];
        const uint32_t cw = carry[b * g.nx + x];
        const uint32_t at_or_above = m & (0xFFFFFFFFu >> (31u - r)), at_or_below = m >> r;
        const uint32_t yu = at_or_above ? b * CM_COST_ROWS + 31u - static_cast<uint32_t>(__clz(at_or_above)) : (cw & 0xFFFFu);
        const uint32_t yd = at_or_below ? y + static_cast<uint32_t>(__ffs(at_or_below)) - 1u : (cw >> 16);
        const uint32_t gu = yu == CM_COST_NO_ROW ? CM_COST_FAR : y - yu;
        const uint32_t gd = yd == CM_COST_NO_ROW ? CM_COST_FAR : yd - y;
        const uint32_t gv = gu < gd ? gu : gd;
        g2[x] = gv == CM_COST_FAR ? CM_COST_FAR : gv * gv;
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < g.nx; x += CM_COST_BLOCK) {
        uint32_t best = g2[x];
        const uint32_t left = x, right = g.nx - 1u - x;
        const uint32_t reach = left > right ? left : right;
        for (uint32_t dx = 1; dx <= reach && dx * dx < best; ++dx) {
            const uint32_t a = dx <= left ? g2[x - dx] : CM_COST_FAR;
            const uint32_t c = dx <= right ? g2[x + dx] : CM_COST_FAR;
            const uint32_t v = (a < c ? a : c) + dx * dx;      // (at most CM_COST_FAR + 2047^2: no overflow)
            best = v < best ? v : best;
        }
        const uint32_t d = best >= CM_COST_FAR ? kNoDist : best;
        const uint32_t cell = y * g.nx + x;
        dist2[cell] = d;
        const uint32_t infl = d <= g.r2 ? lut[d] : 0u;
        const int v = image[cell];
        uint32_t out;
        if (v == 100) out = 254u;
        else if (v == 0) out = infl;
        else out = (g.inflate_unknown ? infl > 0u : infl >= 253u) ? infl : 255u;
        cost[cell] = static_cast<unsigned char>(out);
    }
}

bool cost_window_ok(const CmCostDev& g) {
    return g.nx >= 1 && g.ny >= 1 && g.nx <= CM_COST_MAX_AXIS_DEV && g.ny <= CM_COST_MAX_AXIS_DEV;
}

dim3 cost_column_grid(const CmCostDev& g) {
    return dim3((g.nx + CM_COST_BLOCK - 1) / CM_COST_BLOCK, (g.ny + CM_COST_ROWS - 1) / CM_COST_ROWS);
}

}  // namespace

void cmk_cost_colmask(hipStream_t s, const void* image, const CmCostDev& g, uint32_t* masks) {
    if (!cost_window_ok(g)) return;
    hipLaunchKernelGGL(k_cost_colmask, cost_column_grid(g), dim3(CM_COST_BLOCK), 0, s, reinterpret_cast<const signed char*>(image), g, masks);
}

void cmk_cost_colcarry(hipStream_t s, const uint32_t* masks, const CmCostDev& g, uint32_t* carry) {
    if (!cost_window_ok(g)) return;
    hipLaunchKernelGGL(k_cost_colcarry, cost_column_grid(g), dim3(CM_COST_BLOCK), 0, s, masks, g, carry);
}

void cmk_cost_rows(hipStream_t s, const void* image, const uint32_t* masks, const uint32_t* carry, const unsigned char* lut,
                   const CmCostDev& g, uint32_t* dist2, unsigned char* cost) {
    if (!cost_window_ok(g)) return;
    hipLaunchKernelGGL(k_cost_rows, dim3(g.ny), dim3(CM_COST_BLOCK), 0, s, reinterpret_cast<const signed char*>(image), masks, carry, lut, g,
                       dist2, cost);
}
