// cm_kernels_grid.hip — the 2-D grid map of the last frame (per-cell counts, lowest and highest return, occupancy), for gfx950.
//
// A by-product computed on request after a frame (cm_result_grid_map), never part of one. It reads the frame's clouds in
// place through the frame descriptor and the two masks (the keep-mask behind cm_merged_copy, the ground mask behind
// cm_ground_copy) and writes into buffers of its own only (the semantics are in include/cloudmerge.h).
//
//   k_grid_bin     one workgroup per tile of 4096 raw points, the frame's own front end (sensor_of_tile, load_point, xf_point,
//                  point_valid) and both masks in the same pass. Every field of a cell is a count or an extreme, so the
//                  records are accumulated as integer images whose zero means "nothing yet" (cm_device.h): adds and maxima
//                  into a table cleared to zero bytes, in any order. A flat stretch of road puts tens of points of one tile
//                  into one cell, so the tile's distinct cells are first gathered in an LDS hash table (CM_GRID_HASH slots,
//                  LDS atomics) and flushed once per cell and tile; a point that finds no slot within CM_GRID_PROBES goes to
//                  the table in HBM itself. Either way a maximum that a plain read shows cannot move the word is skipped
//                  (max_into; it, ld_agent and the images f2ord / ord2f are cm_search.hpp's).
//   k_grid_finish  one thread per cell: the images back to floats (nothing -> the canonical NaN), the state in place, the
//                  occupancy byte.
//
// The table's bytes cannot depend on which way a point took: integer adds and maxima commute.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

// A word of the table in HBM only grows, so max_into (cm_search.hpp) may skip the atomic on a stale read. v == 0 (nothing)
// never goes.
__device__ __forceinline__ void add_into(uint32_t* p, uint32_t v) { if (v) atomicAdd(p, v); }
// A word of the tile's LDS table as other lanes' atomics left it (or a moment earlier: the same argument).
__device__ __forceinline__ uint32_t ld_lds(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One point's or one LDS slot's seven words into cell `cell` of the table.
__device__ __forceinline__ void flush_cell(uint32_t* __restrict__ table, uint32_t cell, const uint32_t (&w)[7]) {
    uint32_t* g = table + static_cast<size_t>(cell) * CM_GRID_WORDS;
    add_into(g + 0, w[0]);
    add_into(g + 1, w[1]);
#pragma unroll
    for (int k = 2; k < 7; ++k) max_into(g + k, w[k]);
}

// (the cell coordinate of step 1, grid_axis, is cm_search.hpp's: k_ray_mark takes the same one)
#define CM_GRID_EMPTY 0xFFFFFFFFu

__global__ __launch_bounds__(CM_BLOCK) void k_grid_bin(const CmFrameDev* __restrict__ fd, CmGridDev g,
                                                       const unsigned char* __restrict__ keep,
                                                       const unsigned char* __restrict__ ground,
                                                       uint32_t* __restrict__ table) {
    __shared__ uint32_t s_key[CM_GRID_HASH];
    __shared__ uint32_t s_w[7][CM_GRID_HASH];
    for (uint32_t k = threadIdx.x; k < CM_GRID_HASH; k += CM_BLOCK) {
        s_key[k] = CM_GRID_EMPTY;
#pragma unroll
        for (int f = 0; f < 7; ++f) s_w[f][k] = 0u;
    }
    __syncthreads();
    const uint32_t tile = blockIdx.x;
    const uint32_t s = sensor_of_tile(fd, tile);
    const CmSensorDev& sd = fd->s[s];
    const uint32_t first = tile * CM_TILE - sd.base;
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = first + r * CM_BLOCK + threadIdx.x;
        if (i >= sd.n) continue;
        const Pt p = load_point(sd.data, sd.layout, sd.point_step, sd.off_x, sd.off_y, sd.off_z, sd.off_i, i);
        float x, y, z;
        xf_point(sd.m, p, x, y, z);
        if (!point_valid(x, y, z, fd->crop_enable, fd->crop_min, fd->crop_max)) continue;
        const uint32_t slot = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        const bool in_a = !keep || keep[slot];
        const bool in_g = ground && ground[slot];
        if (!in_a && !in_g) continue;
        uint32_t ix, iy;
        if (!grid_axis(x, g.origin[0], g.inv, g.nx, &ix) || !grid_axis(y, g.origin[1], g.inv, g.ny, &iy)) continue;
        if (!(g.z_min <= z && z <= g.z_max)) continue;
        const uint32_t cell = ix + iy * g.nx;
        const uint32_t oz = f2ord(z);
        uint32_t w[7];
        w[0] = in_a ? 1u : 0u;
        w[1] = in_g ? 1u : 0u;
        w[2] = in_a ? ~oz : 0u;
        w[3] = in_a ? oz : 0u;
        w[4] = in_g ? ~oz : 0u;
        w[5] = in_g ? oz : 0u;
        w[6] = (p.i == p.i) ? f2ord(p.i) : 0u;
        // the tile's table: linear probing from a multiplicative hash of the cell
        uint32_t h = (cell * 2654435761u) >> 22;
        static_assert(CM_GRID_HASH == 1u << 10, "the hash keeps ten bits");
        bool placed = false;
        for (int q = 0; q < CM_GRID_PROBES; ++q) {
            const uint32_t at = (h + q) & (CM_GRID_HASH - 1u);
            uint32_t old = ld_lds(&s_key[at]);
            if (old == CM_GRID_EMPTY) old = atomicCAS(&s_key[at], CM_GRID_EMPTY, cell);
            if (old == CM_GRID_EMPTY || old == cell) { h = at; placed = true; break; }
        }
        if (!placed) { flush_cell(table, cell, w); continue; }
        if (w[0]) atomicAdd(&s_w[0][h], 1u);
        if (w[1]) atomicAdd(&s_w[1][h], 1u);
#pragma unroll
        for (int k = 2; k < 7; ++k)
            if (w[k] > ld_lds(&s_w[k][h])) atomicMax(&s_w[k][h], w[k]);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < CM_GRID_HASH; k += CM_BLOCK) {
        const uint32_t cell = s_key[k];
        if (cell == CM_GRID_EMPTY) continue;
        uint32_t w[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) w[f] = s_w[f][k];
        flush_cell(table, cell, w);
    }
}

// table: n_cells records of images in, cm_grid_cell out (in place); image: the occupancy bytes.
__global__ __launch_bounds__(256) void k_grid_finish(uint32_t* __restrict__ table, signed char* __restrict__ image, uint32_t n_cells,
                                                     float obstacle_height, uint32_t min_points) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    uint4* rec = reinterpret_cast<uint4*>(table + static_cast<size_t>(c) * CM_GRID_WORDS);
    const uint4 a = rec[0], b = rec[1];
    const uint32_t n = a.x, ng = a.y;
    const uint32_t nan = 0x7FC00000u;
    const uint32_t lo_c = a.z > b.x ? a.z : b.x;     // complements: the larger is the smaller height; 0 where there is none
    uint32_t state = CM_GRID_UNKNOWN_DEV;
    if (n + ng >= min_points) {
        state = CM_GRID_FREE_DEV;
        if (n && __fsub_rn(ord2f(a.w), ord2f(~lo_c)) >= obstacle_height) state = CM_GRID_OCCUPIED_DEV;
    }
    uint4 o0, o1;
    o0.x = n;
    o0.y = ng;
    o0.z = a.z ? __float_as_uint(ord2f(~a.z)) : nan;
    o0.w = a.w ? __float_as_uint(ord2f(a.w)) : nan;
    o1.x = b.x ? __float_as_uint(ord2f(~b.x)) : nan;
    o1.y = b.y ? __float_as_uint(ord2f(b.y)) : nan;
    o1.z = b.z ? __float_as_uint(ord2f(b.z)) : nan;
    o1.w = state;
    rec[0] = o0;
    rec[1] = o1;
    image[c] = state == CM_GRID_UNKNOWN_DEV ? -1 : (state == CM_GRID_FREE_DEV ? 0 : 100);
}

}  // namespace

void cmk_grid_bin(hipStream_t s, const CmFrameDev* fd, const CmGridDev& g, const unsigned char* keep, const unsigned char* ground,
                  void* table, uint32_t n_tiles) {
    if (n_tiles) hipLaunchKernelGGL(k_grid_bin, dim3(n_tiles), dim3(CM_BLOCK), 0, s, fd, g, keep, ground, reinterpret_cast<uint32_t*>(table));
}

void cmk_grid_finish(hipStream_t s, void* table, void* image, uint32_t n_cells, float obstacle_height, uint32_t min_points) {
    if (n_cells)
        hipLaunchKernelGGL(k_grid_finish, dim3((n_cells + 255) / 256), dim3(256), 0, s, reinterpret_cast<uint32_t*>(table),
                           reinterpret_cast<signed char*>(image), n_cells, obstacle_height, min_points);
}
