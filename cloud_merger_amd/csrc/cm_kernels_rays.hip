// cm_kernels_rays.hip — free-space ray casting over the 2-D grid map of the last frame (per-cell pass and end counts, the
// cleared occupancy image), for gfx950.
//
// A by-product computed on request after a frame (cm_result_grid_rays), behind the grid map of the same call. It reads the
// frame's clouds in place exactly as k_grid_bin does, the grid table's state words, and writes buffers of its own only
// (the semantics are in include/cloudmerge.h).
//
//   k_ray_mark    one workgroup per tile of 4096 raw points, the frame's own front end and both masks, the predicate of
//                 k_grid_bin built from the same helpers (grid_axis is cm_search.hpp's). A counted point of descriptor sensor
//                 s in cell c sets bit c of sensor s's bitmap: the set of distinct (sensor, end cell) pairs, which is the ray
//                 set. A word only grows, so the atomicOr is skipped where a plain read shows the bit (max_into's argument).
//   k_ray_cast    one workgroup per run of CM_RAY_RUN words of one sensor's bitmap (blockIdx.y: the sensor). The set bits of
//                 the run are listed in LDS; one wave takes one ray at a time and its lanes take the steps k, k + 64, ... of
//                 the closed form of step 5, so a wave-instruction touches 64 distinct cells (no ray crosses a cell twice).
//                 The crossed cells are gathered in an LDS hash table of (cell, count) — CM_RAY_HASH slots, atomicCAS on the
//                 key, linear probing, CM_RAY_PROBES tries — and flushed once per distinct cell; a step that finds no slot adds
//                 to the table in HBM itself. The end cell's n_end takes one add per ray.
//   k_ray_finish  one thread per cell: the cleared byte from the grid table's state word and n_pass.
//
// Every quantity is an integer count over a set: adds commute, and which way a step took cannot show in the bytes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

#define CM_RAY_EMPTY 0xFFFFFFFFu

__device__ __forceinline__ uint32_t ld_lds(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// bits: n_sensors bitmaps of `words` words each, zero before the launch.
__global__ __launch_bounds__(CM_BLOCK) void k_ray_mark(const CmFrameDev* __restrict__ fd, CmGridDev g,
                                                       const unsigned char* __restrict__ keep,
                                                       const unsigned char* __restrict__ ground,
                                                       uint32_t* __restrict__ bits, uint32_t words) {
    const uint32_t tile = blockIdx.x;
    const uint32_t s = sensor_of_tile(fd, tile);
    const CmSensorDev& sd = fd->s[s];
    const uint32_t first = tile * CM_TILE - sd.base;
    uint32_t* map = bits + static_cast<size_t>(s) * words;
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
        const uint32_t m = 1u << (cell & 31u);
        uint32_t* w = map + (cell >> 5);
        if (!(ld_agent(w) & m)) atomicOr(w, m);
    }
}

// rays: n_cells records of (n_pass, n_end), zero before the launch. blockIdx.y is the descriptor sensor.
__global__ __launch_bounds__(CM_BLOCK) void k_ray_cast(const uint32_t* __restrict__ bits, uint32_t words, CmRayDev rd,
                                                       uint32_t* __restrict__ rays) {
    __shared__ uint32_t s_key[CM_RAY_HASH];
    __shared__ uint32_t s_cnt[CM_RAY_HASH];
    __shared__ uint32_t s_ray[CM_RAY_RUN * 32];       // the end cells of the run's rays
    __shared__ uint32_t s_word[CM_RAY_RUN];
    __shared__ uint32_t s_n;
    const uint32_t s = blockIdx.y;
    if (!rd.has[s]) return;                           // (uniform: the sensor casts nothing)
    const uint32_t w0 = blockIdx.x * CM_RAY_RUN;
    uint32_t mine = 0u;
    if (threadIdx.x < CM_RAY_RUN) {
        const uint32_t w = w0 + threadIdx.x;
        mine = w < words ? bits[static_cast<size_t>(s) * words + w] : 0u;
        s_word[threadIdx.x] = mine;
    }
    if (threadIdx.x == 0) s_n = 0u;
    if (!__syncthreads_or(mine != 0u)) return;        // a run of zero words leaves at once
    for (uint32_t k = threadIdx.x; k < CM_RAY_HASH; k += CM_BLOCK) {
        s_key[k] = CM_RAY_EMPTY;
        s_cnt[k] = 0u;
    }
    // the run's set bits, in any order: the counts do not depend on it
    for (uint32_t b = threadIdx.x; b < CM_RAY_RUN * 32u; b += CM_BLOCK) {
        if (!((s_word[b >> 5] >> (b & 31u)) & 1u)) continue;
        const uint32_t cell = w0 * 32u + b;
        s_ray[atomicAdd(&s_n, 1u)] = cell;
        atomicAdd(rays + static_cast<size_t>(cell) * 2u + 1u, 1u);      // n_end: one add per ray
    }
    __syncthreads();
    const uint32_t n_rays = s_n;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int ox = rd.ox[s], oy = rd.oy[s];
    for (uint32_t r = wave; r < n_rays; r += CM_WAVES) {
        const uint32_t e = s_ray[r];
        const int dx = static_cast<int>(e % rd.nx) - ox, dy = static_cast<int>(e / rd.nx) - oy;
        const uint32_t ax = static_cast<uint32_t>(dx < 0 ? -dx : dx), ay = static_cast<uint32_t>(dy < 0 ? -dy : dy);
        const uint32_t L = ax > ay ? ax : ay;
        const uint32_t K = rd.max_range && rd.max_range < L ? rd.max_range : L;
        // (2 k a + L < 3 * 2^22: a * L < nx * ny, k < L)
        for (uint32_t k = lane; k < K; k += 64u) {
            const uint32_t qx = ax == L ? k : (2u * k * ax + L) / (2u * L);
            const uint32_t qy = ay == L ? k : (2u * k * ay + L) / (2u * L);
            const int cx = ox + (dx < 0 ? -static_cast<int>(qx) : static_cast<int>(qx));
            const int cy = oy + (dy < 0 ? -static_cast<int>(qy) : static_cast<int>(qy));
            const uint32_t cell = static_cast<uint32_t>(cx) + static_cast<uint32_t>(cy) * rd.nx;
            const uint32_t h = (cell * 2654435761u) >> (32 - CM_RAY_HASH_BITS);
            bool placed = false;
            for (int q = 0; q < CM_RAY_PROBES; ++q) {
                const uint32_t at = (h + q) & (CM_RAY_HASH - 1u);
                uint32_t old = ld_lds(&s_key[at]);
                if (old == CM_RAY_EMPTY) old = atomicCAS(&s_key[at], CM_RAY_EMPTY, cell);
                if (old == CM_RAY_EMPTY || old == cell) { atomicAdd(&s_cnt[at], 1u); placed = true; break; }
            }
            if (!placed) atomicAdd(rays + static_cast<size_t>(cell) * 2u, 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < CM_RAY_HASH; k += CM_BLOCK) {
        const uint32_t cell = s_key[k];
        if (cell != CM_RAY_EMPTY) atomicAdd(rays + static_cast<size_t>(cell) * 2u, s_cnt[k]);
    }
}

// grid: the finished cm_grid_cell table (state in word 7); rays: the finished counts; image: the cleared bytes.
__global__ __launch_bounds__(256) void k_ray_finish(const uint32_t* __restrict__ grid, const uint32_t* __restrict__ rays,
                                                    signed char* __restrict__ image, uint32_t n_cells, uint32_t min_pass) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t state = grid[static_cast<size_t>(c) * CM_GRID_WORDS + 7];
    const uint32_t n_pass = rays[static_cast<size_t>(c) * 2u];
    signed char v = state == CM_GRID_OCCUPIED_DEV ? 100 : 0;
    if (state == CM_GRID_UNKNOWN_DEV && n_pass < min_pass) v = -1;
    image[c] = v;
}

}  // namespace

void cmk_ray_mark(hipStream_t s, const CmFrameDev* fd, const CmGridDev& g, const unsigned char* keep, const unsigned char* ground,
                  uint32_t* bits, uint32_t words, uint32_t n_tiles) {
    if (n_tiles) hipLaunchKernelGGL(k_ray_mark, dim3(n_tiles), dim3(CM_BLOCK), 0, s, fd, g, keep, ground, bits, words);
}

void cmk_ray_cast(hipStream_t s, const uint32_t* bits, uint32_t words, const CmRayDev& rd, uint32_t n_sensors, void* rays) {
    if (n_sensors && words)
        hipLaunchKernelGGL(k_ray_cast, dim3((words + CM_RAY_RUN - 1) / CM_RAY_RUN, n_sensors), dim3(CM_BLOCK), 0, s, bits, words, rd,
                           reinterpret_cast<uint32_t*>(rays));
}

void cmk_ray_finish(hipStream_t s, const void* grid, const void* rays, void* image, uint32_t n_cells, uint32_t min_pass) {
    if (n_cells)
        hipLaunchKernelGGL(k_ray_finish, dim3((n_cells + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(grid),
                           reinterpret_cast<const uint32_t*>(rays), reinterpret_cast<signed char*>(image), n_cells, min_pass);
}
