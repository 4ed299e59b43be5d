// cm_kernels_cast.hip — the cast layer behind the cost layer: from many poses, in many directions, the first occupied cell of
// the occupancy map on an integer line (amcl's beam model and a virtual LaserScan want these expected ranges), for gfx950
// (wave64).
//
// Computed on request (cm_map_cast_evaluate / _evaluate_mcl) from the map's image and info, the cost layer's dist2 and the
// poses; it writes buffers of the cast layer only (the semantics are in include/cloudmerge.h). Everything after
// the origin cell is integer arithmetic (cm_cast_math.hpp, shared with the host), so neither the lanes, the order of the
// atomics nor the grid can show in a table.
//
//   k_cast_steps   one thread per four window cells: the skip table, one byte per cell from dist2 (0 on an occupied cell,
//                  otherwise the smallest j >= 1 with 2 j^2 >= dist2, capped at 255), stored as one word. Run by the first
//                  evaluate after a cost update, never under CM_CAST_PLAIN.
//   k_cast_rays    one lane per ray, CM_CAST_BLOCK threads per workgroup, the grid sized to the device with a stride over the
//                  rays; ray p * n_bearings + a, so a wave holds consecutive bearings of one pose and its lanes walk
//                  neighbouring cells. The workgroup stages the direction table (16 KiB) in LDS once. A lane reads its pose
//                  (three words, the same address across most of a wave) and its bearing, finds the origin cell by the map's
//                  step 1, and walks: by default it jumps steps[cell] steps at a time and never looks past the last step inside
//                  the window, which it finds up front; under CM_CAST_PLAIN it goes cell by cell through the image. Pose and
//                  bearing of a ray index come from an exact quotient by an fp32 reciprocal with one correction, as the
//                  line's cells do: no emulated integer division. The record leaves as one 8-byte vector store. The four
//                  status counts are summed per lane over the stride, per wave by shuffles, per workgroup in LDS, then one
//                  integer atomicAdd per non-zero count and workgroup.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

#define CM_CAST_FN __device__ __forceinline__
#define CM_CAST_RCP(d) __builtin_amdgcn_rcpf(d)
#include "cm_cast_math.hpp"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m));
    return v;
}

__global__ __launch_bounds__(CM_CAST_BLOCK) void k_cast_steps(const uint32_t* __restrict__ dist2, uint32_t n_cells, unsigned char* __restrict__ steps) {
    const uint32_t c0 = (blockIdx.x * CM_CAST_BLOCK + threadIdx.x) * 4u;
    if (c0 >= n_cells) return;
    if (c0 + 4u <= n_cells) {
        uint32_t w = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) w |= cm_cast_step_of(dist2[c0 + i], CM_CAST_STEP_CAP) << (8u * i);
        *reinterpret_cast<uint32_t*>(steps + c0) = w;                  // (c0 is a multiple of 4 and the table an allocation of its own)
    } else {
        for (uint32_t c = c0; c < n_cells; ++c) steps[c] = static_cast<unsigned char>(cm_cast_step_of(dist2[c], CM_CAST_STEP_CAP));
    }
}

__global__ __launch_bounds__(CM_CAST_BLOCK) void k_cast_rays(const signed char* __restrict__ image, const unsigned char* __restrict__ steps, CmCastDev g,
                                                             const uint32_t* __restrict__ poses, const uint32_t* __restrict__ bearings,
                                                             const uint32_t* __restrict__ dirs, uint2* __restrict__ rays, uint32_t* __restrict__ words) {
    __shared__ uint32_t s_dir[CM_CAST_DIRS];
    __shared__ uint32_t s_cnt[CM_CAST_BLOCK / 64][CM_CAST_WORDS];
    for (uint32_t i = threadIdx.x; i < CM_CAST_DIRS / 4; i += CM_CAST_BLOCK)
        reinterpret_cast<uint4*>(s_dir)[i] = reinterpret_cast<const uint4*>(dirs)[i];
    __syncthreads();
    const uint32_t n_rays = g.n_poses * g.n_bearings;                  // (<= 2^24)
    const float r_nb = __builtin_amdgcn_rcpf(static_cast<float>(g.n_bearings));
    uint32_t n_max = 0u, n_hit = 0u, n_off = 0u, n_none = 0u;
    for (uint32_t r = blockIdx.x * CM_CAST_BLOCK + threadIdx.x; r < n_rays; r += gridDim.x * CM_CAST_BLOCK) {
        const uint32_t p = cm_cast_quot(r, g.n_bearings, r_nb), a = r - p * g.n_bearings;      // (r < 2^24, p < 2^16)
        const uint32_t* const q = poses + static_cast<size_t>(p) * g.pose_words;
        const float x = __builtin_bit_cast(float, q[0]), y = __builtin_bit_cast(float, q[1]);
        const uint32_t e = s_dir[((q[2] + bearings[a] + 0x80000u) >> 20) & (CM_CAST_DIRS - 1u)];
        const int32_t dx = static_cast<int16_t>(e & 0xFFFFu), dy = static_cast<int16_t>(e >> 16);
        int gx = 0, gy = 0;
        const bool exists = world_axis(x, g.inv, &gx) & world_axis(y, g.inv, &gy);
        // (|gx| < 2^30 and |ax| < 2^30 + 2^21: the wrapped difference is below nx only where the true one is)
        const uint32_t ox = static_cast<uint32_t>(gx) - static_cast<uint32_t>(g.ax), oy = static_cast<uint32_t>(gy) - static_cast<uint32_t>(g.ay);
        CmCastWords w;
        w.a = 3u << 16;                                                // CM_CAST_NO_ORIGIN, k 0
        w.b = 0u;
        if (exists && ox < g.nx && oy < g.ny) w = g.plain ? cm_cast_walk_plain(dx, dy, ox, oy, g.nx, g.ny, image) : cm_cast_walk_skip(dx, dy, ox, oy, g.nx, g.ny, steps);
        rays[r] = make_uint2(w.a, w.b);
        const uint32_t status = w.a >> 16;
        n_max += status == 0u;
        n_hit += status == 1u;
        n_off += status == 2u;
        n_none += status == 3u;
    }
    n_max = wave_sum(n_max);
    n_hit = wave_sum(n_hit);
    n_off = wave_sum(n_off);
    n_none = wave_sum(n_none);
    if ((threadIdx.x & 63u) == 0u) {
        uint32_t* const s = s_cnt[threadIdx.x >> 6];
        s[0] = n_max;
        s[1] = n_hit;
        s[2] = n_off;
        s[3] = n_none;
    }
    __syncthreads();
    if (threadIdx.x < CM_CAST_WORDS) {
        uint32_t t = 0u;
        for (uint32_t v = 0; v < CM_CAST_BLOCK / 64; ++v) t += s_cnt[v][threadIdx.x];
        if (t) atomicAdd(words + threadIdx.x, t);                      // (integers: the order cannot show)
    }
}

bool cast_ok(const CmCastDev& g) {
    return g.nx >= 1 && g.ny >= 1 && static_cast<uint64_t>(g.nx) * g.ny <= (1u << 22) && g.n_poses >= 1 && g.n_poses <= CM_CAST_MAX_POSES_DEV &&
           g.n_bearings >= 1 && g.n_bearings <= CM_CAST_MAX_BEARINGS_DEV && static_cast<uint64_t>(g.n_poses) * g.n_bearings <= CM_CAST_MAX_RAYS_DEV &&
           (g.pose_words == 3u || g.pose_words == 6u);
}

// Workgroups of k_cast_rays: enough to fill the device a few times over, never more than the rays need.
uint32_t cast_grid(uint32_t n_rays) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint32_t want = (n_rays + CM_CAST_BLOCK - 1) / CM_CAST_BLOCK, cap = static_cast<uint32_t>(cus) * 8u;
    return want < cap ? want : cap;
}

}  // namespace

void cmk_cast_steps(hipStream_t s, const uint32_t* dist2, uint32_t n_cells, unsigned char* steps) {
    const uint32_t n_threads = (n_cells + 3u) / 4u;
    if (n_threads) hipLaunchKernelGGL(k_cast_steps, dim3((n_threads + CM_CAST_BLOCK - 1) / CM_CAST_BLOCK), dim3(CM_CAST_BLOCK), 0, s, dist2, n_cells, steps);
}

void cmk_cast_rays(hipStream_t s, const void* image, const unsigned char* steps, const CmCastDev& g, const void* poses, const uint32_t* bearings,
                   const void* dirs, void* rays, uint32_t* words) {
    if (!cast_ok(g)) return;
    hipLaunchKernelGGL(k_cast_rays, dim3(cast_grid(g.n_poses * g.n_bearings)), dim3(CM_CAST_BLOCK), 0, s, static_cast<const signed char*>(image), steps, g,
                       static_cast<const uint32_t*>(poses), bearings, static_cast<const uint32_t*>(dirs), static_cast<uint2*>(rays), words);
}
