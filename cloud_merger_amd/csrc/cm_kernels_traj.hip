// cm_kernels_traj.hip — the rollout layer behind the plan layer: sampled velocity commands rolled forward from a pose, their
// footprint checked against the inflated costmap pose by pose, scored by the largest cost byte met and by the plan layer's
// potential at the end (base_local_planner's rollout without its wavefront: pot is that grid), for gfx950 (wave64).
//
// Computed on request (cm_map_traj_evaluate) from the cost layer's cost table and the plan layer's pot; it writes buffers of
// the rollout layer only (the semantics are in include/cloudmerge.h). Positions are fp32 with every operation
// rounded on its own (the _rn intrinsics: nothing contracts), headings and scores are integers, and the class of a pose is a
// vote over its points, so neither the lanes nor the batches can show in the records.
//
//   k_traj_roll   one wave per trajectory, CM_TRAJ_WAVES waves per workgroup. Every lane carries the pose recurrence (it is
//                 wave-uniform: a table entry, one multiplication and one addition per axis, one integer addition). The wave
//                 advances CM_TRAJ_STEP_BATCH poses, then its lanes stride over the n_foot + 1 points (the centre is point
//                 0) and each lane issues the cost-byte loads of its point under all poses of the batch before it looks at
//                 any of them: the loads do not depend on one another, only the decision to stop does. Per pose the lanes
//                 vote (off map, collision) in pose order; the first bad pose ends the wave as a whole. A valid trajectory
//                 ends with a wave maximum over the lanes' largest bytes and one read of pot. Lane 0 writes the record.
//                 The heading table (32 KiB) is read through the caches; with CM_TRAJ_DIRS_LDS every workgroup stages it
//                 in LDS first (measured slower).
//   k_traj_best   one workgroup: every thread takes records tid, tid + CM_TRAJ_BEST_BLOCK, ..., keeps the smallest
//                 (total, index) among the valid ones and counts them; a wave reduction, then one across the waves in LDS.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

constexpr uint32_t kUnreachable = 0xFFFFFFFFu;     // CM_PLAN_UNREACHABLE
constexpr int kBatch = CM_TRAJ_STEP_BATCH;

// Step 2: the table entry of a heading.
__device__ __forceinline__ uint32_t heading_entry(uint32_t h) { return ((h + 0x80000u) >> 20) & (CM_TRAJ_HEADINGS_DEV - 1u); }

__global__ __launch_bounds__(CM_TRAJ_WAVES * 64) void k_traj_roll(const unsigned char* __restrict__ cost, const uint32_t* __restrict__ pot,
                                                                  CmTrajDev g, const float* __restrict__ steps, const uint32_t* __restrict__ dh,
                                                                  const float2* __restrict__ dirs_hbm, const float2* __restrict__ foot,
                                                                  CmTrajScoreDev* __restrict__ out) {
#if CM_TRAJ_DIRS_LDS
    __shared__ float2 s_dirs[CM_TRAJ_HEADINGS_DEV];
    for (uint32_t i = threadIdx.x; i < CM_TRAJ_HEADINGS_DEV; i += CM_TRAJ_WAVES * 64) s_dirs[i] = dirs_hbm[i];
    __syncthreads();                                   // (before any wave leaves)
    const float2* const dirs = s_dirs;
#else
    const float2* const dirs = dirs_hbm;
#endif
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * CM_TRAJ_WAVES + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    if (t >= g.nv * g.nw) return;                      // (the whole wave)
    const float sl = steps[t / g.nw];
    const uint32_t d = dh[t % g.nw];
    const uint32_t n_pts = g.n_foot + 1u;
    float x = g.x, y = g.y, ex = g.x, ey = g.y;
    uint32_t h = g.h0;
    float2 e = dirs[heading_entry(h)];
    uint32_t occ = 0u, status = CM_TRAJ_VALID_DEV, bad_step = 0u;
    for (uint32_t k0 = 0; k0 < g.n_steps && status == CM_TRAJ_VALID_DEV; k0 += kBatch) {
        // step 3: the poses k0 + 1 .. k0 + kBatch (those beyond n_steps are computed and never looked at)
        float px[kBatch], py[kBatch], pc[kBatch], ps[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            x = __fadd_rn(x, __fmul_rn(sl, e.x));
            y = __fadd_rn(y, __fmul_rn(sl, e.y));
            h += d;
            e = dirs[heading_entry(h)];
            px[b] = x;
            py[b] = y;
            pc[b] = e.x;
            ps[b] = e.y;
        }
        // steps 4 and 5 per lane: its points under every pose of the batch
        uint32_t off[kBatch], hit[kBatch], mx[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) off[b] = hit[b] = mx[b] = 0u;
        for (uint32_t p = lane; p < n_pts; p += 64u) {
            const float2 f = p ? foot[p - 1u] : make_float2(0.0f, 0.0f);      // (point 0: the centre; adding and subtracting zeros leaves its cell)
            uint32_t v[kBatch];
            bool in[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const float wx = __fsub_rn(__fadd_rn(px[b], __fmul_rn(pc[b], f.x)), __fmul_rn(ps[b], f.y));
                const float wy = __fadd_rn(__fadd_rn(py[b], __fmul_rn(ps[b], f.x)), __fmul_rn(pc[b], f.y));
                int gx = 0, gy = 0;
                const bool exists = world_axis(wx, g.inv, &gx) & world_axis(wy, g.inv, &gy);
                // (|gx| < 2^30 and |ax| < 2^30 + 2^21: the wrapped difference is below nx only where the true one is)
                const uint32_t ix = static_cast<uint32_t>(gx) - static_cast<uint32_t>(g.ax), iy = static_cast<uint32_t>(gy) - static_cast<uint32_t>(g.ay);
                in[b] = exists && ix < g.nx && iy < g.ny;
                v[b] = in[b] && k0 + b < g.n_steps ? cost[iy * g.nx + ix] : 0u;
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const bool live = k0 + b < g.n_steps;
                off[b] |= live && !in[b] ? 1u : 0u;
                hit[b] |= live && in[b] && (v[b] == 254u || (v[b] == 255u && !g.allow_unknown) || (p == 0u && v[b] == 253u)) ? 1u : 0u;
                const uint32_t contributes = v[b] == 255u ? 0u : v[b];
                mx[b] = contributes > mx[b] ? contributes : mx[b];
            }
        }
        // the votes, in pose order: the first bad pose ends the trajectory
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (status != CM_TRAJ_VALID_DEV || k0 + b >= g.n_steps) break;
            ex = px[b];
            ey = py[b];
            const bool any_off = __any(static_cast<int>(off[b])) != 0, any_hit = __any(static_cast<int>(hit[b])) != 0;
            if (any_off || any_hit) {
                status = any_off ? CM_TRAJ_OFF_MAP_DEV : CM_TRAJ_COLLISION_DEV;
                bad_step = k0 + static_cast<uint32_t>(b) + 1u;
            }
            occ = mx[b] > occ ? mx[b] : occ;
        }
    }
    uint32_t pot_end = kUnreachable;
    if (status == CM_TRAJ_VALID_DEV) {
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(occ), m));
            occ = o > occ ? o : occ;
        }
        // step 6: the last pose passed step 5, so its centre's cell is in the window
        int gx = 0, gy = 0;
        world_axis(ex, g.inv, &gx);
        world_axis(ey, g.inv, &gy);
        const uint32_t ix = static_cast<uint32_t>(gx) - static_cast<uint32_t>(g.ax), iy = static_cast<uint32_t>(gy) - static_cast<uint32_t>(g.ay);
        if (ix < g.nx && iy < g.ny) pot_end = pot[iy * g.nx + ix];
        if (pot_end == kUnreachable) {
            status = CM_TRAJ_NO_POTENTIAL_DEV;
            bad_step = g.n_steps;
        }
    }
    if (lane == 0u) {
        const bool valid = status == CM_TRAJ_VALID_DEV;
        CmTrajScoreDev r;
        r.status = status;
        r.bad_step = bad_step;
        r.occ = valid ? occ : 0u;
        r.pot_end = valid ? pot_end : kUnreachable;
        r.total = valid ? static_cast<unsigned long long>(g.occ_scale) * occ + static_cast<unsigned long long>(g.goal_scale) * pot_end : ~0ull;
        r.end_x = ex;
        r.end_y = ey;
        out[t] = r;
    }
}

// info: CM_TRAJ_INFO_WORDS words { best, n_valid }.
__global__ __launch_bounds__(CM_TRAJ_BEST_BLOCK) void k_traj_best(const CmTrajScoreDev* __restrict__ scores, uint32_t n, uint32_t* __restrict__ info) {
    __shared__ unsigned long long s_total[CM_TRAJ_BEST_BLOCK / 64];
    __shared__ uint32_t s_index[CM_TRAJ_BEST_BLOCK / 64], s_count[CM_TRAJ_BEST_BLOCK / 64];
    unsigned long long total = ~0ull;
    uint32_t index = 0xFFFFFFFFu, count = 0u;          // CM_TRAJ_NONE
    for (uint32_t i = threadIdx.x; i < n; i += CM_TRAJ_BEST_BLOCK) {      // (ascending i: a tie keeps the lower index)
        if (scores[i].status != CM_TRAJ_VALID_DEV) continue;
        ++count;
        const unsigned long long v = scores[i].total;
        if (index == 0xFFFFFFFFu || v < total) {
            total = v;
            index = i;
        }
    }
    const auto fold = [&](unsigned long long ot, uint32_t oi, uint32_t oc) {
        count += oc;
        if (oi != 0xFFFFFFFFu && (index == 0xFFFFFFFFu || ot < total || (ot == total && oi < index))) {
            total = ot;
            index = oi;
        }
    };
    for (int m = 1; m < 64; m <<= 1) fold(__shfl_xor(total, m), static_cast<uint32_t>(__shfl_xor(static_cast<int>(index), m)),
                                          static_cast<uint32_t>(__shfl_xor(static_cast<int>(count), m)));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_total[wave] = total;
        s_index[wave] = index;
        s_count[wave] = count;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CM_TRAJ_BEST_BLOCK / 64; ++w) fold(s_total[w], s_index[w], s_count[w]);
        info[0] = index;
        info[1] = count;
    }
}

bool traj_ok(const CmTrajDev& g) {
    return g.nx >= 1 && g.ny >= 1 && g.nv >= 1 && g.nw >= 1 && static_cast<uint64_t>(g.nv) * g.nw <= CM_TRAJ_MAX_SAMPLES_DEV && g.n_steps >= 1 &&
           g.n_steps <= CM_TRAJ_MAX_STEPS_DEV && g.n_foot >= 1 && g.n_foot <= CM_TRAJ_MAX_FOOT_DEV;
}

}  // namespace

void cmk_traj_roll(hipStream_t s, const unsigned char* cost, const uint32_t* pot, const CmTrajDev& g, const float* steps, const uint32_t* dh,
                   const float* dirs, const float* foot, CmTrajScoreDev* out) {
    if (!traj_ok(g)) return;
    const uint32_t n = g.nv * g.nw;
    hipLaunchKernelGGL(k_traj_roll, dim3((n + CM_TRAJ_WAVES - 1) / CM_TRAJ_WAVES), dim3(CM_TRAJ_WAVES * 64), 0, s, cost, pot, g, steps, dh,
                       reinterpret_cast<const float2*>(dirs), reinterpret_cast<const float2*>(foot), out);
}

void cmk_traj_best(hipStream_t s, const CmTrajScoreDev* scores, uint32_t n, uint32_t* info) {
    if (n == 0 || n > CM_TRAJ_MAX_SAMPLES_DEV) return;
    hipLaunchKernelGGL(k_traj_best, dim3(1), dim3(CM_TRAJ_BEST_BLOCK), 0, s, scores, n, info);
}
