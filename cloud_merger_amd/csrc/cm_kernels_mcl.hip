// cm_kernels_mcl.hip — the localisation layer behind the cost layer: a particle filter of the vehicle's pose against the
// likelihood field of the occupancy map (amcl's Monte Carlo localisation against a likelihood field), for gfx950 (wave64).
//
// Computed on request (cm_map_mcl_init_pose / _init_uniform / _predict / _update) from the frame's clouds in place exactly as
// k_match_mark reads them, the map's info and image and the cost layer's dist2; it writes buffers of the localisation layer
// only (the semantics are in include/cloudmerge.h). Scores and weights are integers, positions are fp32 with
// every operation rounded on its own (the _rn intrinsics: nothing contracts), the noise is an integer sum of fields of a
// counter-based draw (cm_mcl_math.hpp) and the resampling is integer systematic resampling, so neither the lanes, the order of
// the atomics nor the grid can show in a table.
//
//   k_mcl_mark       one workgroup per tile of 4096 raw points: k_match_mark's front end and masks without candidates. A
//                    counted point's body cell (floorf(x * inv), floorf(y * inv)) within range_cells sets its bit in the body
//                    bitmap, side x side bits in (b_y, b_x) order, the atomicOr skipped where a plain read shows the bit.
//   k_mcl_free_bits  one thread per word: the bitmap of the window cells whose image byte is 0.
//   k_mcl_count, k_mcl_scan, k_mcl_emit   the ordered compaction of a bitmap by a popcount scan: per CM_MCL_BLOCK words their
//                    set bits, the exclusive scan of those counts in one workgroup, which also picks the stride
//                    max(1, ceil(n / max_out)), then every set bit's rank from its block's base and a scan inside the block;
//                    rank r with r % stride == 0 writes its bit index to list[r / stride]. It serves the beams (with their
//                    stride) and the free cells of cm_map_mcl_init_uniform (stride 1).
//   k_mcl_init_pose, k_mcl_init_uniform, k_mcl_predict   one thread per particle.
//   k_mcl_score      one wave per particle, CM_MCL_WAVES waves per workgroup, the grid sized to the device with a stride over
//                    the particles. The workgroup stages the beams once in LDS as float2 (the centre of a list entry's body
//                    cell). A lane takes beams lane, lane + 64, ... and issues the field loads of CM_MCL_BEAM_BATCH of them
//                    before it adds any: the loads do not depend on one another. An integer wave reduction; lane 0 stores S_p
//                    and the new acc_p by plain vector stores.
//   k_mcl_beam       k_mcl_score's shape for the beam model: a beam is a ray on the map's integer line from the
//                    particle's cell to the beam's end cell and over_cells past it, walked by cm_cast_math.hpp's reach forms (by
//                    the skip bytes of cmk_cast_steps, or cell by cell through the image under CM_MCL_BEAM_PLAIN), and scored
//                    at once by a table byte from LDS; two independent walks per lane in flight (one or four by a measurement's switch). The six outcome
//                    counts are summed per lane, per wave by shuffles, per workgroup in LDS, then one 64-bit integer atomicAdd
//                    per non-zero count and workgroup.
//   k_mcl_best       one workgroup: the largest acc, ties to the lowest index; the best particle's x, y, h.
//   k_mcl_weights    one thread per particle: W_p through cm_exp_neg (cm_ndt_math.hpp with the _rn macros), and the six sums
//                    of step 9 combined per wave by shuffles and per workgroup in LDS before one 64-bit integer atomicAdd per
//                    sum and workgroup.
//   k_mcl_spread     the same shape for the three spread sums about the integer means.
//   k_mcl_cum        one workgroup: the inclusive prefix sum of W in particle order, and the resampling decision, taken here
//                    on the device from the sums: n_eff in double with the host's three operations.
//   k_mcl_gather     one thread per new particle: a binary search in the prefix sums, the copy into the second buffer; without
//                    resampling it sets the parents of the first. Under the hypotheses mode the last n_inject new particles are
//                    k_mcl_init_uniform's body over the mode's free list instead.
// The hypotheses mode (cm_map_mcl_hyp_configure), between k_mcl_spread and k_mcl_cum:
//   k_mcl_hyp_bins   one lane per particle: its bin's 64-bit key goes into an open-addressing table by atomicCAS (at most a
//                    quarter full); the lane that took a free slot makes it a root; the particle keeps its slot.
//   k_mcl_hyp_link   one lane per slot: the 13 neighbour keys of one half-space are looked up and united with cm_search.hpp's
//                    lock-free union-find (the frontier layer's), headings wrapping.
//   k_mcl_hyp_roots, k_mcl_hyp_flatten   a root takes a component number (one atomic per workgroup) and clears its record;
//                    then every slot takes its root's number and its key falls into the record's label (atomicMin).
//   k_mcl_hyp_sums, k_mcl_hyp_spread   one lane per particle: the component's n, five weighted sums and top (one 64-bit
//                    atomicMax of W << 32 | ~p), then the spread sums about its integer mean. Lanes of a wave that share a
//                    component reduce among themselves and one lane sends the atomics (wave_by_component).
//   k_mcl_hyp_pick   one workgroup: the first max_hyp records by (sum_w descending, label ascending).
//   k_mcl_hyp_recover   one thread: the average score, its slow and fast averages and the injection count, in double with
//                    every operation rounded on its own.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

// the rounded fp64 operations of cm_ndt_math.hpp, as cm_kernels_ndt.hip sets them
#define CM_NDT_FN __device__ __forceinline__
#define CM_NDT_MUL(a, b) __dmul_rn((a), (b))
#define CM_NDT_ADD(a, b) __dadd_rn((a), (b))
#define CM_NDT_SUB(a, b) __dsub_rn((a), (b))
#include "cm_ndt_math.hpp"
#define CM_MCL_FN __device__ __forceinline__
#include "cm_mcl_math.hpp"
// the line and the walks of cm_cast_math.hpp, as cm_kernels_cast.hip sets them
#define CM_CAST_FN __device__ __forceinline__
#define CM_CAST_RCP(d) __builtin_amdgcn_rcpf(d)
#include "cm_cast_math.hpp"

namespace {

typedef unsigned long long u64;
constexpr double kTurn = 4294967296.0 / 6.283185307179586;     // K: binary angle units per radian (the rollout layer's)

// The rollout layer's step 2: the table entry of a heading.
__device__ __forceinline__ uint32_t heading_entry(uint32_t h) { return ((h + 0x80000u) >> 20) & (CM_TRAJ_HEADINGS_DEV - 1u); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m));
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// Inclusive scan of v over the WAVES * 64 threads of a workgroup (all of them call it); s_w: WAVES words of LDS.
template <int WAVES, class T>
__device__ __forceinline__ T block_scan(T v, T* s_w) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= static_cast<uint32_t>(d)) v += o;
    }
    __syncthreads();                                   // (s_w may still be read from an earlier call)
    if (lane == 63u) s_w[wave] = v;
    __syncthreads();
    T before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += s_w[w];
    return v + before;
}

// ---- the front end and the ordered compaction ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_BLOCK) void k_mcl_mark(const CmFrameDev* __restrict__ fd, CmMclDev g, const unsigned char* __restrict__ keep,
                                                       uint32_t* __restrict__ bits) {
    const uint32_t tile = blockIdx.x;
    const uint32_t s = sensor_of_tile(fd, tile);
    const CmSensorDev& sd = fd->s[s];
    const uint32_t first = tile * CM_TILE - sd.base;
    const int R = static_cast<int>(g.range);
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = first + r * CM_BLOCK + threadIdx.x;
        if (i >= sd.n) continue;
        const Pt p = load_point(sd.data, sd.layout, sd.point_step, sd.off_x, sd.off_y, sd.off_z, sd.off_i, i);
        float x, y, z;
        xf_point(sd.m, p, x, y, z);
        if (!point_valid(x, y, z, fd->crop_enable, fd->crop_min, fd->crop_max)) continue;
        const uint32_t slot = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        if (keep && !keep[slot]) continue;             // (a counted point of A)
        if (!(g.z_min <= z && z <= g.z_max)) continue;
        int bx, by;
        if (!world_axis(x, g.inv, &bx) || !world_axis(y, g.inv, &by)) continue;
        if (bx < -R || bx > R || by < -R || by > R) continue;
        const uint32_t cell = static_cast<uint32_t>(bx + R) + static_cast<uint32_t>(by + R) * g.side;      // (< side * side)
        const uint32_t b = 1u << (cell & 31u);
        uint32_t* w = bits + (cell >> 5);
        if (!(ld_agent(w) & b)) atomicOr(w, b);
    }
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_free_bits(const signed char* __restrict__ image, uint32_t n_cells, uint32_t n_words,
                                                                uint32_t* __restrict__ bits) {
    const uint32_t w = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (w >= n_words) return;
    uint32_t m = 0u;
    for (uint32_t b = 0; b < 32u; ++b) {
        const uint32_t c = w * 32u + b;
        if (c < n_cells && image[c] == 0) m |= 1u << b;
    }
    bits[w] = m;
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_count(const uint32_t* __restrict__ bits, uint32_t n_words, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_w[CM_MCL_BLOCK / 64];
    const uint32_t w = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    const uint32_t v = wave_sum(w < n_words ? static_cast<uint32_t>(__popc(bits[w])) : 0u);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0u;
        for (uint32_t k = 0; k < CM_MCL_BLOCK / 64; ++k) t += s_w[k];
        counts[blockIdx.x] = t;
    }
}

// n_blocks <= CM_MCL_ONE_BLOCK: one count per thread.
__global__ __launch_bounds__(CM_MCL_ONE_BLOCK) void k_mcl_scan(uint32_t* __restrict__ counts, uint32_t n_blocks, uint32_t max_out, u64* __restrict__ words) {
    __shared__ uint32_t s_w[CM_MCL_ONE_BLOCK / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t v = t < n_blocks ? counts[t] : 0u;
    const uint32_t incl = block_scan<CM_MCL_ONE_BLOCK / 64>(v, s_w);
    if (t < n_blocks) counts[t] = incl - v;
    if (t == CM_MCL_ONE_BLOCK - 1u) {
        const uint32_t n = incl;
        const uint32_t stride = n > max_out ? (n + max_out - 1u) / max_out : 1u;
        words[CM_MCL_W_NCELLS] = n;
        words[CM_MCL_W_STRIDE] = stride;
        words[CM_MCL_W_NBEAMS] = (n + stride - 1u) / stride;
    }
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_emit(const uint32_t* __restrict__ bits, uint32_t n_words, const uint32_t* __restrict__ counts,
                                                           const u64* __restrict__ words, uint32_t max_out, uint32_t* __restrict__ list) {
    __shared__ uint32_t s_w[CM_MCL_BLOCK / 64];
    const uint32_t w = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    uint32_t m = w < n_words ? bits[w] : 0u;
    const uint32_t v = static_cast<uint32_t>(__popc(m));
    uint32_t r = counts[blockIdx.x] + block_scan<CM_MCL_BLOCK / 64>(v, s_w) - v;
    const uint32_t stride = static_cast<uint32_t>(words[CM_MCL_W_STRIDE]);
    while (m) {
        const uint32_t b = static_cast<uint32_t>(__ffs(static_cast<int>(m))) - 1u;
        m &= m - 1u;
        if (r % stride == 0u) {
            const uint32_t o = r / stride;
            if (o < max_out) list[o] = w * 32u + b;
        }
        ++r;
    }
}

// ---- the particles -------------------------------------------------------------------------------------------------------------
// The low 32 bits of (int64)rint(((double)yaw + (double)nz) * K): steps 3 and 5.
__device__ __forceinline__ uint32_t turn_of(double yaw, float nz) {
    return static_cast<uint32_t>(static_cast<long long>(rint(__dmul_rn(__dadd_rn(yaw, static_cast<double>(nz)), kTurn))));
}
__device__ __forceinline__ float noise_of(u64 base, uint32_t p, uint32_t i, float sc) {
    return __fmul_rn(static_cast<float>(cm_mcl_noise(cm_mcl_draw(base, p, i))), sc);
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_init_pose(CmMclMoveDev m, uint32_t n, CmMclParticleDev* __restrict__ parts) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (p >= n) return;
    CmMclParticleDev q;
    q.x = __fadd_rn(m.a, noise_of(m.base, p, 0u, m.sc_a));
    q.y = __fadd_rn(m.b, noise_of(m.base, p, 1u, m.sc_b));
    q.h = turn_of(m.yaw, noise_of(m.base, p, 2u, m.sc_yaw));
    q.parent = p;
    q.acc = 0ull;
    parts[p] = q;
}

// Step 4 for particle p over the n_free >= 1 free cells of list: its x, y, h, parent = p and acc = 0.
__device__ __forceinline__ CmMclParticleDev uniform_particle(const CmMclDev& g, u64 base, uint32_t p, const uint32_t* __restrict__ list, u64 n_free) {
    const uint32_t c = list[__umul64hi(cm_mcl_draw(base, p, 0u), n_free)];
    const int ix = static_cast<int>(c % g.nx), iy = static_cast<int>(c / g.nx);
    const float ux = __fmul_rn(static_cast<float>(cm_mcl_draw(base, p, 1u) >> 40), 0x1p-24f);
    const float uy = __fmul_rn(static_cast<float>(cm_mcl_draw(base, p, 2u) >> 40), 0x1p-24f);
    CmMclParticleDev q;
    q.x = __fmul_rn(__fadd_rn(static_cast<float>(g.ax + ix), ux), g.cell);
    q.y = __fmul_rn(__fadd_rn(static_cast<float>(g.ay + iy), uy), g.cell);
    q.h = static_cast<uint32_t>(cm_mcl_draw(base, p, 3u) >> 32);
    q.parent = p;
    q.acc = 0ull;
    return q;
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_init_uniform(CmMclDev g, u64 base, const uint32_t* __restrict__ list, const u64* __restrict__ words,
                                                                   CmMclParticleDev* __restrict__ parts) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (p >= g.n) return;
    parts[p] = uniform_particle(g, base, p, list, words[CM_MCL_W_NCELLS]);      // (>= 1 free cell: the host looked)
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_predict(CmMclMoveDev m, uint32_t n, const float2* __restrict__ dirs,
                                                              CmMclParticleDev* __restrict__ parts) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (p >= n) return;
    CmMclParticleDev q = parts[p];
    const float2 e = dirs[heading_entry(q.h)];
    const float a = __fadd_rn(m.a, noise_of(m.base, p, 0u, m.sc_a));
    const float b = __fadd_rn(m.b, noise_of(m.base, p, 1u, m.sc_b));
    q.x = __fsub_rn(__fadd_rn(q.x, __fmul_rn(e.x, a)), __fmul_rn(e.y, b));
    q.y = __fadd_rn(__fadd_rn(q.y, __fmul_rn(e.y, a)), __fmul_rn(e.x, b));
    q.h += turn_of(m.yaw, noise_of(m.base, p, 2u, m.sc_yaw));
    parts[p] = q;
}

// ---- the score -----------------------------------------------------------------------------------------------------------------
// Dynamic LDS: g.max_beams float2.
__global__ __launch_bounds__(CM_MCL_WAVES * 64) void k_mcl_score(const unsigned char* __restrict__ field, CmMclDev g, const uint32_t* __restrict__ list,
                                                                 const u64* __restrict__ words, const float2* __restrict__ dirs,
                                                                 CmMclParticleDev* __restrict__ parts, CmMclWeightDev* __restrict__ wts) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    float2* const s_beam = reinterpret_cast<float2*>(s_mem);
    const uint32_t n_words = static_cast<uint32_t>(words[CM_MCL_W_NBEAMS]);
    const uint32_t n_beams = n_words < g.max_beams ? n_words : g.max_beams;       // (it is at most max_beams: the room of s_beam)
    for (uint32_t i = threadIdx.x; i < n_beams; i += CM_MCL_WAVES * 64) {
        const uint32_t c = list[i];
        const int bx = static_cast<int>(c % g.side) - static_cast<int>(g.range), by = static_cast<int>(c / g.side) - static_cast<int>(g.range);
        s_beam[i] = make_float2(__fmul_rn(__fadd_rn(static_cast<float>(bx), 0.5f), g.cell), __fmul_rn(__fadd_rn(static_cast<float>(by), 0.5f), g.cell));
    }
    __syncthreads();                                   // (the only barrier: the waves part ways below)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    for (uint32_t p = blockIdx.x * CM_MCL_WAVES + wave; p < g.n; p += gridDim.x * CM_MCL_WAVES) {
        const CmMclParticleDev q = parts[p];
        const float2 e = dirs[heading_entry(q.h)];
        uint32_t sum = 0u;
        for (uint32_t b0 = lane; b0 < n_beams; b0 += 64u * CM_MCL_BEAM_BATCH) {
            uint32_t v[CM_MCL_BEAM_BATCH];
#pragma unroll
            for (int k = 0; k < CM_MCL_BEAM_BATCH; ++k) {
                const uint32_t b = b0 + 64u * static_cast<uint32_t>(k);
                v[k] = 0u;
                if (b < n_beams) {
                    const float2 f = s_beam[b];
                    const float wx = __fsub_rn(__fadd_rn(q.x, __fmul_rn(e.x, f.x)), __fmul_rn(e.y, f.y));
                    const float wy = __fadd_rn(__fadd_rn(q.y, __fmul_rn(e.y, f.x)), __fmul_rn(e.x, f.y));
                    int gx = 0, gy = 0;
                    const bool exists = world_axis(wx, g.inv, &gx) & world_axis(wy, g.inv, &gy);
                    // (|gx| < 2^30 and |ax| < 2^30 + 2^21: the wrapped difference is below nx only where the true one is)
                    const uint32_t ix = static_cast<uint32_t>(gx) - static_cast<uint32_t>(g.ax), iy = static_cast<uint32_t>(gy) - static_cast<uint32_t>(g.ay);
                    if (exists && ix < g.nx && iy < g.ny) v[k] = field[iy * g.nx + ix];
                }
            }
#pragma unroll
            for (int k = 0; k < CM_MCL_BEAM_BATCH; ++k) sum += v[k];
        }
        sum = wave_sum(sum);
        if (lane == 0u) {
            wts[p].score = sum;
            parts[p].acc = q.acc + sum;
        }
    }
}

// ---- the beam score ------------------------------------------------------------------------------------------------------------
// Step 7 under the beam model (cm_map_mcl_beam_configure): k_mcl_score's shape, but every beam is a ray from the particle's
// cell to the beam's end cell and bm.over steps past it, walked at once and turned into a table byte; no per-ray record.
// Dynamic LDS: g.max_beams float2, then CM_MCL_WAVES * CM_MCL_BEAM_COUNTS count words, then the 2 * over + 3 table bytes.
// A lane walks WALKS rays at a time (beams b, b + 64, ...): their byte loads do not depend on one another.
template <int WALKS>
__global__ __launch_bounds__(CM_MCL_WAVES * 64) void k_mcl_beam(const signed char* __restrict__ image, const unsigned char* __restrict__ steps,
                                                                const unsigned char* __restrict__ table, CmMclDev g, CmMclBeamDev bm,
                                                                const uint32_t* __restrict__ list, const u64* __restrict__ words,
                                                                const float2* __restrict__ dirs, CmMclParticleDev* __restrict__ parts,
                                                                CmMclWeightDev* __restrict__ wts, u64* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    float2* const s_beam = reinterpret_cast<float2*>(s_mem);
    uint32_t(*const s_cnt)[CM_MCL_BEAM_COUNTS] = reinterpret_cast<uint32_t(*)[CM_MCL_BEAM_COUNTS]>(s_mem + static_cast<size_t>(g.max_beams) * sizeof(float2));
    unsigned char* const s_tab = reinterpret_cast<unsigned char*>(s_cnt + CM_MCL_WAVES);
    const uint32_t n_words = static_cast<uint32_t>(words[CM_MCL_W_NBEAMS]);
    const uint32_t n_beams = n_words < g.max_beams ? n_words : g.max_beams;       // (it is at most max_beams: the room of s_beam)
    const uint32_t E = bm.over;                        // (<= CM_CAST_MAX_OVER: the launcher looked)
    for (uint32_t i = threadIdx.x; i < n_beams; i += CM_MCL_WAVES * 64) {
        const uint32_t c = list[i];
        const int bx = static_cast<int>(c % g.side) - static_cast<int>(g.range), by = static_cast<int>(c / g.side) - static_cast<int>(g.range);
        s_beam[i] = make_float2(__fmul_rn(__fadd_rn(static_cast<float>(bx), 0.5f), g.cell), __fmul_rn(__fadd_rn(static_cast<float>(by), 0.5f), g.cell));
    }
    for (uint32_t i = threadIdx.x; i < 2u * E + 3u; i += CM_MCL_WAVES * 64) s_tab[i] = table[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    uint32_t cnt[CM_MCL_BEAM_COUNTS] = {0u, 0u, 0u, 0u, 0u, 0u};       // early, at, late, beyond, off, skipped (a lane has below 2^23 rays)
    for (uint32_t p = blockIdx.x * CM_MCL_WAVES + wave; p < g.n; p += gridDim.x * CM_MCL_WAVES) {
        const CmMclParticleDev q = parts[p];
        const float2 e = dirs[heading_entry(q.h)];
        int px = 0, py = 0;
        const bool there = world_axis(q.x, g.inv, &px) & world_axis(q.y, g.inv, &py);
        // (|px| < 2^30 and |ax| < 2^30 + 2^21: the wrapped difference is below nx only where the true one is)
        const uint32_t ox = static_cast<uint32_t>(px) - static_cast<uint32_t>(g.ax), oy = static_cast<uint32_t>(py) - static_cast<uint32_t>(g.ay);
        const bool origin = there && ox < g.nx && oy < g.ny;
        uint32_t sum = 0u;
        for (uint32_t b0 = lane; b0 < n_beams; b0 += 64u * WALKS) {
            CmCastLine ln[WALKS];
            bool live[WALKS];
            uint32_t out[WALKS];
#pragma unroll
            for (int k = 0; k < WALKS; ++k) {
                const uint32_t b = b0 + 64u * static_cast<uint32_t>(k);
                live[k] = false;
                out[k] = 4u << 16;                     // no beam here
                ln[k] = CmCastLine{1, 1, 0u, 1u, 0.5f, true};
                if (b >= n_beams) continue;
                out[k] = 3u << 16;                     // skipped
                if (!origin) continue;
                const float2 f = s_beam[b];
                const float wx = __fsub_rn(__fadd_rn(q.x, __fmul_rn(e.x, f.x)), __fmul_rn(e.y, f.y));
                const float wy = __fadd_rn(__fadd_rn(q.y, __fmul_rn(e.y, f.x)), __fmul_rn(e.x, f.y));
                int gx = 0, gy = 0;
                if (!(world_axis(wx, g.inv, &gx) & world_axis(wy, g.inv, &gy))) continue;
                const long long dx = static_cast<long long>(gx) - static_cast<long long>(px), dy = static_cast<long long>(gy) - static_cast<long long>(py);
                const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
                const long long L = adx > ady ? adx : ady;
                if (L > static_cast<long long>(CM_CAST_MAX_D)) continue;          // (sharpened in the header: skipped)
                if (L == 0) {                          // only the origin cell is looked at: a hit at 0 or beyond
                    out[k] = image[oy * g.nx + ox] == 100 ? (1u << 16) : 0u;
                    continue;
                }
                ln[k] = cm_cast_line(static_cast<int32_t>(dx), static_cast<int32_t>(dy));
                live[k] = true;
            }
            if (bm.plain) cm_cast_reach_plain_n<WALKS>(ln, live, E, ox, oy, g.nx, g.ny, image, out);
            else cm_cast_reach_skip_n<WALKS>(ln, live, E, ox, oy, g.nx, g.ny, steps, out);
#pragma unroll
            for (int k = 0; k < WALKS; ++k) {
                const uint32_t status = out[k] >> 16;
                if (status == 4u) continue;
                if (status == 3u) {
                    ++cnt[5];
                    continue;
                }
                uint32_t idx;
                if (status == 1u) {
                    const int32_t d = static_cast<int32_t>(out[k] & 0xFFFFu) - static_cast<int32_t>(live[k] ? ln[k].L : 0u);
                    const int32_t ee = d < -static_cast<int32_t>(E) ? -static_cast<int32_t>(E) : d;
                    idx = static_cast<uint32_t>(ee + static_cast<int32_t>(E));
                    cnt[0] += ee < 0;
                    cnt[1] += ee == 0;
                    cnt[2] += ee > 0;
                } else if (status == 0u) {
                    idx = 2u * E + 1u;
                    ++cnt[3];
                } else {
                    idx = 2u * E + 2u;
                    ++cnt[4];
                }
                sum += s_tab[idx];
            }
        }
        sum = wave_sum(sum);
        if (lane == 0u) {
            wts[p].score = sum;
            parts[p].acc = q.acc + sum;
        }
    }
#pragma unroll
    for (int k = 0; k < CM_MCL_BEAM_COUNTS; ++k) cnt[k] = wave_sum(cnt[k]);       // (a wave has below 2^29 rays)
    if (lane == 0u)
        for (int k = 0; k < CM_MCL_BEAM_COUNTS; ++k) s_cnt[wave][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < CM_MCL_BEAM_COUNTS) {
        u64 t = 0ull;
        for (uint32_t w = 0; w < CM_MCL_WAVES; ++w) t += s_cnt[w][threadIdx.x];
        if (t) atomicAdd(counts + threadIdx.x, t);     // (integers: the order cannot show)
    }
}

__global__ __launch_bounds__(CM_MCL_ONE_BLOCK) void k_mcl_best(const CmMclParticleDev* __restrict__ parts, uint32_t n, u64* __restrict__ words) {
    __shared__ u64 s_acc[CM_MCL_ONE_BLOCK / 64];
    __shared__ uint32_t s_index[CM_MCL_ONE_BLOCK / 64];
    u64 acc = 0ull;
    uint32_t index = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < n; i += CM_MCL_ONE_BLOCK) {        // (ascending i: a tie keeps the lower index)
        const u64 v = parts[i].acc;
        if (index == 0xFFFFFFFFu || v > acc) {
            acc = v;
            index = i;
        }
    }
    const auto fold = [&](u64 oa, uint32_t oi) {
        if (oi != 0xFFFFFFFFu && (index == 0xFFFFFFFFu || oa > acc || (oa == acc && oi < index))) {
            acc = oa;
            index = oi;
        }
    };
    for (int m = 1; m < 64; m <<= 1) fold(__shfl_xor(acc, m), static_cast<uint32_t>(__shfl_xor(static_cast<int>(index), m)));
    if ((threadIdx.x & 63u) == 0u) {
        s_acc[threadIdx.x >> 6] = acc;
        s_index[threadIdx.x >> 6] = index;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CM_MCL_ONE_BLOCK / 64; ++w) fold(s_acc[w], s_index[w]);
        const CmMclParticleDev q = parts[index];       // (n >= 1: there is one)
        words[CM_MCL_W_AMAX] = acc;
        words[CM_MCL_W_BEST] = index;
        words[CM_MCL_W_BEST_X] = __builtin_bit_cast(uint32_t, q.x);
        words[CM_MCL_W_BEST_Y] = __builtin_bit_cast(uint32_t, q.y);
        words[CM_MCL_W_BEST_H] = q.h;
    }
}

// Step 9's q(v): clamp(llrint(v * 1024), -2^30, 2^30), 0 for a v that is not finite. The clamp comes first, in double: the
// limits are integers and rounding is monotone, so the result is the same and no conversion overflows.
__device__ __forceinline__ long long quant_of(float v) {
    if (!finite_f32(v)) return 0;
    double x = __dmul_rn(static_cast<double>(v), 1024.0);
    x = x < -1073741824.0 ? -1073741824.0 : x > 1073741824.0 ? 1073741824.0 : x;
    return __double2ll_rn(x);
}

// floor(a / b) for 0 < b <= 2^32.
__device__ __forceinline__ long long floor_div(long long a, u64 b) {
    const long long d = static_cast<long long>(b);
    long long q = a / d;
    if (a % d < 0) --q;
    return q;
}

// K sums of a workgroup of CM_MCL_BLOCK threads into words[first ...]: shuffles inside a wave, the wave sums through LDS, one
// atomicAdd per non-zero sum (integers: the order cannot show).
template <int K>
__device__ __forceinline__ void block_add(u64 (&v)[K], u64* words, const int (&slot)[K]) {
    __shared__ u64 s_sum[CM_MCL_BLOCK / 64][K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < K; ++k) s_sum[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < static_cast<uint32_t>(K)) {
        u64 t = 0ull;
        for (uint32_t w = 0; w < CM_MCL_BLOCK / 64; ++w) t += s_sum[w][threadIdx.x];
        if (t) atomicAdd(words + slot[threadIdx.x], t);
    }
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_weights(const CmMclParticleDev* __restrict__ parts, uint32_t n, double beta,
                                                              const float2* __restrict__ dirs, CmMclWeightDev* __restrict__ wts, u64* __restrict__ words) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    u64 v[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (p < n) {
        const CmMclParticleDev q = parts[p];
        const u64 d = words[CM_MCL_W_AMAX] - q.acc;
        const u64 w = static_cast<u64>(floor(__dmul_rn(65536.0, cm_exp_neg(__dmul_rn(__ull2double_rn(d), beta)))));
        wts[p].weight = static_cast<uint32_t>(w);
        const float2 e = dirs[heading_entry(q.h)];
        const long long ci = static_cast<long long>(rintf(__fmul_rn(e.x, 32768.0f))), si = static_cast<long long>(rintf(__fmul_rn(e.y, 32768.0f)));
        const long long sw = static_cast<long long>(w);
        v[0] = w;
        v[1] = w * w;
        v[2] = static_cast<u64>(sw * quant_of(q.x));   // (signed sums wrap as two's complement: the total is exact, header)
        v[3] = static_cast<u64>(sw * quant_of(q.y));
        v[4] = static_cast<u64>(sw * ci);
        v[5] = static_cast<u64>(sw * si);
    }
    const int slot[6] = {CM_MCL_W_SW, CM_MCL_W_SW2, CM_MCL_W_SWQX, CM_MCL_W_SWQY, CM_MCL_W_SWC, CM_MCL_W_SWS};
    block_add<6>(v, words, slot);
}

__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_spread(const CmMclParticleDev* __restrict__ parts, uint32_t n, const CmMclWeightDev* __restrict__ wts,
                                                             u64* __restrict__ words) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    u64 v[3] = {0ull, 0ull, 0ull};
    if (p < n) {
        const u64 sum_w = words[CM_MCL_W_SW];          // (>= 65536: the best particle's weight)
        const long long mx = floor_div(static_cast<long long>(words[CM_MCL_W_SWQX]), sum_w), my = floor_div(static_cast<long long>(words[CM_MCL_W_SWQY]), sum_w);
        const auto clamp16 = [](long long d) { return d < -32768 ? -32768ll : d > 32767 ? 32767ll : d; };
        const long long dx = clamp16(quant_of(parts[p].x) - mx), dy = clamp16(quant_of(parts[p].y) - my);
        const long long w = wts[p].weight;
        v[0] = static_cast<u64>(w * dx * dx);
        v[1] = static_cast<u64>(w * dy * dy);
        v[2] = static_cast<u64>(w * dx * dy);
    }
    const int slot[3] = {CM_MCL_W_SWDXX, CM_MCL_W_SWDYY, CM_MCL_W_SWDXY};
    block_add<3>(v, words, slot);
}

// ---- the hypotheses and the recovery (cm_map_mcl_hyp_configure) -------------------------------------------------
// Every output is a function of keys and integer sums: which slot a key lands in, which slot is a root and which number a
// component gets depend on the order of arrival and show nowhere.
__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int m = 1; m < 64; m <<= 1) {
        const u64 o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

constexpr long long kHypOff = 1ll << 24;               // |bx|, |by| <= 2^24: |q| <= 2^30 and bin_q >= 64

__device__ __forceinline__ u64 hyp_key(long long by, long long bx, uint32_t bh) {
    return (static_cast<u64>(by + kHypOff) << 34) | (static_cast<u64>(bx + kHypOff) << 8) | bh;
}
__device__ __forceinline__ uint32_t hyp_hash(u64 key, uint32_t cap_bits) { return static_cast<uint32_t>((key * 0x9E3779B97F4A7C15ull) >> (64u - cap_bits)); }

// H1: one lane per particle inserts its key; the lane whose compare-and-swap took a free slot makes it a tree of its own.
// The table is at most a quarter full, so a probe always ends.
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_hyp_bins(const CmMclParticleDev* __restrict__ parts, CmMclHypDev hy) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    const uint32_t mask = (1u << hy.cap_bits) - 1u;
    bool won = false;
    if (p < hy.n) {
        const CmMclParticleDev q = parts[p];
        const long long bx = floor_div(quant_of(q.x), hy.bin_q), by = floor_div(quant_of(q.y), hy.bin_q);
        const uint32_t bh = hy.heading_bits ? q.h >> (32u - hy.heading_bits) : 0u;
        const u64 key = hyp_key(by, bx, bh);
        uint32_t s = hyp_hash(key, hy.cap_bits);
        for (;;) {
            const u64 old = atomicCAS(hy.keys + s, CM_MCL_HYP_EMPTY, key);
            if (old == CM_MCL_HYP_EMPTY) {
                won = true;
                hy.parent[s] = s;
                break;
            }
            if (old == key) break;
            s = (s + 1u) & mask;
        }
        hy.slot[p] = s;
    }
    const u64 m = __ballot(won);
    if (m && (threadIdx.x & 63u) == 0u) atomicAdd(hy.words + CM_MCL_HW_NBINS, static_cast<u64>(__popcll(m)));
}

// H3: one lane per occupied slot looks up the 13 neighbour keys of one half-space ((dy, dx, dh) after (0, 0, 0) in that
// order; the other half is covered from the neighbour's side) and unites. Headings wrap modulo 2^heading_bits.
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_hyp_link(CmMclHypDev hy) {
    const uint32_t s = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    const uint32_t mask = (1u << hy.cap_bits) - 1u;
    if (s > mask) return;
    const u64 key = hy.keys[s];
    if (key == CM_MCL_HYP_EMPTY) return;
    const uint32_t hmask = (1u << hy.heading_bits) - 1u;
    const uint32_t bh = static_cast<uint32_t>(key & 0xFFu);
    const long long bx = static_cast<long long>((key >> 8) & 0x3FFFFFFull) - kHypOff, by = static_cast<long long>(key >> 34) - kHypOff;
    for (int dy = 0; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
            for (int dh = -1; dh <= 1; ++dh) {
                if (dy == 0 && (dx < 0 || (dx == 0 && dh <= 0))) continue;
                const long long ny = by + dy, nx = bx + dx;
                if (ny > kHypOff || nx > kHypOff || nx < -kHypOff) continue;   // (no particle has such a bin)
                const u64 nkey = hyp_key(ny, nx, (bh + static_cast<uint32_t>(dh)) & hmask);
                if (nkey == key) continue;
                uint32_t t = hyp_hash(nkey, hy.cap_bits);
                for (;;) {
                    const u64 k = hy.keys[t];
                    if (k == nkey) {
                        cm_uf_unite(hy.parent, s, t);
                        break;
                    }
                    if (k == CM_MCL_HYP_EMPTY) break;
                    t = (t + 1u) & mask;
                }
            }
}

// One lane per slot: a root takes the next component number (one atomic per workgroup) and clears its record.
__global__ __launch_bounds__(CM_MCL_ONE_BLOCK) void k_mcl_hyp_roots(CmMclHypDev hy) {
    __shared__ uint32_t s_w[CM_MCL_ONE_BLOCK / 64];
    __shared__ uint32_t s_base;
    const uint32_t s = blockIdx.x * CM_MCL_ONE_BLOCK + threadIdx.x;
    const uint32_t mask = (1u << hy.cap_bits) - 1u;
    const bool root = s <= mask && hy.keys[s] != CM_MCL_HYP_EMPTY && hy.parent[s] == s;
    const uint32_t incl = block_scan<CM_MCL_ONE_BLOCK / 64>(root ? 1u : 0u, s_w);
    if (threadIdx.x == CM_MCL_ONE_BLOCK - 1u) s_base = incl ? static_cast<uint32_t>(atomicAdd(hy.words + CM_MCL_HW_NCOMP, static_cast<u64>(incl))) : 0u;
    __syncthreads();
    if (!root) return;
    const uint32_t c = s_base + incl - 1u;             // (< n: a component holds a particle)
    hy.comp[s] = c;
    CmMclHypRecDev r;
    r.label = CM_MCL_HYP_EMPTY;
    r.n = r.sum_w = r.sum_wqx = r.sum_wqy = r.sum_wc = r.sum_ws = r.top = r.sum_wdxx = r.sum_wdyy = r.sum_wdxy = 0ull;
    hy.rec[c] = r;
}

// One lane per occupied slot: its root's number becomes its own, and its key falls into the component's label.
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_hyp_flatten(CmMclHypDev hy) {
    const uint32_t s = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (s >= (1u << hy.cap_bits)) return;
    const u64 key = hy.keys[s];
    if (key == CM_MCL_HYP_EMPTY) return;
    const uint32_t r = cm_uf_find(hy.parent, s);
    const uint32_t c = hy.comp[r];                     // (written by k_mcl_hyp_roots; only roots are read here)
    if (r != s) hy.comp[s] = c;
    u64* const label = &hy.rec[c].label;
    if (key < __hip_atomic_load(label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(label, key);
}

// Lanes of a wave that share a component combine their K sums (and the largest `top`) before one of them calls issue(c,
// sums, top): in a converged belief every particle adds to one record. Per round the first lane still waiting names the
// component; a lane alone in its component issues its own values without a reduction. Every lane of the wave calls this.
template <int K, class F>
__device__ __forceinline__ void wave_by_component(bool active, uint32_t c, const u64 (&v)[K], u64 top, bool agg, F&& issue) {
    if (!agg) {
        if (active) issue(c, v, top);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    u64 left = __ballot(active);
    while (left) {                                     // (wave-uniform: at most one round per distinct component of the wave)
        const uint32_t lead = static_cast<uint32_t>(__ffsll(static_cast<long long>(left))) - 1u;
        const uint32_t c0 = static_cast<uint32_t>(__shfl(static_cast<int>(c), static_cast<int>(lead)));
        const bool same = active && c == c0;
        const u64 m = __ballot(same);
        if (__popcll(m) == 1) {
            if (lane == lead) issue(c, v, top);
        } else {
            u64 t[K];
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] = wave_sum(same ? v[k] : 0ull);
            const u64 tp = wave_max(same ? top : 0ull);
            if (lane == lead) issue(c0, t, tp);
        }
        if (same) active = false;
        left &= ~m;
    }
}

// H4: one lane per particle; n, the five weighted sums and top of its component, and the sum of the scores (R1).
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_hyp_sums(const CmMclParticleDev* __restrict__ parts, const CmMclWeightDev* __restrict__ wts,
                                                               const float2* __restrict__ dirs, CmMclHypDev hy) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    const bool in = p < hy.n;
    u64 v[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, top = 0ull, score = 0ull;
    uint32_t c = 0u;
    if (in) {
        const CmMclParticleDev q = parts[p];
        const CmMclWeightDev w = wts[p];
        const float2 e = dirs[heading_entry(q.h)];
        const long long ci = static_cast<long long>(rintf(__fmul_rn(e.x, 32768.0f))), si = static_cast<long long>(rintf(__fmul_rn(e.y, 32768.0f)));
        const long long sw = static_cast<long long>(w.weight);
        c = hy.comp[hy.slot[p]];
        v[0] = 1ull;
        v[1] = w.weight;
        v[2] = static_cast<u64>(sw * quant_of(q.x));   // (signed sums wrap as two's complement: the total is exact)
        v[3] = static_cast<u64>(sw * quant_of(q.y));
        v[4] = static_cast<u64>(sw * ci);
        v[5] = static_cast<u64>(sw * si);
        top = (static_cast<u64>(w.weight) << 32) | static_cast<u64>(~p);
        score = w.score;
    }
    score = wave_sum(score);
    if ((threadIdx.x & 63u) == 0u && score) atomicAdd(hy.words + CM_MCL_HW_SUMS, score);
    CmMclHypRecDev* const rec = hy.rec;
    wave_by_component<6>(in, c, v, top, hy.agg != 0u, [rec](uint32_t cc, const u64 (&t)[6], u64 tp) {
        CmMclHypRecDev* const r = rec + cc;
        atomicAdd(&r->n, t[0]);
        if (t[1]) atomicAdd(&r->sum_w, t[1]);
        if (t[2]) atomicAdd(&r->sum_wqx, t[2]);
        if (t[3]) atomicAdd(&r->sum_wqy, t[3]);
        if (t[4]) atomicAdd(&r->sum_wc, t[4]);
        if (t[5]) atomicAdd(&r->sum_ws, t[5]);
        atomicMax(&r->top, tp);
    });
}

// H4's spread sums about the component's integer mean.
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_hyp_spread(const CmMclParticleDev* __restrict__ parts, const CmMclWeightDev* __restrict__ wts,
                                                                 CmMclHypDev hy) {
    const uint32_t p = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    const bool in = p < hy.n;
    u64 v[3] = {0ull, 0ull, 0ull};
    uint32_t c = 0u;
    bool any = false;
    if (in) {
        c = hy.comp[hy.slot[p]];
        const long long w = wts[p].weight;
        const u64 sum_w = hy.rec[c].sum_w;
        if (w && sum_w) {                              // (a component of weight 0 has zero spread sums)
            const long long mx = floor_div(static_cast<long long>(hy.rec[c].sum_wqx), sum_w), my = floor_div(static_cast<long long>(hy.rec[c].sum_wqy), sum_w);
            const auto clamp16 = [](long long d) { return d < -32768 ? -32768ll : d > 32767 ? 32767ll : d; };
            const long long dx = clamp16(quant_of(parts[p].x) - mx), dy = clamp16(quant_of(parts[p].y) - my);
            v[0] = static_cast<u64>(w * dx * dx);
            v[1] = static_cast<u64>(w * dy * dy);
            v[2] = static_cast<u64>(w * dx * dy);
            any = (v[0] | v[1] | v[2]) != 0ull;
        }
    }
    CmMclHypRecDev* const rec = hy.rec;
    wave_by_component<3>(any, c, v, 0ull, hy.agg != 0u, [rec](uint32_t cc, const u64 (&t)[3], u64) {
        CmMclHypRecDev* const r = rec + cc;
        if (t[0]) atomicAdd(&r->sum_wdxx, t[0]);
        if (t[1]) atomicAdd(&r->sum_wdyy, t[1]);
        if (t[2]) atomicAdd(&r->sum_wdxy, t[2]);
    });
}

// H5: one workgroup picks the first min(n_components, max_hyp) records by sum_w descending, ties by label ascending (labels
// are distinct: the order is total). A thread keeps the best record of its strip that comes after the last one chosen; per
// round the workgroup reduces the threads' candidates and the thread that held the winner looks for its next.
__global__ __launch_bounds__(CM_MCL_ONE_BLOCK) void k_mcl_hyp_pick(CmMclHypDev hy) {
    __shared__ u64 s_sw[CM_MCL_ONE_BLOCK / 64], s_label[CM_MCL_ONE_BLOCK / 64];
    __shared__ uint32_t s_index[CM_MCL_ONE_BLOCK / 64];
    __shared__ u64 s_win_sw, s_win_label;
    __shared__ uint32_t s_win;
    constexpr uint32_t kNoRec = 0xFFFFFFFFu;
    const uint32_t n_comp = static_cast<uint32_t>(hy.words[CM_MCL_HW_NCOMP]);
    const uint32_t n_hyp = n_comp < hy.max_hyp ? n_comp : hy.max_hyp;
    const auto before = [](u64 sw_a, u64 label_a, u64 sw_b, u64 label_b) { return sw_a > sw_b || (sw_a == sw_b && label_a < label_b); };
    u64 sw = 0ull, label = 0ull;
    uint32_t index = kNoRec;
    // the best of the strip that comes after (last_sw, last_label); first: everything counts
    const auto rescan = [&](bool first, u64 last_sw, u64 last_label) {
        index = kNoRec;
        for (uint32_t i = threadIdx.x; i < n_comp; i += CM_MCL_ONE_BLOCK) {
            const u64 a = hy.rec[i].sum_w, l = hy.rec[i].label;
            if (!first && !before(last_sw, last_label, a, l)) continue;
            if (index == kNoRec || before(a, l, sw, label)) {
                sw = a;
                label = l;
                index = i;
            }
        }
    };
    rescan(true, 0ull, 0ull);
    for (uint32_t r = 0; r < n_hyp; ++r) {
        u64 bsw = sw, bl = label;
        uint32_t bi = index;
        const auto fold = [&](u64 osw, u64 ol, uint32_t oi) {
            if (oi != kNoRec && (bi == kNoRec || before(osw, ol, bsw, bl))) {
                bsw = osw;
                bl = ol;
                bi = oi;
            }
        };
        for (int m = 1; m < 64; m <<= 1) fold(__shfl_xor(bsw, m), __shfl_xor(bl, m), static_cast<uint32_t>(__shfl_xor(static_cast<int>(bi), m)));
        if ((threadIdx.x & 63u) == 0u) {
            s_sw[threadIdx.x >> 6] = bsw;
            s_label[threadIdx.x >> 6] = bl;
            s_index[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            for (uint32_t w = 1; w < CM_MCL_ONE_BLOCK / 64; ++w) fold(s_sw[w], s_label[w], s_index[w]);
            s_win = bi;                                // (r < n_comp: there is one)
            s_win_sw = bsw;
            s_win_label = bl;
            if (bi != kNoRec) hy.out[r] = hy.rec[bi];
        }
        __syncthreads();
        if (index != kNoRec && index == s_win) rescan(false, s_win_sw, s_win_label);
        __syncthreads();                               // (s_win is read before the next round writes it)
    }
    if (threadIdx.x == 0u) hy.words[CM_MCL_HW_NHYP] = n_hyp;
}

// R1 to R3 by one thread, in double with every operation rounded on its own, as k_mcl_cum computes n_eff.
__global__ void k_mcl_hyp_recover(CmMclHypDev hy, const u64* __restrict__ layer_words) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    u64* const hw = hy.words;
    const u64 n_beams = layer_words[CM_MCL_W_NBEAMS];
    double slow = __builtin_bit_cast(double, hw[CM_MCL_HW_STATE_SLOW]), fast = __builtin_bit_cast(double, hw[CM_MCL_HW_STATE_FAST]);
    double w_avg = 0.0, p = 0.0;
    uint32_t n_inject = 0u;
    if (n_beams) {
        const double den = __dmul_rn(__dmul_rn(static_cast<double>(hy.n), __ull2double_rn(n_beams)), 255.0);
        w_avg = __ddiv_rn(__ull2double_rn(hw[CM_MCL_HW_SUMS]), den);
        slow = slow == 0.0 ? w_avg : __dadd_rn(slow, __dmul_rn(hy.a_slow, __dsub_rn(w_avg, slow)));
        fast = fast == 0.0 ? w_avg : __dadd_rn(fast, __dmul_rn(hy.a_fast, __dsub_rn(w_avg, fast)));
        if (slow > 0.0 && fast < slow) p = __dsub_rn(1.0, __ddiv_rn(fast, slow));
        const uint32_t want = static_cast<uint32_t>(floor(__dmul_rn(p, static_cast<double>(hy.n))));       // (0 <= p <= 1: at most n)
        n_inject = want < hy.inject_max ? want : hy.inject_max;
        if (hw[CM_MCL_HW_NFREE] == 0ull) n_inject = 0u;                // (inject_max == 0 builds no list: n_free stays 0)
    }
    hw[CM_MCL_HW_STATE_SLOW] = __builtin_bit_cast(u64, slow);
    hw[CM_MCL_HW_STATE_FAST] = __builtin_bit_cast(u64, fast);
    hw[CM_MCL_HW_WAVG] = __builtin_bit_cast(u64, w_avg);
    hw[CM_MCL_HW_WSLOW] = __builtin_bit_cast(u64, slow);
    hw[CM_MCL_HW_WFAST] = __builtin_bit_cast(u64, fast);
    hw[CM_MCL_HW_PINJECT] = __builtin_bit_cast(u64, p);
    hw[CM_MCL_HW_NINJECT] = n_inject;
}

// ---- resampling ----------------------------------------------------------------------------------------------------------------
// hyp_words: the words of the hypotheses mode, or nullptr with the mode off; an injection (R4) resamples whatever n_eff says.
__global__ __launch_bounds__(CM_MCL_ONE_BLOCK) void k_mcl_cum(const CmMclWeightDev* __restrict__ wts, uint32_t n, double thr, uint32_t always,
                                                              u64* __restrict__ cum, u64* __restrict__ words, const u64* __restrict__ hyp_words) {
    __shared__ u64 s_w[CM_MCL_ONE_BLOCK / 64];
    const uint32_t per = (n + CM_MCL_ONE_BLOCK - 1u) / CM_MCL_ONE_BLOCK;
    const uint32_t lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    u64 own = 0ull;
    for (uint32_t p = lo; p < hi; ++p) own += wts[p].weight;
    u64 c = block_scan<CM_MCL_ONE_BLOCK / 64>(own, s_w) - own;
    for (uint32_t p = lo; p < hi; ++p) {
        c += wts[p].weight;
        cum[p] = c;
    }
    if (threadIdx.x == 0u) {
        const double sw = __ull2double_rn(words[CM_MCL_W_SW]), sw2 = __ull2double_rn(words[CM_MCL_W_SW2]);
        const double n_eff = __ddiv_rn(__dmul_rn(sw, sw), sw2);
        const bool inject = hyp_words && hyp_words[CM_MCL_HW_NINJECT] != 0ull;
        words[CM_MCL_W_RESAMPLED] = (always || n_eff < thr || inject) ? 1ull : 0ull;
    }
}

// hy.on: the last n_inject new particles (R4) are step 4 over hy.free_list with the update's own draws; the others share T.
__global__ __launch_bounds__(CM_MCL_BLOCK) void k_mcl_gather(CmMclParticleDev* __restrict__ src, CmMclParticleDev* __restrict__ dst, uint32_t n,
                                                             const u64* __restrict__ cum, u64 r_draw, const u64* __restrict__ words, CmMclDev g,
                                                             u64 base, CmMclHypDev hy) {
    const uint32_t j = blockIdx.x * CM_MCL_BLOCK + threadIdx.x;
    if (j >= n) return;
    if (!words[CM_MCL_W_RESAMPLED]) {
        src[j].parent = j;
        return;
    }
    const uint32_t n_inject = hy.on ? static_cast<uint32_t>(hy.words[CM_MCL_HW_NINJECT]) : 0u;       // (<= inject_max <= n - 1)
    const uint32_t m = n - n_inject;
    if (j >= m) {
        CmMclParticleDev o = uniform_particle(g, base, j, hy.free_list, hy.words[CM_MCL_HW_NFREE]);      // (n_free >= 1 where n_inject > 0)
        o.parent = 0xFFFFFFFFu;
        dst[j] = o;
        return;
    }
    const u64 T = words[CM_MCL_W_SW];
    const u64 t = (static_cast<u64>(j) * T + __umul64hi(r_draw, T)) / m;          // (< T = cum[n - 1]: there is a p)
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {                                  // the smallest p with cum[p] > t
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > t) hi = mid; else lo = mid + 1u;
    }
    const CmMclParticleDev q = src[lo];
    CmMclParticleDev o;
    o.x = q.x;
    o.y = q.y;
    o.h = q.h;
    o.parent = lo;
    o.acc = 0ull;
    dst[j] = o;
}

bool mcl_ok(const CmMclDev& g) {
    return g.nx >= 1 && g.ny >= 1 && static_cast<uint64_t>(g.nx) * g.ny <= (1u << 22) && g.n >= 1 && g.n <= CM_MCL_MAX_PARTICLES_DEV && g.max_beams >= 1 &&
           g.max_beams <= CM_MCL_MAX_BEAMS_DEV && g.range >= 1 && g.range <= CM_MCL_MAX_RANGE_DEV && g.side == 2u * g.range + 1u;
}

// The table holds four slots per particle at least (a probe ends), the records fit and an injection leaves a particle.
bool hyp_ok(const CmMclHypDev& hy, uint32_t n) {
    return hy.on && hy.n == n && n >= 1 && n <= CM_MCL_MAX_PARTICLES_DEV && hy.cap_bits >= 6 && hy.cap_bits <= 20 && (1ull << hy.cap_bits) >= 4ull * n &&
           hy.bin_q >= 64 && hy.bin_q <= (1u << 20) && hy.heading_bits <= 8 && hy.max_hyp >= 1 && hy.max_hyp <= CM_MCL_HYP_MAX_DEV && hy.inject_max < n &&
           hy.keys && hy.parent && hy.comp && hy.slot && hy.rec && hy.out && hy.words && (hy.inject_max == 0 || hy.free_list);
}

// Workgroups of k_mcl_score: enough to fill the device a few times over, never more than the particles need.
uint32_t score_grid(uint32_t n) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const uint32_t want = (n + CM_MCL_WAVES - 1) / CM_MCL_WAVES, cap = static_cast<uint32_t>(cus) * 8u;
    return want < cap ? want : cap;
}

}  // namespace

void cmk_mcl_mark(hipStream_t s, const CmFrameDev* fd, const CmMclDev& g, const unsigned char* keep, uint32_t* bits, uint32_t n_tiles) {
    if (!mcl_ok(g)) return;
    if (n_tiles) hipLaunchKernelGGL(k_mcl_mark, dim3(n_tiles), dim3(CM_BLOCK), 0, s, fd, g, keep, bits);
}

void cmk_mcl_free_bits(hipStream_t s, const void* image, uint32_t n_cells, uint32_t* bits) {
    const uint32_t n_words = (n_cells + 31u) / 32u;
    if (n_words)
        hipLaunchKernelGGL(k_mcl_free_bits, dim3((n_words + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, static_cast<const signed char*>(image),
                           n_cells, n_words, bits);
}

void cmk_mcl_compact(hipStream_t s, const uint32_t* bits, uint32_t n_words, uint32_t max_out, uint32_t* counts, uint32_t* list,
                     unsigned long long* words) {
    const uint32_t n_blocks = (n_words + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK;
    if (n_blocks == 0 || n_blocks > CM_MCL_ONE_BLOCK || max_out == 0) return;
    hipLaunchKernelGGL(k_mcl_count, dim3(n_blocks), dim3(CM_MCL_BLOCK), 0, s, bits, n_words, counts);
    hipLaunchKernelGGL(k_mcl_scan, dim3(1), dim3(CM_MCL_ONE_BLOCK), 0, s, counts, n_blocks, max_out, words);
    hipLaunchKernelGGL(k_mcl_emit, dim3(n_blocks), dim3(CM_MCL_BLOCK), 0, s, bits, n_words, counts, words, max_out, list);
}

void cmk_mcl_init_pose(hipStream_t s, const CmMclMoveDev& m, uint32_t n, CmMclParticleDev* parts) {
    if (n == 0 || n > CM_MCL_MAX_PARTICLES_DEV) return;
    hipLaunchKernelGGL(k_mcl_init_pose, dim3((n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, m, n, parts);
}

void cmk_mcl_init_uniform(hipStream_t s, const CmMclDev& g, unsigned long long base, const uint32_t* list, const unsigned long long* words,
                          CmMclParticleDev* parts) {
    if (!mcl_ok(g)) return;
    hipLaunchKernelGGL(k_mcl_init_uniform, dim3((g.n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, g, base, list, words, parts);
}

void cmk_mcl_predict(hipStream_t s, const CmMclMoveDev& m, uint32_t n, const float* dirs, CmMclParticleDev* parts) {
    if (n == 0 || n > CM_MCL_MAX_PARTICLES_DEV) return;
    hipLaunchKernelGGL(k_mcl_predict, dim3((n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, m, n, reinterpret_cast<const float2*>(dirs), parts);
}

void cmk_mcl_score(hipStream_t s, const unsigned char* field, const CmMclDev& g, const uint32_t* list, const unsigned long long* words,
                   const float* dirs, CmMclParticleDev* parts, CmMclWeightDev* wts) {
    if (!mcl_ok(g)) return;
    const size_t lds = static_cast<size_t>(g.max_beams) * sizeof(float2);          // (at most 64 KiB)
    hipLaunchKernelGGL(k_mcl_score, dim3(score_grid(g.n)), dim3(CM_MCL_WAVES * 64), lds, s, field, g, list, words, reinterpret_cast<const float2*>(dirs),
                       parts, wts);
}

void cmk_mcl_beam(hipStream_t s, const void* image, const unsigned char* steps, const unsigned char* table, const CmMclDev& g, const CmMclBeamDev& bm,
                  const uint32_t* list, const unsigned long long* words, const float* dirs, CmMclParticleDev* parts, CmMclWeightDev* wts,
                  unsigned long long* counts) {
    if (!mcl_ok(g) || bm.over > CM_CAST_MAX_OVER) return;
    const size_t lds = static_cast<size_t>(g.max_beams) * sizeof(float2) + CM_MCL_WAVES * CM_MCL_BEAM_COUNTS * sizeof(uint32_t) + ((2u * bm.over + 3u + 15u) & ~15u);
    // (up to 64 KiB of beams and 240 bytes behind them: above the default limit of dynamic LDS, below the CU's 160 KiB)
    const auto kernel = bm.walks == 1u ? k_mcl_beam<1> : bm.walks == 4u ? k_mcl_beam<4> : k_mcl_beam<2>;
    if (lds > 65536u && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess) return;
    hipLaunchKernelGGL(kernel, dim3(score_grid(g.n)), dim3(CM_MCL_WAVES * 64), lds, s, static_cast<const signed char*>(image), steps, table, g, bm, list, words,
                       reinterpret_cast<const float2*>(dirs), parts, wts, counts);
}

void cmk_mcl_best(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, unsigned long long* words) {
    if (n == 0 || n > CM_MCL_MAX_PARTICLES_DEV) return;
    hipLaunchKernelGGL(k_mcl_best, dim3(1), dim3(CM_MCL_ONE_BLOCK), 0, s, parts, n, words);
}

void cmk_mcl_weights(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, double beta, const float* dirs, CmMclWeightDev* wts,
                     unsigned long long* words) {
    if (n == 0 || n > CM_MCL_MAX_PARTICLES_DEV) return;
    hipLaunchKernelGGL(k_mcl_weights, dim3((n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, parts, n, beta,
                       reinterpret_cast<const float2*>(dirs), wts, words);
}

void cmk_mcl_spread(hipStream_t s, const CmMclParticleDev* parts, uint32_t n, const CmMclWeightDev* wts, unsigned long long* words) {
    if (n == 0 || n > CM_MCL_MAX_PARTICLES_DEV) return;
    hipLaunchKernelGGL(k_mcl_spread, dim3((n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, parts, n, wts, words);
}

void cmk_mcl_resample(hipStream_t s, CmMclParticleDev* src, CmMclParticleDev* dst, const CmMclDev& g, const CmMclWeightDev* wts, unsigned long long* cum,
                      unsigned long long base, unsigned long long r_draw, double thr, uint32_t always, unsigned long long* words, const CmMclHypDev& hy) {
    const uint32_t n = g.n;
    if (!mcl_ok(g) || (hy.on && !hyp_ok(hy, n))) return;
    hipLaunchKernelGGL(k_mcl_cum, dim3(1), dim3(CM_MCL_ONE_BLOCK), 0, s, wts, n, thr, always, cum, words, hy.on ? hy.words : nullptr);
    hipLaunchKernelGGL(k_mcl_gather, dim3((n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, src, dst, n, cum, r_draw, words, g, base, hy);
}

void cmk_mcl_hyp_bins(hipStream_t s, const CmMclParticleDev* parts, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_bins, dim3((hy.n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, parts, hy);
}

void cmk_mcl_hyp_link(hipStream_t s, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_link, dim3(((1u << hy.cap_bits) + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, hy);
}

void cmk_mcl_hyp_flatten(hipStream_t s, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    const uint32_t cap = 1u << hy.cap_bits;
    hipLaunchKernelGGL(k_mcl_hyp_roots, dim3((cap + CM_MCL_ONE_BLOCK - 1) / CM_MCL_ONE_BLOCK), dim3(CM_MCL_ONE_BLOCK), 0, s, hy);
    hipLaunchKernelGGL(k_mcl_hyp_flatten, dim3((cap + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, hy);
}

void cmk_mcl_hyp_sums(hipStream_t s, const CmMclParticleDev* parts, const CmMclWeightDev* wts, const float* dirs, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_sums, dim3((hy.n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, parts, wts, reinterpret_cast<const float2*>(dirs), hy);
}

void cmk_mcl_hyp_spread(hipStream_t s, const CmMclParticleDev* parts, const CmMclWeightDev* wts, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_spread, dim3((hy.n + CM_MCL_BLOCK - 1) / CM_MCL_BLOCK), dim3(CM_MCL_BLOCK), 0, s, parts, wts, hy);
}

void cmk_mcl_hyp_pick(hipStream_t s, const CmMclHypDev& hy) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_pick, dim3(1), dim3(CM_MCL_ONE_BLOCK), 0, s, hy);
}

void cmk_mcl_hyp_recover(hipStream_t s, const CmMclHypDev& hy, const unsigned long long* layer_words) {
    if (!hyp_ok(hy, hy.n)) return;
    hipLaunchKernelGGL(k_mcl_hyp_recover, dim3(1), dim3(64), 0, s, hy, layer_words);
}
