// cm_kernels_match.hip — correlative scan matching of the last frame against the occupancy map: an exhaustive search over a
// window of (yaw, x, y) around a prior pose, every candidate scored by looking the frame's hit cells up in a likelihood field
// of the map (Olson's real-time correlative scan matching, cartographer's RealTimeCorrelativeScanMatcher), for gfx950 (wave64).
//
// Computed on request (cm_map_match_evaluate) from the frame's clouds in place exactly as k_map_mark reads them, the map's
// info and the cost layer's dist2; it writes buffers of the matching layer only (the semantics are in
// include/cloudmerge.h). A score is an integer sum over a set of cells, so neither the order of the atomics nor the order of
// a workgroup's cell list can show in the volume.
//
//   k_match_field  one thread per window cell: dist2 through the field table into one byte L.
//   k_match_mark   one workgroup per tile of 4096 raw points: k_map_mark's front end and masks (points of A in the height
//                  band), each point read once and carried through the 2 n_a + 1 candidate matrices, which the host built;
//                  the index of a candidate is uniform over the workgroup, its six floats one cache line's worth of loads.
//                  A point's window cell under candidate k sets its bit in k's bitmap, the atomicOr skipped where a plain
//                  read shows the bit.
//   k_match_score  one workgroup per (candidate k, tile of CM_MATCH_TILE x CM_MATCH_TILE window cells). The tile's rows of
//                  k's bitmap are cut out of at most two words each; a tile without a bit ends there. Otherwise the set bits
//                  become a list of LDS offsets, the tile's L bytes with a halo of (wx, wy) cells (0 outside the window) are
//                  staged in LDS, and every thread takes translations tid, tid + CM_MATCH_BLOCK, ...: the sum of the bytes
//                  at list offset + translation offset, one integer atomicAdd per non-zero sum into the zeroed volume.
//   k_match_best   one workgroup: the largest score, ties to the smallest i * i + j * j, then the smallest |k| (one 64-bit
//                  key), then the lowest entry index; then the popcount of the best candidate's bitmap and the scores of the
//                  best entry's four neighbours for the host's sub-cell step.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

constexpr uint32_t kTile = CM_MATCH_TILE;
static_assert(kTile == 32, "a tile row is cut out of two bitmap words");
static_assert((kTile + 2 * CM_MATCH_MAX_SHIFT_DEV) * (kTile + 2 * CM_MATCH_MAX_SHIFT_DEV) <= 65536, "a list entry is a 16-bit LDS offset");

__global__ __launch_bounds__(256) void k_match_field(const uint32_t* __restrict__ dist2, const unsigned char* __restrict__ lut, uint32_t r2,
                                                     uint32_t n_cells, unsigned char* __restrict__ field) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const uint32_t d2 = dist2[c];
    field[c] = d2 <= r2 ? lut[d2] : static_cast<unsigned char>(0);     // (CM_MAP_DIST_NONE is beyond every table)
}

// q: per candidate the six floats Q00 Q01 Q02 Q10 Q11 Q12. bits: g.n_k bitmaps of g.words words, zero before the launch.
__global__ __launch_bounds__(CM_BLOCK) void k_match_mark(const CmFrameDev* __restrict__ fd, CmMatchDev g, const float* __restrict__ q,
                                                         const unsigned char* __restrict__ keep, uint32_t* __restrict__ bits) {
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
        if (keep && !keep[slot]) continue;             // (a counted point of A)
        if (!(g.z_min <= z && z <= g.z_max)) continue;
        for (uint32_t k = 0; k < g.n_k; ++k) {
            const float* m = q + 6u * k;
            int gx, gy;
            if (!world_axis(xf_row(m[0], m[1], m[2], g.tx, x, y, z), g.inv, &gx) ||
                !world_axis(xf_row(m[3], m[4], m[5], g.ty, x, y, z), g.inv, &gy)) continue;
            const long long ix = static_cast<long long>(gx) - g.ax, iy = static_cast<long long>(gy) - g.ay;
            if (ix < 0 || ix >= static_cast<long long>(g.nx) || iy < 0 || iy >= static_cast<long long>(g.ny)) continue;
            const uint32_t cell = static_cast<uint32_t>(ix) + static_cast<uint32_t>(iy) * g.nx;
            const uint32_t b = 1u << (cell & 31u);
            uint32_t* w = bits + static_cast<size_t>(k) * g.words + (cell >> 5);
            if (!(ld_agent(w) & b)) atomicOr(w, b);
        }
    }
}

// Dynamic LDS: kTile * kTile list entries (16-bit offsets into the staged field), then the staged field,
// (kTile + 2 wx) x (kTile + 2 wy) bytes.
__global__ __launch_bounds__(CM_MATCH_BLOCK) void k_match_score(const unsigned char* __restrict__ field, const uint32_t* __restrict__ bits,
                                                                CmMatchDev g, uint32_t tiles_x, uint32_t* __restrict__ vol) {
    extern __shared__ __align__(16) unsigned char s_mem[];
    __shared__ uint32_t s_rows[kTile];
    __shared__ uint32_t s_n;
    unsigned short* const s_list = reinterpret_cast<unsigned short*>(s_mem);
    unsigned char* const s_field = s_mem + kTile * kTile * sizeof(unsigned short);
    const uint32_t tid = threadIdx.x, k = blockIdx.y;
    const uint32_t x0 = (blockIdx.x % tiles_x) * kTile, y0 = (blockIdx.x / tiles_x) * kTile;
    const uint32_t tw = g.nx - x0 < kTile ? g.nx - x0 : kTile;
    const uint32_t pitch = kTile + 2u * g.wx, rows = kTile + 2u * g.wy;
    const uint32_t* const bk = bits + static_cast<size_t>(k) * g.words;
    if (tid < kTile) {
        uint32_t m = 0u;
        if (y0 + tid < g.ny) {
            const uint32_t b0 = (y0 + tid) * g.nx + x0, w = b0 >> 5, sh = b0 & 31u;
            const unsigned long long lo = bk[w], hi = w + 1u < g.words ? bk[w + 1u] : 0u;
            m = static_cast<uint32_t>(((hi << 32) | lo) >> sh);
            if (tw < 32u) m &= (1u << tw) - 1u;
        }
        s_rows[tid] = m;
    }
    if (tid == 0u) s_n = 0u;
    __syncthreads();
    for (uint32_t c = tid; c < kTile * kTile; c += CM_MATCH_BLOCK) {
        const uint32_t r = c / kTile, b = c % kTile;
        if ((s_rows[r] >> b) & 1u) s_list[atomicAdd(&s_n, 1u)] = static_cast<unsigned short>(r * pitch + b);
    }
    __syncthreads();
    const uint32_t n = s_n;
    if (n == 0u) return;                               // (the whole workgroup: an empty tile costs its 64 word loads)
    for (uint32_t t = tid; t < pitch * rows; t += CM_MATCH_BLOCK) {
        const long long gx = static_cast<long long>(x0) + (t % pitch) - g.wx, gy = static_cast<long long>(y0) + (t / pitch) - g.wy;
        const bool in = gx >= 0 && gx < static_cast<long long>(g.nx) && gy >= 0 && gy < static_cast<long long>(g.ny);
        s_field[t] = in ? field[static_cast<size_t>(gy) * g.nx + static_cast<size_t>(gx)] : static_cast<unsigned char>(0);
    }
    __syncthreads();
    const uint32_t sx = 2u * g.wx + 1u, sy = 2u * g.wy + 1u;
    uint32_t* const vk = vol + static_cast<size_t>(k) * sx * sy;
    const uint32_t n4 = n & ~3u;
    for (uint32_t t = tid; t < sx * sy; t += CM_MATCH_BLOCK) {
        // translation (i, j) = (t % sx - wx, t / sx - wy): tile cell (b, r) shifted by it is staged at (b + i + wx, r + j + wy)
        const unsigned char* const f = s_field + (t / sx) * pitch + (t % sx);
        uint32_t sum = 0u;
        for (uint32_t c = 0; c < n4; c += 4u) {
            const ushort4 o = *reinterpret_cast<const ushort4*>(s_list + c);
            sum += static_cast<uint32_t>(f[o.x]) + f[o.y] + f[o.z] + f[o.w];
        }
        for (uint32_t c = n4; c < n; ++c) sum += f[s_list[c]];
        if (sum) atomicAdd(vk + t, sum);
    }
}

// The total order of step 6 without its last rule: a larger key is better.
__device__ __forceinline__ unsigned long long match_key(uint32_t score, uint32_t e, const CmMatchDev& g) {
    const uint32_t sx = 2u * g.wx + 1u, sy = 2u * g.wy + 1u;
    const int i = static_cast<int>(e % sx) - static_cast<int>(g.wx), j = static_cast<int>((e / sx) % sy) - static_cast<int>(g.wy);
    const int k = static_cast<int>(e / (sx * sy)) - static_cast<int>(g.n_a);
    const uint32_t d2 = static_cast<uint32_t>(i * i + j * j), ak = static_cast<uint32_t>(k < 0 ? -k : k);
    return (static_cast<unsigned long long>(score) << 21) | (static_cast<unsigned long long>(16383u - d2) << 7) | (127u - ak);
}

__global__ __launch_bounds__(CM_MATCH_BEST_BLOCK) void k_match_best(const uint32_t* __restrict__ vol, const uint32_t* __restrict__ bits, CmMatchDev g,
                                                                   uint32_t* __restrict__ info) {
    __shared__ unsigned long long s_key[CM_MATCH_BEST_BLOCK / 64];
    __shared__ uint32_t s_index[CM_MATCH_BEST_BLOCK / 64], s_count[CM_MATCH_BEST_BLOCK / 64];
    __shared__ uint32_t s_best;
    const uint32_t sx = 2u * g.wx + 1u, sy = 2u * g.wy + 1u, n = g.n_k * sx * sy;
    unsigned long long key = 0ull;
    uint32_t index = 0xFFFFFFFFu;
    for (uint32_t e = threadIdx.x; e < n; e += CM_MATCH_BEST_BLOCK) {     // (ascending e: a tie keeps the lower index)
        const unsigned long long v = match_key(vol[e], e, g);
        if (index == 0xFFFFFFFFu || v > key) {
            key = v;
            index = e;
        }
    }
    const auto fold = [&](unsigned long long ok, uint32_t oi) {
        if (oi != 0xFFFFFFFFu && (index == 0xFFFFFFFFu || ok > key || (ok == key && oi < index))) {
            key = ok;
            index = oi;
        }
    };
    for (int m = 1; m < 64; m <<= 1) fold(__shfl_xor(key, m), static_cast<uint32_t>(__shfl_xor(static_cast<int>(index), m)));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_key[wave] = key;
        s_index[wave] = index;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CM_MATCH_BEST_BLOCK / 64; ++w) fold(s_key[w], s_index[w]);
        s_best = index;
    }
    __syncthreads();
    const uint32_t best = s_best;                      // (n >= 1: there is one)
    const uint32_t* const bk = bits + static_cast<size_t>(best / (sx * sy)) * g.words;
    uint32_t count = 0u;
    for (uint32_t w = threadIdx.x; w < g.words; w += CM_MATCH_BEST_BLOCK) count += static_cast<uint32_t>(__popc(bk[w]));
    for (int m = 1; m < 64; m <<= 1) count += static_cast<uint32_t>(__shfl_xor(static_cast<int>(count), m));
    if ((threadIdx.x & 63u) == 0u) s_count[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CM_MATCH_BEST_BLOCK / 64; ++w) count += s_count[w];
        const uint32_t bi = best % sx, bj = (best / sx) % sy;
        info[0] = best;
        info[1] = count;
        info[2] = vol[best];
        info[3] = bi > 0u ? vol[best - 1u] : 0u;
        info[4] = bi + 1u < sx ? vol[best + 1u] : 0u;
        info[5] = bj > 0u ? vol[best - sx] : 0u;
        info[6] = bj + 1u < sy ? vol[best + sx] : 0u;
        info[7] = 0u;
    }
}

bool match_ok(const CmMatchDev& g) {
    return g.nx >= 1 && g.ny >= 1 && static_cast<uint64_t>(g.nx) * g.ny <= (1u << 22) && g.n_k == 2u * g.n_a + 1u && g.n_k <= CM_MATCH_MAX_ANGLES_DEV &&
           g.wx <= CM_MATCH_MAX_SHIFT_DEV && g.wy <= CM_MATCH_MAX_SHIFT_DEV &&
           static_cast<uint64_t>(g.n_k) * (2u * g.wx + 1u) * (2u * g.wy + 1u) <= (1u << 22) &&
           g.words == static_cast<uint32_t>((static_cast<uint64_t>(g.nx) * g.ny + 31u) / 32u);
}

}  // namespace

void cmk_match_field(hipStream_t s, const uint32_t* dist2, const unsigned char* lut, uint32_t r2, uint32_t n_cells, unsigned char* field) {
    if (n_cells) hipLaunchKernelGGL(k_match_field, dim3((n_cells + 255) / 256), dim3(256), 0, s, dist2, lut, r2, n_cells, field);
}

void cmk_match_mark(hipStream_t s, const CmFrameDev* fd, const CmMatchDev& g, const float* q, const unsigned char* keep, uint32_t* bits,
                    uint32_t n_tiles) {
    if (!match_ok(g)) return;
    if (n_tiles) hipLaunchKernelGGL(k_match_mark, dim3(n_tiles), dim3(CM_BLOCK), 0, s, fd, g, q, keep, bits);
}

void cmk_match_score(hipStream_t s, const unsigned char* field, const uint32_t* bits, const CmMatchDev& g, uint32_t* vol) {
    if (!match_ok(g)) return;
    const uint32_t tiles_x = (g.nx + kTile - 1) / kTile, tiles_y = (g.ny + kTile - 1) / kTile;
    const size_t lds = kTile * kTile * sizeof(unsigned short) + static_cast<size_t>(kTile + 2u * g.wx) * (kTile + 2u * g.wy);
    hipLaunchKernelGGL(k_match_score, dim3(tiles_x * tiles_y, g.n_k), dim3(CM_MATCH_BLOCK), lds, s, field, bits, g, tiles_x, vol);
}

void cmk_match_best(hipStream_t s, const uint32_t* vol, const uint32_t* bits, const CmMatchDev& g, uint32_t* info) {
    if (!match_ok(g)) return;
    hipLaunchKernelGGL(k_match_best, dim3(1), dim3(CM_MATCH_BEST_BLOCK), 0, s, vol, bits, g, info);
}
