// cm_kernels_msearch.hip — branch-and-bound scan matching of the last frame against the occupancy map over wide windows: the
// search layer behind the cost layer (cm_map_match_search), for gfx950 (wave64). The exhaustive layer's k_match_field and
// k_match_mark (cm_kernels_match.hip) fill this layer's field and bitmaps; what is here is the rest (the
// semantics are in include/cloudmerge.h).
//
// A node is one word: (k + n_a) << 24 | (j0 + wy) << 12 | (i0 + wx), so that the order of the words is the node order and, at
// level 0, the order of the entry indices. Every sum is an integer sum over a set of cells and every list stands for a set of
// nodes: neither the order in which workgroups arrive nor the order of a list can show in a score, in the bound B, in a
// count or in the best entry. No workgroup waits for another; every loop runs over a list length, a cell count or 64 lanes.
//
//   k_msearch_pyramid  one thread per stored byte of level h: the four-way max of level h - 1 at offsets {0, 2^(h-1)}^2,
//                      0 where level h - 1 stores nothing (the ring of 2^h - 1 bytes on the negative side is what the
//                      storage is wider by).
//   k_msearch_list     one thread per bitmap word of a candidate: popcount, a prefix over the wave, one atomicAdd per wave
//                      into the candidate's count, the cells written as x | y << 16 behind the wave's base, none at or
//                      beyond max_cells (the count still counts them all: that is the overflow the host reports).
//   k_msearch_score    one workgroup per node of a list and stripe of its candidate's cells (blockIdx.y of `splits`
//                      stripes): the node's offset is uniform over the workgroup, every thread takes cells of the stripe 256
//                      apart, one byte gather from the level's table each (0 outside its storage), a wave reduction, one LDS
//                      combine, then one store (splits == 1) or one integer atomicAdd into a zeroed score (a short list over
//                      many cells would otherwise leave most of the device idle). The list's length is read from device
//                      memory, so the descent for B runs without the host.
//   k_msearch_pick     one workgroup: the node of the largest U of a list, ties to the first in node order; its children in
//                      range become the next tiny list, or, at level 0, B = max(U, U of the prior's leaf).
//   k_msearch_select   one thread per node: U >= B, the children in range written behind a per-wave base from one atomicAdd
//                      (none at or beyond the capacity), the live nodes and the children counted.
//   k_msearch_best     one workgroup over the leaves: step 6's key over those with U >= B, the best one's score and cell
//                      count, the number of live leaves, and the four neighbours of step 7 as a list of leaves.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_device.h"
#include "cm_kernels.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;                // the node that does not exist: its score is 0

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m));
    return v;
}

// (inclusive prefix over the wave)
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = static_cast<uint32_t>(__shfl_up(static_cast<int>(v), m));
        if (lane >= static_cast<uint32_t>(m)) v += o;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_msearch_pyramid(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, uint32_t nx,
                                                         uint32_t ny, uint32_t h) {
    const uint32_t s = 1u << (h - 1u), off = 2u * s - 1u, soff = s - 1u;
    const uint32_t pw = nx + off, ph = ny + off, spw = nx + soff, sph = ny + soff;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= pw * ph) return;
    // level coordinates (x, y) = (X - off, Y - off); level h - 1 stores (x', y') at (x' + soff, y' + soff)
    const int X = static_cast<int>(t % pw) - static_cast<int>(off) + static_cast<int>(soff);
    const int Y = static_cast<int>(t / pw) - static_cast<int>(off) + static_cast<int>(soff);
    uint32_t m = 0u;
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
            const int sx = X + a * static_cast<int>(s), sy = Y + b * static_cast<int>(s);
            if (sx >= 0 && sx < static_cast<int>(spw) && sy >= 0 && sy < static_cast<int>(sph)) {
                const uint32_t v = src[static_cast<size_t>(sy) * spw + static_cast<size_t>(sx)];
                m = v > m ? v : m;
            }
        }
    dst[t] = static_cast<unsigned char>(m);
}

__global__ __launch_bounds__(256) void k_msearch_list(const uint32_t* __restrict__ bits, uint32_t words, uint32_t nx, uint32_t n_cells,
                                                      uint32_t max_cells, uint32_t* __restrict__ cells, uint32_t* __restrict__ counts) {
    const uint32_t k = blockIdx.y, w = blockIdx.x * 256 + threadIdx.x;
    uint32_t word = w < words ? bits[static_cast<size_t>(k) * words + w] : 0u;
    const uint32_t cnt = static_cast<uint32_t>(__popc(word));
    const uint32_t incl = wave_scan(cnt);
    uint32_t base = 0u;
    if ((threadIdx.x & 63u) == 63u && incl) base = atomicAdd(counts + k, incl);
    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), 63));
    uint32_t pos = base + incl - cnt;
    uint32_t* const out = cells + static_cast<size_t>(k) * max_cells;
    while (word) {                                     // (at most 32 rounds)
        const uint32_t b = static_cast<uint32_t>(__ffs(static_cast<int>(word))) - 1u;
        word &= word - 1u;
        const uint32_t cell = w * 32u + b;
        if (cell < n_cells && pos < max_cells) out[pos] = (cell % nx) | ((cell / nx) << 16);
        ++pos;
    }
}

__global__ __launch_bounds__(CM_MSEARCH_BLOCK) void k_msearch_score(const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_ptr, CmMSearchDev g,
                                                                    const unsigned char* __restrict__ tab, uint32_t h,
                                                                    const uint32_t* __restrict__ cells, const uint32_t* __restrict__ counts,
                                                                    uint32_t splits, uint32_t* __restrict__ U) {
    __shared__ uint32_t s_sum[CM_MSEARCH_BLOCK / 64];
    const uint32_t b = blockIdx.x;
    if (b >= *n_ptr) return;                           // (uniform over the workgroup)
    const uint32_t node = list[b], kk = node >> 24;
    uint32_t sum = 0u;
    if (node != kNone && kk < g.n_k) {
        const uint32_t off = (1u << h) - 1u, pw = g.nx + off, ph = g.ny + off;
        // storage column of cell x under the node: x + i0 + off, i0 = (node & 4095) - wx; rows likewise
        const int dx = static_cast<int>(node & 4095u) - static_cast<int>(g.wx) + static_cast<int>(off);
        const int dy = static_cast<int>((node >> 12) & 4095u) - static_cast<int>(g.wy) + static_cast<int>(off);
        const uint32_t n = counts[kk] < g.max_cells ? counts[kk] : g.max_cells;
        const uint32_t* const ck = cells + static_cast<size_t>(kk) * g.max_cells;
#pragma unroll 4                                       // (several gathers in flight per thread)
        for (uint32_t c = blockIdx.y * CM_MSEARCH_BLOCK + threadIdx.x; c < n; c += CM_MSEARCH_BLOCK * splits) {
            const uint32_t cell = ck[c];
            const int x = static_cast<int>(cell & 0xFFFFu) + dx, y = static_cast<int>(cell >> 16) + dy;
            if (x >= 0 && x < static_cast<int>(pw) && y >= 0 && y < static_cast<int>(ph)) sum += tab[static_cast<size_t>(y) * pw + static_cast<size_t>(x)];
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < CM_MSEARCH_BLOCK / 64; ++w) sum += s_sum[w];
        if (splits == 1u) U[b] = sum;
        else if (sum) atomicAdd(U + b, sum);
    }
}

// The children of `node` at level h > 0 that are in range, in node order; returns their number.
__device__ __forceinline__ uint32_t children_of(uint32_t node, uint32_t h, const CmMSearchDev& g, uint32_t out[4]) {
    const uint32_t s = 1u << (h - 1u), ii = node & 4095u, jj = (node >> 12) & 4095u, top = node & 0xFF000000u;
    uint32_t n = 0u;
    for (uint32_t b = 0; b < 2u; ++b)
        for (uint32_t a = 0; a < 2u; ++a)
            if (ii + a * s <= 2u * g.wx && jj + b * s <= 2u * g.wy) out[n++] = top | ((jj + b * s) << 12) | (ii + a * s);
    return n;
}

// words: the layer's info words (CM_MSEARCH_W_*). list / U hold *n_ptr >= 1 nodes of level h.
__global__ __launch_bounds__(CM_MSEARCH_ONE_BLOCK) void k_msearch_pick(const uint32_t* list, const uint32_t* U, const uint32_t* n_ptr, uint32_t n_max,
                                                                       CmMSearchDev g, uint32_t h, uint32_t* words) {
    __shared__ unsigned long long s_key[CM_MSEARCH_ONE_BLOCK / 64];
    const uint32_t n = *n_ptr < n_max ? *n_ptr : n_max;
    unsigned long long key = 0ull;                     // (U << 32 | ~node: the largest U, then the first node; 0: none)
    for (uint32_t e = threadIdx.x; e < n; e += CM_MSEARCH_ONE_BLOCK) {
        const unsigned long long v = (static_cast<unsigned long long>(U[e]) << 32) | (~list[e]);
        key = v > key ? v : key;
    }
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63u) == 0u) s_key[threadIdx.x >> 6] = key;
    __syncthreads();                                   // (every read of list and U lies before it: the tiny list may be both)
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < CM_MSEARCH_ONE_BLOCK / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
    const uint32_t node = ~static_cast<uint32_t>(key), u = static_cast<uint32_t>(key >> 32);
    for (uint32_t t = 0; t < 4u; ++t) words[CM_MSEARCH_W_TINY_U + t] = 0u;     // (the next level's scores are added into them)
    if (n == 0u) {                                     // (cannot happen: there is a root)
        words[CM_MSEARCH_W_TN] = 0u;
        return;
    }
    if (h == 0u) {
        const uint32_t p = words[CM_MSEARCH_W_PRIOR_U];
        words[CM_MSEARCH_W_B] = u > p ? u : p;
        words[CM_MSEARCH_W_TN] = 0u;
        return;
    }
    uint32_t ch[4];
    const uint32_t nc = children_of(node, h, g, ch);
    for (uint32_t t = 0; t < nc; ++t) words[CM_MSEARCH_W_TINY + t] = ch[t];
    words[CM_MSEARCH_W_TN] = nc;
    words[CM_MSEARCH_W_PROBE] += nc;
}

// counters[0] += live nodes, counters[1] += their children; next holds the first `cap` children that arrive.
__global__ __launch_bounds__(256) void k_msearch_select(const uint32_t* __restrict__ list, const uint32_t* __restrict__ U, uint32_t n, CmMSearchDev g,
                                                        uint32_t h, const uint32_t* __restrict__ bound, uint32_t* __restrict__ next, uint32_t cap,
                                                        uint32_t* __restrict__ counters) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = e < n && U[e] >= *bound;
    uint32_t ch[4];
    const uint32_t nc = live ? children_of(list[e], h, g, ch) : 0u;
    const unsigned long long mask = __ballot(live);
    const uint32_t incl = wave_scan(nc);
    uint32_t base = 0u;
    if (lane == 63u && incl) base = atomicAdd(counters + 1, incl);
    base = static_cast<uint32_t>(__shfl(static_cast<int>(base), 63));
    if (lane == 0u && mask) atomicAdd(counters, static_cast<uint32_t>(__popcll(mask)));
    const uint32_t pos = base + incl - nc;
    for (uint32_t t = 0; t < nc; ++t)
        if (pos + t < cap) next[pos + t] = ch[t];
}

// Step 6 over the leaves: a larger key is better, an equal key goes to the lower node (the lower entry index).
__device__ __forceinline__ unsigned long long msearch_key(uint32_t score, uint32_t node, const CmMSearchDev& g) {
    const int i = static_cast<int>(node & 4095u) - static_cast<int>(g.wx), j = static_cast<int>((node >> 12) & 4095u) - static_cast<int>(g.wy);
    const int k = static_cast<int>(node >> 24) - static_cast<int>(g.n_a);
    const uint32_t d2 = static_cast<uint32_t>(i * i + j * j), ak = static_cast<uint32_t>(k < 0 ? -k : k);     // d2 <= 2 * 1024^2: 22 bits
    return (static_cast<unsigned long long>(score) << 29) | (static_cast<unsigned long long>(0x3FFFFFu - d2) << 7) | (127u - ak);
}

__global__ __launch_bounds__(CM_MSEARCH_ONE_BLOCK) void k_msearch_best(const uint32_t* __restrict__ list, const uint32_t* __restrict__ U, uint32_t n,
                                                                       CmMSearchDev g, const uint32_t* __restrict__ counts, uint32_t* words) {
    __shared__ unsigned long long s_key[CM_MSEARCH_ONE_BLOCK / 64];
    __shared__ uint32_t s_node[CM_MSEARCH_ONE_BLOCK / 64], s_live[CM_MSEARCH_ONE_BLOCK / 64];
    const uint32_t B = words[CM_MSEARCH_W_B];
    unsigned long long key = 0ull;
    uint32_t node = kNone, live = 0u;
    const auto fold = [&](unsigned long long ok, uint32_t on) {
        if (on != kNone && (node == kNone || ok > key || (ok == key && on < node))) {
            key = ok;
            node = on;
        }
    };
    for (uint32_t e = threadIdx.x; e < n; e += CM_MSEARCH_ONE_BLOCK) {
        const uint32_t u = U[e];
        if (u < B) continue;
        ++live;
        fold(msearch_key(u, list[e], g), list[e]);
    }
    for (int m = 1; m < 64; m <<= 1) fold(__shfl_xor(key, m), static_cast<uint32_t>(__shfl_xor(static_cast<int>(node), m)));
    live = wave_sum(live);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_key[wave] = key;
        s_node[wave] = node;
        s_live[wave] = live;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1; w < CM_MSEARCH_ONE_BLOCK / 64; ++w) {
        fold(s_key[w], s_node[w]);
        live += s_live[w];
    }
    words[CM_MSEARCH_W_LIVE0] = live;
    words[CM_MSEARCH_W_BEST] = node;
    if (node == kNone) return;                         // (cannot happen: the entry B was taken from is live)
    const uint32_t kk = node >> 24, ii = node & 4095u, jj = (node >> 12) & 4095u;
    words[CM_MSEARCH_W_SCORE] = static_cast<uint32_t>(key >> 29);
    words[CM_MSEARCH_W_NCELLS] = kk < g.n_k ? counts[kk] : 0u;
    words[CM_MSEARCH_W_NEIGH + 0] = ii > 0u ? node - 1u : kNone;
    words[CM_MSEARCH_W_NEIGH + 1] = ii < 2u * g.wx ? node + 1u : kNone;
    words[CM_MSEARCH_W_NEIGH + 2] = jj > 0u ? node - (1u << 12) : kNone;
    words[CM_MSEARCH_W_NEIGH + 3] = jj < 2u * g.wy ? node + (1u << 12) : kNone;
}

bool msearch_ok(const CmMSearchDev& g) {
    return g.nx >= 1 && g.ny >= 1 && g.nx <= 65535u && g.ny <= 65535u && static_cast<uint64_t>(g.nx) * g.ny <= (1u << 22) && g.n_k == 2u * g.n_a + 1u &&
           g.n_k <= 255u && g.wx <= CM_MSEARCH_MAX_SHIFT_DEV && g.wy <= CM_MSEARCH_MAX_SHIFT_DEV && g.max_cells >= 1u;
}

}  // namespace

void cmk_msearch_pyramid(hipStream_t s, const unsigned char* src, unsigned char* dst, uint32_t nx, uint32_t ny, uint32_t h) {
    if (h < 1u || h > CM_MSEARCH_MAX_DEPTH_DEV || !nx || !ny) return;
    const uint64_t n = static_cast<uint64_t>(nx + (1u << h) - 1u) * (ny + (1u << h) - 1u);
    hipLaunchKernelGGL(k_msearch_pyramid, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, s, src, dst, nx, ny, h);
}

void cmk_msearch_list(hipStream_t s, const uint32_t* bits, const CmMSearchDev& g, uint32_t words, uint32_t* cells, uint32_t* counts) {
    if (!msearch_ok(g) || !words) return;
    hipLaunchKernelGGL(k_msearch_list, dim3((words + 255) / 256, g.n_k), dim3(256), 0, s, bits, words, g.nx, g.nx * g.ny, g.max_cells, cells, counts);
}

void cmk_msearch_score(hipStream_t s, const uint32_t* list, const uint32_t* n_ptr, uint32_t n_max, const CmMSearchDev& g, const unsigned char* tab,
                       uint32_t h, const uint32_t* cells, const uint32_t* counts, uint32_t splits, uint32_t* U) {
    if (!msearch_ok(g) || h > CM_MSEARCH_MAX_DEPTH_DEV || !n_max || splits < 1u || splits > 65535u) return;
    hipLaunchKernelGGL(k_msearch_score, dim3(n_max, splits), dim3(CM_MSEARCH_BLOCK), 0, s, list, n_ptr, g, tab, h, cells, counts, splits, U);
}

void cmk_msearch_pick(hipStream_t s, const uint32_t* list, const uint32_t* U, const uint32_t* n_ptr, uint32_t n_max, const CmMSearchDev& g, uint32_t h,
                      uint32_t* words) {
    if (!msearch_ok(g) || h > CM_MSEARCH_MAX_DEPTH_DEV) return;
    hipLaunchKernelGGL(k_msearch_pick, dim3(1), dim3(CM_MSEARCH_ONE_BLOCK), 0, s, list, U, n_ptr, n_max, g, h, words);
}

void cmk_msearch_select(hipStream_t s, const uint32_t* list, const uint32_t* U, uint32_t n, const CmMSearchDev& g, uint32_t h, const uint32_t* bound,
                        uint32_t* next, uint32_t cap, uint32_t* counters) {
    if (!msearch_ok(g) || h < 1u || h > CM_MSEARCH_MAX_DEPTH_DEV || !n) return;
    hipLaunchKernelGGL(k_msearch_select, dim3((n + 255) / 256), dim3(256), 0, s, list, U, n, g, h, bound, next, cap, counters);
}

void cmk_msearch_best(hipStream_t s, const uint32_t* list, const uint32_t* U, uint32_t n, const CmMSearchDev& g, const uint32_t* counts, uint32_t* words) {
    if (!msearch_ok(g)) return;
    hipLaunchKernelGGL(k_msearch_best, dim3(1), dim3(CM_MSEARCH_ONE_BLOCK), 0, s, list, U, n, g, counts, words);
}
