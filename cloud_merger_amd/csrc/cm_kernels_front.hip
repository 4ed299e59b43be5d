// cm_kernels_front.hip — the frontier layer behind the plan layer: the frontier cells of the occupancy map's image (free, cheap
// enough, an unknown edge neighbour in the window), their 8-connected components, the components of at least min_cells cells
// numbered by their smallest cell, a label per cell, a table entry per frontier and the choice among them, for gfx950 (wave64).
//
// Computed on request (cm_map_frontier_update) from the map's image, the cost layer's cost table and the plan layer's pot; it
// writes buffers of the frontier layer only (the semantics are in include/cloudmerge.h). Every quantity is an
// integer and every reduction commutative (count, sum, min, max), and a component's root is its smallest cell whatever the
// order of the unions, so the order in which the device works cannot show in the words.
//
//   k_front_local    one workgroup of CM_FRONT_BLOCK threads per tile of CM_FRONT_TILE x CM_FRONT_TILE cells: the tile's image
//                    bytes and one ring around them in LDS (a cell outside the window is not unknown), the predicate of
//                    step 1 per cell, then labels in LDS that fall to the smallest label among the eight neighbours in the
//                    tile and once more to that cell's own label, until a round changes nothing (at most CM_FRONT_TILE^2
//                    rounds: after round k every cell within k steps of its tile-local component's smallest cell holds it).
//                    Writes parent[c]: the window cell of that smallest cell, CM_FRONT_NONE_DEV for other cells; clears
//                    size[c]; counts the frontier cells.
//   k_front_merge    one thread per cell: for the pairs right, down and both diagonals below that straddle a tile edge or
//                    corner and are both frontier cells, unites the two trees: find both roots (parents strictly decrease),
//                    atomicMin the larger root's word to the smaller, go on with what the word held if it was no root.
//   k_front_flatten  one thread per cell: parent[c] becomes the root, size[root] counts (lanes of a wave that share a root
//                    add once, into one of CM_FRONT_SLOTS slots of the workgroup in LDS where the root finds one free, and
//                    the workgroup sends each slot on with one add).
//   k_front_count    per block of CM_FRONT_BLOCK cells the roots with size >= min_cells; adds the roots to the info.
//   k_front_scan     one workgroup: the exclusive scan of those counts in place, n_frontiers and n_written.
//   k_front_number   per block again: a root's number is its block's offset plus the roots of frontiers before it in the
//                    block; size[root] becomes the number (CM_FRONT_NONE_DEV below min_cells) and entry `number` of the table
//                    is initialised with first_cell and n_cells.
//   k_front_table    one thread per cell: the label becomes the root's number, and the cell's ix, iy and pot go into
//                    table[number] and box[number] for number < max_frontiers; lanes of a wave that share a number reduce
//                    among themselves first and one lane sends the atomics, through the workgroup's slots as in
//                    k_front_flatten: a frontier of a hundred thousand cells would otherwise send every wave to one entry.
//   k_front_best     one workgroup: puts every written entry into cm_frontier's form, scores it and reduces the choice.
//
// No workgroup waits on another, no loop spins: finds end at a root, a union's larger root strictly falls, the per-wave loops
// run once per distinct key of the wave.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"
#define CM_FRONT_FN __device__ __forceinline__
#include "cm_front_score.hpp"

namespace {

constexpr uint32_t kNone = CM_FRONT_NONE_DEV;
constexpr int kRing = CM_FRONT_TILE + 2;               // a tile's row in LDS with its ring
constexpr uint32_t kNoLabel = 0xFFFFu;                 // in LDS: no frontier cell

static_assert(sizeof(CmFrontEntryDev) == 40, "cm_frontier is 40 bytes");
static_assert(CM_FRONT_BLOCK == CM_FRONT_TILE * CM_FRONT_TILE && CM_FRONT_BLOCK % 64 == 0, "one thread per cell of a tile");

// The union-find on the label words (every word of a frontier cell holds a cell of the same component that is not above
// it): cm_search.hpp's, which the localisation layer's hypotheses share.
__device__ __forceinline__ uint32_t front_load(const uint32_t* p) { return cm_uf_load(p); }
__device__ __forceinline__ uint32_t front_find(const uint32_t* parent, uint32_t c) { return cm_uf_find(parent, c); }
__device__ __forceinline__ void front_unite(uint32_t* parent, uint32_t a, uint32_t b) { cm_uf_unite(parent, a, b); }

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_local(const signed char* __restrict__ image, const unsigned char* __restrict__ cost,
                                                                CmFrontDev g, uint32_t* __restrict__ labels, uint32_t* __restrict__ size,
                                                                uint32_t* __restrict__ info) {
    __shared__ signed char si[kRing * kRing];
    __shared__ uint16_t sl[kRing * kRing];
    const uint32_t tile = blockIdx.x;
    const uint32_t tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(kRing * kRing); i += CM_FRONT_BLOCK) {
        const int x = static_cast<int>(tx * CM_FRONT_TILE + i % kRing) - 1, y = static_cast<int>(ty * CM_FRONT_TILE + i / kRing) - 1;
        signed char v = 1;                             // (neither free nor unknown: outside the window)
        if (x >= 0 && y >= 0 && x < static_cast<int>(g.nx) && y < static_cast<int>(g.ny)) v = image[static_cast<uint32_t>(y) * g.nx + static_cast<uint32_t>(x)];
        si[i] = v;
        sl[i] = static_cast<uint16_t>(kNoLabel);
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % CM_FRONT_TILE, ly = threadIdx.x / CM_FRONT_TILE;
    const int li = static_cast<int>(ly + 1u) * kRing + static_cast<int>(lx + 1u);
    const uint32_t x = tx * CM_FRONT_TILE + lx, y = ty * CM_FRONT_TILE + ly;
    const bool inside = x < g.nx && y < g.ny;
    const uint32_t cell = y * g.nx + x;
    bool f = false;
    if (inside)
        f = si[li] == 0 && cost[cell] <= g.max_cost && (si[li + 1] == -1 || si[li - 1] == -1 || si[li + kRing] == -1 || si[li - kRing] == -1);
    uint32_t lab = f ? threadIdx.x : kNoLabel;         // (row-major in the tile: the order of the window cells of the tile)
    sl[li] = static_cast<uint16_t>(lab);
    __syncthreads();
    // Rounds in place: a thread may read a neighbour's label before or after that neighbour's store of the same round; both
    // are cells of the same tile-local component, labels only fall, and the round after a change runs again.
    for (uint32_t round = 0; round < CM_FRONT_TILE * CM_FRONT_TILE; ++round) {
        int changed = 0;
        if (f) {
            uint32_t m = lab, v;
            v = sl[li + 1];         m = v < m ? v : m;
            v = sl[li - 1];         m = v < m ? v : m;
            v = sl[li + kRing];     m = v < m ? v : m;
            v = sl[li - kRing];     m = v < m ? v : m;
            v = sl[li + kRing + 1]; m = v < m ? v : m;
            v = sl[li + kRing - 1]; m = v < m ? v : m;
            v = sl[li - kRing + 1]; m = v < m ? v : m;
            v = sl[li - kRing - 1]; m = v < m ? v : m;
            if (m < lab) {
                v = sl[static_cast<int>(m / CM_FRONT_TILE + 1u) * kRing + static_cast<int>(m % CM_FRONT_TILE + 1u)];   // (that cell's own label: a shortcut)
                lab = v < m ? v : m;
                sl[li] = static_cast<uint16_t>(lab);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (inside) {
        labels[cell] = f ? (ty * CM_FRONT_TILE + lab / CM_FRONT_TILE) * g.nx + tx * CM_FRONT_TILE + lab % CM_FRONT_TILE : kNone;
        size[cell] = 0u;
    }
    const int n = __syncthreads_count(f ? 1 : 0);
    if (threadIdx.x == 0 && n) atomicAdd(info, static_cast<uint32_t>(n));
}

// (labels is read and written by other threads of the same launch: no __restrict__ on it)
__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_merge(CmFrontDev g, uint32_t* labels) {
    const uint32_t c = blockIdx.x * CM_FRONT_BLOCK + threadIdx.x;
    if (c >= g.nx * g.ny) return;
    const uint32_t x = c % g.nx, y = c / g.nx;
    const bool l = x % CM_FRONT_TILE == 0u, r = x % CM_FRONT_TILE == CM_FRONT_TILE - 1u, t = y % CM_FRONT_TILE == CM_FRONT_TILE - 1u;
    if (!(l || r || t)) return;                        // (no pair of this cell straddles a tile edge)
    if (front_load(labels + c) == kNone) return;
    const bool xr = x + 1u < g.nx, xl = x >= 1u, yt = y + 1u < g.ny;
    if (r && xr && front_load(labels + c + 1u) != kNone) front_unite(labels, c, c + 1u);
    if (t && yt && front_load(labels + c + g.nx) != kNone) front_unite(labels, c, c + g.nx);
    if ((r || t) && xr && yt && front_load(labels + c + g.nx + 1u) != kNone) front_unite(labels, c, c + g.nx + 1u);
    if ((l || t) && xl && yt && front_load(labels + c + g.nx - 1u) != kNone) front_unite(labels, c, c + g.nx - 1u);
}

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_flatten(CmFrontDev g, uint32_t* labels, uint32_t* __restrict__ size) {
    __shared__ uint32_t s_key[CM_FRONT_SLOTS], s_n[CM_FRONT_SLOTS];
    const uint32_t c = blockIdx.x * CM_FRONT_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < CM_FRONT_SLOTS) {
        s_key[threadIdx.x] = kNone;
        s_n[threadIdx.x] = 0u;
    }
    __syncthreads();
    bool active = c < g.nx * g.ny;
    uint32_t root = kNone;
    if (active) active = front_load(labels + c) != kNone;
    if (active) {
        root = front_find(labels, c);
        labels[c] = root;                              // (an ancestor: a walk through c still ends at the root)
    }
    // One add per distinct root of the wave, at most 64 rounds: into the workgroup's slot of that root if the slot is free or
    // already the root's, to the size word itself otherwise. A big frontier then costs one add per workgroup, not one per wave.
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t k = __shfl(root, leader);
        const unsigned long long grp = __ballot(active && root == k);
        if (lane == static_cast<uint32_t>(leader)) {
            const uint32_t n = static_cast<uint32_t>(__popcll(grp)), slot = k % CM_FRONT_SLOTS;
            const uint32_t old = atomicCAS(s_key + slot, kNone, k);
            if (old == kNone || old == k) atomicAdd(s_n + slot, n);
            else atomicAdd(size + k, n);
        }
        todo &= ~grp;
    }
    __syncthreads();
    if (threadIdx.x < CM_FRONT_SLOTS && s_key[threadIdx.x] != kNone) atomicAdd(size + s_key[threadIdx.x], s_n[threadIdx.x]);
}

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_count(CmFrontDev g, const uint32_t* __restrict__ labels, const uint32_t* __restrict__ size,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ info) {
    const uint32_t c = blockIdx.x * CM_FRONT_BLOCK + threadIdx.x;
    const bool root = c < g.nx * g.ny && labels[c] == c;
    const bool front = root && size[c] >= g.min_cells;
    const int n_front = __syncthreads_count(front ? 1 : 0);
    const int n_root = __syncthreads_count(root ? 1 : 0);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = static_cast<uint32_t>(n_front);
        if (n_root) atomicAdd(info + 1, static_cast<uint32_t>(n_root));
    }
}

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_scan(CmFrontDev g, uint32_t* __restrict__ counts, uint32_t* __restrict__ info) {
    __shared__ uint32_t s[CM_FRONT_BLOCK];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < g.n_blocks; base += CM_FRONT_BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < g.n_blocks ? counts[i] : 0u;
        uint32_t incl = v;
        s[threadIdx.x] = incl;
        __syncthreads();
        for (uint32_t d = 1; d < CM_FRONT_BLOCK; d <<= 1) {
            const uint32_t o = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
            __syncthreads();
            incl += o;
            s[threadIdx.x] = incl;
            __syncthreads();
        }
        if (i < g.n_blocks) counts[i] = carry + incl - v;
        carry += s[CM_FRONT_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        info[2] = carry;
        info[3] = carry < g.max_frontiers ? carry : g.max_frontiers;
    }
}

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_number(CmFrontDev g, const uint32_t* __restrict__ labels, uint32_t* __restrict__ size,
                                                                 const uint32_t* __restrict__ counts, CmFrontEntryDev* __restrict__ table,
                                                                 uint32_t* __restrict__ box) {
    __shared__ uint32_t sw[CM_FRONT_BLOCK / 64];
    const uint32_t c = blockIdx.x * CM_FRONT_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool root = c < g.nx * g.ny && labels[c] == c;
    const uint32_t n = root ? size[c] : 0u;
    const bool front = root && n >= g.min_cells;
    const unsigned long long bal = __ballot(front);
    if (lane == 0u) sw[wave] = static_cast<uint32_t>(__popcll(bal));
    __syncthreads();
    if (!root) return;
    uint32_t num = counts[blockIdx.x] + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
    for (uint32_t w = 0; w < wave; ++w) num += sw[w];
    size[c] = front ? num : kNone;
    if (front && num < g.max_frontiers) {
        CmFrontEntryDev e;
        e.first_cell = c;
        e.n_cells = n;
        e.sum_x = 0ull;
        e.sum_y = 0ull;
        e.key = ~0ull;
        e.box01 = 0u;
        e.box23 = 0u;
        table[num] = e;
        box[4u * num + 0u] = 0xFFFFFFFFu;
        box[4u * num + 1u] = 0xFFFFFFFFu;
        box[4u * num + 2u] = 0u;
        box[4u * num + 3u] = 0u;
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_table(CmFrontDev g, const uint32_t* __restrict__ pot, uint32_t* __restrict__ labels,
                                                                const uint32_t* __restrict__ size, CmFrontEntryDev* __restrict__ table,
                                                                uint32_t* __restrict__ box) {
    __shared__ uint32_t s_key[CM_FRONT_SLOTS], s_sx[CM_FRONT_SLOTS], s_sy[CM_FRONT_SLOTS], s_box[4][CM_FRONT_SLOTS];
    __shared__ unsigned long long s_min[CM_FRONT_SLOTS];
    const uint32_t c = blockIdx.x * CM_FRONT_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < CM_FRONT_SLOTS) {
        s_key[threadIdx.x] = kNone;
        s_sx[threadIdx.x] = 0u;
        s_sy[threadIdx.x] = 0u;
        s_box[0][threadIdx.x] = 0xFFFFFFFFu;
        s_box[1][threadIdx.x] = 0xFFFFFFFFu;
        s_box[2][threadIdx.x] = 0u;
        s_box[3][threadIdx.x] = 0u;
        s_min[threadIdx.x] = ~0ull;
    }
    __syncthreads();
    bool active = c < g.nx * g.ny;
    uint32_t num = kNone;
    if (active) {
        const uint32_t root = labels[c];               // (a thread reads its own word of labels only, and writes it)
        if (root != kNone) {
            num = size[root];
            labels[c] = num;
        }
    }
    active = num < g.max_frontiers;                    // (kNone is above every max_frontiers)
    const uint32_t x = active ? c % g.nx : 0u, y = active ? c / g.nx : 0u;
    const uint32_t p = active ? pot[c] : kNone;
    const unsigned long long key = p != kNone ? (static_cast<unsigned long long>(p) << 32) | c : ~0ull;
    // One set of atomics per distinct number of the wave, at most 64 rounds; the other lanes enter each reduction with its
    // neutral element. They go into the workgroup's slot of that number if the slot is free or already the number's (sums of
    // at most CM_FRONT_BLOCK coordinates fit a word), to the table itself otherwise; the slots are sent on at the end.
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll(static_cast<long long>(todo)) - 1;
        const uint32_t k = __shfl(num, leader);
        const bool mine = active && num == k;
        const unsigned long long grp = __ballot(mine);
        const uint32_t sx = wave_sum(mine ? x : 0u), sy = wave_sum(mine ? y : 0u);
        const uint32_t x0 = wave_min(mine ? x : 0xFFFFFFFFu), y0 = wave_min(mine ? y : 0xFFFFFFFFu);
        const uint32_t x1 = wave_max(mine ? x : 0u), y1 = wave_max(mine ? y : 0u);
        const unsigned long long kmin = wave_min64(mine ? key : ~0ull);
        if (lane == static_cast<uint32_t>(leader)) {
            const uint32_t slot = k % CM_FRONT_SLOTS;
            const uint32_t old = atomicCAS(s_key + slot, kNone, k);
            if (old == kNone || old == k) {
                atomicAdd(s_sx + slot, sx);
                atomicAdd(s_sy + slot, sy);
                atomicMin(s_min + slot, kmin);
                atomicMin(&s_box[0][slot], x0);
                atomicMin(&s_box[1][slot], y0);
                atomicMax(&s_box[2][slot], x1);
                atomicMax(&s_box[3][slot], y1);
            } else {
                atomicAdd(&table[k].sum_x, static_cast<unsigned long long>(sx));
                atomicAdd(&table[k].sum_y, static_cast<unsigned long long>(sy));
                if (kmin != ~0ull) atomicMin(&table[k].key, kmin);
                atomicMin(box + 4u * k + 0u, x0);
                atomicMin(box + 4u * k + 1u, y0);
                atomicMax(box + 4u * k + 2u, x1);
                atomicMax(box + 4u * k + 3u, y1);
            }
        }
        todo &= ~grp;
    }
    __syncthreads();
    if (threadIdx.x < CM_FRONT_SLOTS && s_key[threadIdx.x] != kNone) {
        const uint32_t k = s_key[threadIdx.x];
        atomicAdd(&table[k].sum_x, static_cast<unsigned long long>(s_sx[threadIdx.x]));
        atomicAdd(&table[k].sum_y, static_cast<unsigned long long>(s_sy[threadIdx.x]));
        if (s_min[threadIdx.x] != ~0ull) atomicMin(&table[k].key, s_min[threadIdx.x]);
        atomicMin(box + 4u * k + 0u, s_box[0][threadIdx.x]);
        atomicMin(box + 4u * k + 1u, s_box[1][threadIdx.x]);
        atomicMax(box + 4u * k + 2u, s_box[2][threadIdx.x]);
        atomicMax(box + 4u * k + 3u, s_box[3][threadIdx.x]);
    }
}

// info: [0] frontier cells, [1] components, [2] frontiers, [3] entries written (k_front_scan); here [4] best, [5] 0, [6], [7]
// the score (cm_front_score.hpp: step 6 in 64 bits without a wrap).
__global__ __launch_bounds__(CM_FRONT_BLOCK) void k_front_best(CmFrontDev g, CmFrontEntryDev* __restrict__ table, const uint32_t* __restrict__ box,
                                                               uint32_t* __restrict__ info) {
    __shared__ long long ss[CM_FRONT_BLOCK];
    __shared__ uint32_t sk[CM_FRONT_BLOCK];
    const uint32_t n = info[3];
    long long best_s = 0x7FFFFFFFFFFFFFFFll;
    uint32_t best_k = kNone;
    for (uint32_t k = threadIdx.x; k < n; k += CM_FRONT_BLOCK) {
        const unsigned long long key = table[k].key;
        const uint32_t min_pot = static_cast<uint32_t>(key >> 32), min_cell = static_cast<uint32_t>(key);   // (no reachable cell: both words all ones)
        table[k].key = (static_cast<unsigned long long>(min_cell) << 32) | min_pot;
        table[k].box01 = box[4u * k + 0u] | (box[4u * k + 1u] << 16);
        table[k].box23 = box[4u * k + 2u] | (box[4u * k + 3u] << 16);
        if (min_pot == kNone) continue;
        const long long s = cm_front_score(g.pot_scale, g.gain_scale, min_pot, table[k].n_cells);
        if (best_k == kNone || s < best_s) {           // (k rises: a tie keeps the lower number)
            best_s = s;
            best_k = k;
        }
    }
    ss[threadIdx.x] = best_s;
    sk[threadIdx.x] = best_k;
    __syncthreads();
    for (uint32_t d = CM_FRONT_BLOCK / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const long long os = ss[threadIdx.x + d];
            const uint32_t ok = sk[threadIdx.x + d];
            const uint32_t mk = sk[threadIdx.x];
            if (ok != kNone && (mk == kNone || os < ss[threadIdx.x] || (os == ss[threadIdx.x] && ok < mk))) {
                ss[threadIdx.x] = os;
                sk[threadIdx.x] = ok;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long s = sk[0] == kNone ? 0ull : static_cast<unsigned long long>(ss[0]);
        info[4] = sk[0];
        info[5] = 0u;
        info[6] = static_cast<uint32_t>(s);
        info[7] = static_cast<uint32_t>(s >> 32);
    }
}

bool front_window_ok(const CmFrontDev& g) {
    const uint64_t n = static_cast<uint64_t>(g.nx) * g.ny;
    return g.nx >= 1 && g.ny >= 1 && g.nx <= 0xFFFFu && g.ny <= 0xFFFFu && n < 0xFFFFFFFFull &&
           g.tiles_x == (g.nx + CM_FRONT_TILE - 1) / CM_FRONT_TILE && g.tiles_y == (g.ny + CM_FRONT_TILE - 1) / CM_FRONT_TILE &&
           g.n_blocks == (n + CM_FRONT_BLOCK - 1) / CM_FRONT_BLOCK && g.max_frontiers >= 1 && g.max_frontiers <= CM_FRONT_MAX_TABLE_DEV;
}

}  // namespace

void cmk_front_local(hipStream_t s, const void* image, const unsigned char* cost, const CmFrontDev& g, uint32_t* labels, uint32_t* size,
                     uint32_t* info) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_local, dim3(g.tiles_x * g.tiles_y), dim3(CM_FRONT_BLOCK), 0, s, static_cast<const signed char*>(image), cost, g, labels,
                       size, info);
}

void cmk_front_merge(hipStream_t s, const CmFrontDev& g, uint32_t* labels) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_merge, dim3(g.n_blocks), dim3(CM_FRONT_BLOCK), 0, s, g, labels);
}

void cmk_front_flatten(hipStream_t s, const CmFrontDev& g, uint32_t* labels, uint32_t* size) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_flatten, dim3(g.n_blocks), dim3(CM_FRONT_BLOCK), 0, s, g, labels, size);
}

void cmk_front_count(hipStream_t s, const CmFrontDev& g, const uint32_t* labels, const uint32_t* size, uint32_t* counts, uint32_t* info) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_count, dim3(g.n_blocks), dim3(CM_FRONT_BLOCK), 0, s, g, labels, size, counts, info);
}

void cmk_front_scan(hipStream_t s, const CmFrontDev& g, uint32_t* counts, uint32_t* info) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_scan, dim3(1), dim3(CM_FRONT_BLOCK), 0, s, g, counts, info);
}

void cmk_front_number(hipStream_t s, const CmFrontDev& g, const uint32_t* labels, uint32_t* size, const uint32_t* counts, CmFrontEntryDev* table,
                      uint32_t* box) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_number, dim3(g.n_blocks), dim3(CM_FRONT_BLOCK), 0, s, g, labels, size, counts, table, box);
}

void cmk_front_table(hipStream_t s, const CmFrontDev& g, const uint32_t* pot, uint32_t* labels, const uint32_t* size, CmFrontEntryDev* table,
                     uint32_t* box) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_table, dim3(g.n_blocks), dim3(CM_FRONT_BLOCK), 0, s, g, pot, labels, size, table, box);
}

void cmk_front_best(hipStream_t s, const CmFrontDev& g, CmFrontEntryDev* table, const uint32_t* box, uint32_t* info) {
    if (!front_window_ok(g)) return;
    hipLaunchKernelGGL(k_front_best, dim3(1), dim3(CM_FRONT_BLOCK), 0, s, g, table, box, info);
}
