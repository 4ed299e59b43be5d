// cm_kernels_plan.hip — the plan layer behind the cost layer: the exact shortest-path potential of every window cell to a
// goal over the inflated costmap (navfn's potential without its interpolation), and a path by descent, for gfx950 (wave64).
//
// Computed on request (cm_map_plan_update, cm_map_plan_path) from the cost layer's cost table; it writes buffers of the plan
// layer only (the semantics are in include/cloudmerge.h). Every step cost is a positive integer, so the
// Bellman equations have one solution and the order in which cells are relaxed cannot show in the words.
//
//   k_plan_init   one thread per cell: CM_PLAN_UNREACHABLE everywhere, 0 at the goal; the first threads fill the two tile
//                 flag tables: the goal's tile and the tiles around it are dirty for the first sweep (the goal's word never
//                 changes, so no sweep would tell its neighbours across a tile edge).
//   k_plan_sweep  one workgroup of CM_PLAN_BLOCK threads per tile of CM_PLAN_TILE x CM_PLAN_TILE cells; a tile that is not
//                 dirty ends at once. A dirty tile stages its words of pot and one ring of cells around them, and the
//                 traversal weights of the same cells from their cost bytes (0: impassable, or outside the window), into
//                 LDS, relaxes there in pull form, one thread per cell reading its eight neighbours, until a round changes
//                 nothing (at most CM_PLAN_TILE^2 rounds: every round but the last lowers a word to its final value in the
//                 tile; a round is CM_PLAN_INNER passes between two barriers), writes back the words that fell, marks in the other flag table the neighbour tiles whose ring holds
//                 one of them and counts itself in the sweep's counter. No workgroup waits on another: a tile may read ring
//                 words that a neighbour is writing in the same launch. Every word it can see there is the cost of a walk to
//                 the goal, words only fall, and the writer marks this tile for the next launch, which reads what the
//                 previous one wrote (DESIGN.md §24 has the argument).
//   k_plan_path   one wave walks step 6: lanes 0..7 load the potential and the cost byte of the eight neighbours (one round
//                 trip to L2 per step), the straight lanes' weights say which diagonal steps exist, and a minimum over
//                 (cost of the step, direction) picks the next cell. At most max_cells steps.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_device.h"
#include "cm_kernels.h"

namespace {

constexpr uint32_t kUnreachable = 0xFFFFFFFFu;     // CM_PLAN_UNREACHABLE
constexpr int kRing = CM_PLAN_TILE + 2;            // a tile's row in LDS with its ring

// Step 1: the traversal weight of a cost byte; 0 stands for impassable. The goal cell counts as passable.
__device__ __forceinline__ uint32_t plan_weight(uint32_t v, uint32_t cell, const CmPlanDev& g) {
    if (v == 255u && g.allow_unknown) v = 252u;
    const uint32_t w = v >= 253u ? 0u : g.neutral + ((v * g.factor_q8) >> 8);
    return cell == g.goal && w == 0u ? 1u : w;
}

__global__ __launch_bounds__(256) void k_plan_init(CmPlanDev g, uint32_t* __restrict__ pot, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_tiles = g.tiles_x * g.tiles_y;
    if (i < n_tiles) {
        const int dx = static_cast<int>(i % g.tiles_x) - static_cast<int>(g.goal % g.nx / CM_PLAN_TILE);
        const int dy = static_cast<int>(i / g.tiles_x) - static_cast<int>(g.goal / g.nx / CM_PLAN_TILE);
        flags[i] = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1 ? 1u : 0u;
        flags[n_tiles + i] = 0u;
    }
    if (i < g.nx * g.ny) pot[i] = i == g.goal ? 0u : kUnreachable;
}

// (pot is read and written by other tiles of the same launch: no __restrict__ on it)
__global__ __launch_bounds__(CM_PLAN_BLOCK) void k_plan_sweep(const unsigned char* __restrict__ cost, CmPlanDev g, uint32_t* pot,
                                                              uint32_t* __restrict__ cur, uint32_t* __restrict__ next,
                                                              uint32_t* __restrict__ counter) {
    __shared__ uint32_t sp[kRing * kRing];
    __shared__ uint16_t sw[kRing * kRing];
    const uint32_t tile = blockIdx.x;
    if (!cur[tile]) return;                            // (uniform: the whole workgroup leaves; only this workgroup writes the word in this launch, below)
    const uint32_t tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(kRing * kRing); i += CM_PLAN_BLOCK) {
        const int x = static_cast<int>(tx * CM_PLAN_TILE + i % kRing) - 1, y = static_cast<int>(ty * CM_PLAN_TILE + i / kRing) - 1;
        uint32_t p = kUnreachable, w = 0u;
        if (x >= 0 && y >= 0 && x < static_cast<int>(g.nx) && y < static_cast<int>(g.ny)) {
            const uint32_t cell = static_cast<uint32_t>(y) * g.nx + static_cast<uint32_t>(x);
            p = pot[cell];
            w = plan_weight(cost[cell], cell, g);
        }
        sp[i] = p;
        sw[i] = static_cast<uint16_t>(w);              // (at most 255 + 252)
    }
    __syncthreads();
    // Cleared behind the barrier: every wave of the workgroup has read the flag and taken its branch above before any of
    // them passes here, so no wave can see the cleared word and leave alone. This table is the next sweep's `next`.
    if (threadIdx.x == 0) cur[tile] = 0u;
    const uint32_t lx = threadIdx.x % CM_PLAN_TILE, ly = threadIdx.x / CM_PLAN_TILE;
    const int li = static_cast<int>(ly + 1u) * kRing + static_cast<int>(lx + 1u);
    const uint32_t w = sw[li];
    const bool pe = sw[li + 1] != 0, pn = sw[li + kRing] != 0, pw = sw[li - 1] != 0, ps = sw[li - kRing] != 0;
    const uint32_t first = sp[li];
    uint32_t p = first;
    // Rounds in place: a thread may read a neighbour's word before or after that neighbour's store of the same round; both
    // are costs of walks, and the round after a change runs again. A round is CM_PLAN_INNER passes with no barrier between
    // them: the barrier only serves the vote on whether to stop, and fewer of them measured faster. 64-bit sums: an
    // unreachable neighbour never wins.
    for (uint32_t round = 0; round < CM_PLAN_TILE * CM_PLAN_TILE; ++round) {
        int changed = 0;
        for (int inner = 0; inner < CM_PLAN_INNER && w; ++inner) {
            const uint64_t s = 5u * w, d = 7u * w;
            uint64_t best = p;
            uint64_t v;
            v = sp[li + 1] + s;                              best = v < best ? v : best;
            v = sp[li + kRing] + s;                          best = v < best ? v : best;
            v = sp[li - 1] + s;                              best = v < best ? v : best;
            v = sp[li - kRing] + s;                          best = v < best ? v : best;
            v = sp[li + kRing + 1] + d;                      best = pe && pn && v < best ? v : best;
            v = sp[li + kRing - 1] + d;                      best = pw && pn && v < best ? v : best;
            v = sp[li - kRing - 1] + d;                      best = pw && ps && v < best ? v : best;
            v = sp[li - kRing + 1] + d;                      best = pe && ps && v < best ? v : best;
            if (best < p) {
                p = static_cast<uint32_t>(best);
                sp[li] = p;
                changed = 1;
            }
            asm volatile("" ::: "memory");             // (the next pass reads the neighbours' words again)
        }
        if (!__syncthreads_or(changed)) break;
    }
    const bool fell = p != first;                      // (only cells of the window have a weight, so only they fall)
    if (fell) {
        pot[(ty * CM_PLAN_TILE + ly) * g.nx + tx * CM_PLAN_TILE + lx] = p;
        const bool l = lx == 0u && tx > 0u, r = lx == CM_PLAN_TILE - 1u && tx + 1u < g.tiles_x;
        const bool b = ly == 0u && ty > 0u, t = ly == CM_PLAN_TILE - 1u && ty + 1u < g.tiles_y;
        if (l) next[tile - 1u] = 1u;
        if (r) next[tile + 1u] = 1u;
        if (b) next[tile - g.tiles_x] = 1u;
        if (t) next[tile + g.tiles_x] = 1u;
        if (l && b) next[tile - g.tiles_x - 1u] = 1u;
        if (r && b) next[tile - g.tiles_x + 1u] = 1u;
        if (l && t) next[tile + g.tiles_x - 1u] = 1u;
        if (r && t) next[tile + g.tiles_x + 1u] = 1u;
    }
    if (__syncthreads_or(fell ? 1 : 0) && threadIdx.x == 0) atomicAdd(counter, 1u);
}

// out: CM_PLAN_PATH_HEAD words { n_cells, status, pot(start), 0 }, then the cells.
__global__ __launch_bounds__(64) void k_plan_path(const unsigned char* __restrict__ cost, const uint32_t* __restrict__ pot, CmPlanDev g,
                                                  uint32_t start, uint32_t max_cells, uint32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x, d = lane & 7u;
    const int ddx = d == 0u || d == 1u || d == 7u ? 1 : (d == 2u || d == 6u ? 0 : -1);
    const int ddy = d >= 1u && d <= 3u ? 1 : (d == 0u || d == 4u ? 0 : -1);
    const uint32_t k = (d & 1u) ? 7u : 5u;
    const uint32_t pot_start = pot[start];
    uint32_t c = start, n = 0u, status = pot_start == kUnreachable ? CM_PLAN_PATH_UNREACHABLE_DEV : CM_PLAN_PATH_TRUNCATED_DEV;
    for (uint32_t i = 0; i < max_cells && pot_start != kUnreachable; ++i) {
        if (lane == 0u) out[CM_PLAN_PATH_HEAD + i] = c;
        n = i + 1u;
        if (c == g.goal) { status = CM_PLAN_PATH_FOUND_DEV; break; }
        const int x = static_cast<int>(c % g.nx) + ddx, y = static_cast<int>(c / g.nx) + ddy;
        uint32_t pn = kUnreachable, wn = 0u;
        const uint32_t cell = static_cast<uint32_t>(y) * g.nx + static_cast<uint32_t>(x);
        if (x >= 0 && y >= 0 && x < static_cast<int>(g.nx) && y < static_cast<int>(g.ny)) {
            pn = pot[cell];
            wn = plan_weight(cost[cell], cell, g);
        }
        const uint32_t wc = plan_weight(cost[c], c, g);
        const bool pe = __shfl(wn, 0) != 0u, pnn = __shfl(wn, 2) != 0u, pw = __shfl(wn, 4) != 0u, ps = __shfl(wn, 6) != 0u;
        const bool corner = d == 1u ? pe && pnn : d == 3u ? pw && pnn : d == 5u ? pw && ps : d == 7u ? pe && ps : true;
        unsigned long long key = pn != kUnreachable && corner ? ((static_cast<unsigned long long>(pn) + k * wc) << 3) | d : ~0ull;
        for (int m = 1; m < 8; m <<= 1) {
            const unsigned long long o = __shfl_xor(key, m);
            key = o < key ? o : key;
        }
        if (key == ~0ull) { status = CM_PLAN_PATH_BROKEN_DEV; break; }   // (no step from a reachable cell: pot is not a fixed point)
        const uint32_t dd = static_cast<uint32_t>(key & 7u);
        const int sx = dd == 0u || dd == 1u || dd == 7u ? 1 : (dd == 2u || dd == 6u ? 0 : -1);
        const int sy = dd >= 1u && dd <= 3u ? 1 : (dd == 0u || dd == 4u ? 0 : -1);
        c = static_cast<uint32_t>(static_cast<int>(c / g.nx) + sy) * g.nx + static_cast<uint32_t>(static_cast<int>(c % g.nx) + sx);
    }
    if (lane == 0u) {
        out[0] = n;
        out[1] = status;
        out[2] = pot_start;
        out[3] = 0u;
    }
}

bool plan_window_ok(const CmPlanDev& g) {
    return g.nx >= 1 && g.ny >= 1 && g.tiles_x == (g.nx + CM_PLAN_TILE - 1) / CM_PLAN_TILE && g.tiles_y == (g.ny + CM_PLAN_TILE - 1) / CM_PLAN_TILE &&
           g.goal < g.nx * g.ny;
}

}  // namespace

void cmk_plan_init(hipStream_t s, const CmPlanDev& g, uint32_t* pot, uint32_t* flags) {
    if (!plan_window_ok(g)) return;
    hipLaunchKernelGGL(k_plan_init, dim3((g.nx * g.ny + 255u) / 256u), dim3(256), 0, s, g, pot, flags);
}

void cmk_plan_sweep(hipStream_t s, const unsigned char* cost, const CmPlanDev& g, uint32_t* pot, uint32_t* cur, uint32_t* next,
                    uint32_t* counter) {
    if (!plan_window_ok(g)) return;
    hipLaunchKernelGGL(k_plan_sweep, dim3(g.tiles_x * g.tiles_y), dim3(CM_PLAN_BLOCK), 0, s, cost, g, pot, cur, next, counter);
}

void cmk_plan_path(hipStream_t s, const unsigned char* cost, const uint32_t* pot, const CmPlanDev& g, uint32_t start, uint32_t max_cells,
                   uint32_t* out) {
    if (!plan_window_ok(g) || start >= g.nx * g.ny) return;
    hipLaunchKernelGGL(k_plan_path, dim3(1), dim3(64), 0, s, cost, pot, g, start, max_cells, out);
}
