// cm_kernels_cluster.hip — Euclidean cluster extraction on the last frame's result (pcl::EuclideanClusterExtraction), for gfx950.
//
// A by-product computed on request after a frame (cm_result_clusters), never part of one. It reads the result records (and
// out_cnt on a context that keeps it) and writes into buffers of its own only.
//
//   k_cl_bounds   min / max of the centroids as order-preserving integer images (atomicMin / atomicMax: order-free)
//   k_cl_keys     cell key of every centroid in a search grid of its own, cell >= tolerance (cluster_grid, cm_route.cpp);
//                 digit-0 counts per tile and per group of tiles, as k_keys leaves them for the radix sort
//   radix sort    of (cell key, result index) with the general path's k_hist / k_gscan / k_scatter, ballot-ranked
//   k_cl_gather   the centroids in sorted order (x, y, z, result index); parent[i] = i, counters zeroed
//   k_row_*       the (y,z)-row table of the sorted keys (cmk_sorted_rows, shared with the outlier stages)
//   k_cl_hook     one lane per centroid: the candidates that precede it in sorted order (4 rows x 3 cells and its own row up
//                 to itself: every pair is looked at once, the predicate is symmetric), the fp32 predicate of the radius
//                 stage, and a lock-free union on RESULT indices: atomicMin on the parent words, so a parent is always
//                 smaller than its child and a root is the smallest index of its tree
//   k_cl_roots    root of every voxel (parents are final: plain loads), component sizes and point counts at the root
//   k_cl_count / k_cl_scan / k_cl_number   roots that pass the size filter, numbered in ascending order (= ascending
//                 smallest member); the cluster table's first / n_voxels / n_points
//   k_cl_labels   label of every voxel, AABB by atomicMin / atomicMax on integer images, keys of the second sort
//   radix sort    of (cluster number, voxel index), stable: the member lists, ascending inside a cluster
//   k_cl_decode   the AABB images back to floats
//
// Why one hook launch is enough: a union that finds its larger root r already hooked (atomicMin returns a value != r) goes on
// with that older parent and the smaller root, so no link is ever dropped; parents only decrease, so every walk ends. Loads
// of parent words inside the launch bypass the CU's L1 (relaxed agent-scope atomic loads); a value that is stale all the
// same is an older ancestor of the same tree and only costs steps, because the atomicMin that follows sees the truth.
//
// From cm_search.hpp: the integer images (f2ord / ord2f), the guarded atomics (ld_agent, min_into, max_into), the cell of a
// coordinate (grid_cell), the walk of a row's cells (for_row_cells) and the predicate's d2 (d2_of).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

// bounds: [0..2] min images (set to 0xFFFFFFFF), [3..5] max images (set to 0)
__global__ __launch_bounds__(CM_BLOCK) void k_cl_bounds(const float4* __restrict__ recs, uint32_t n, uint32_t* __restrict__ bounds) {
    __shared__ uint32_t sb[6];
    if (threadIdx.x < 6) sb[threadIdx.x] = threadIdx.x < 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * CM_BLOCK + threadIdx.x; i < n; i += gridDim.x * CM_BLOCK) {
        const float4 p = recs[i];
        const uint32_t o[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&sb[a], lo[a]); atomicMax(&sb[3 + a], hi[a]); }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], sb[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&bounds[threadIdx.x], sb[threadIdx.x]);
}

__global__ __launch_bounds__(CM_BLOCK) void k_cl_keys(const float4* __restrict__ recs, uint32_t n, CmClusterGridDev g,
                                                      uint32_t n_passes, CmFrameState* __restrict__ st,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                      uint32_t* __restrict__ grp) {
    __shared__ uint32_t lh[CM_RADIX];
    const uint32_t tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0) {
        // the sort's own state record: what k_hist / k_scatter (status, passes) and the row table (div_b) read
        st->status = CM_DEV_OK;
        st->n_passes = n_passes;
        st->n_valid = 0;
        st->err = 0;
        for (int a = 0; a < 3; ++a) st->div_b[a] = static_cast<int32_t>(g.dims[a]);
    }
    lh[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        uint32_t key = CM_INVALID_KEY;
        if (i < n) {
            const float4 p = recs[i];
            const uint32_t c0 = grid_cell(p.x, g.min[0], g.inv, g.dims[0]);
            const uint32_t c1 = grid_cell(p.y, g.min[1], g.inv, g.dims[1]);
            const uint32_t c2 = grid_cell(p.z, g.min[2], g.inv, g.dims[2]);
            key = c0 + g.dims[0] * (c1 + g.dims[1] * c2);
            atomicAdd(&lh[key & (CM_RADIX - 1)], 1u);
        }
        keys[i] = key;
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    hist[static_cast<size_t>(tile) * CM_RADIX + threadIdx.x] = c;
    if (c) atomicAdd(&grp[static_cast<size_t>(tile / CM_GROUP) * CM_RADIX + threadIdx.x], c);
}

__global__ __launch_bounds__(CM_BLOCK) void k_cl_gather(const float4* __restrict__ recs, const CmFrameState* __restrict__ st,
                                                        const uint32_t* __restrict__ vals_a, const uint32_t* __restrict__ vals_b,
                                                        uint32_t n, float4* __restrict__ pts, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ size, uint32_t* __restrict__ npts) {
    const uint32_t s = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t* __restrict__ vals = pick(st, vals_a, vals_b);
    const uint32_t idx = vals[s];
    const float4 p = recs[idx];
    pts[s] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
    parent[s] = s;
    size[s] = 0;
    npts[s] = 0;
}

// Root of x; halves the path on the way with atomicMin (a parent word is never raised).
__device__ __forceinline__ uint32_t cl_find(uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = ld_agent(&parent[x]);
    while (p != x) {
        const uint32_t gp = ld_agent(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void cl_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;                              // a was a root: hooked under b
        a = old;                                           // a had a parent already: that one and b are still to be joined
    }
}

__global__ __launch_bounds__(CM_BLOCK) void k_cl_hook(const CmFrameState* __restrict__ st, const uint32_t* __restrict__ keys_a,
                                                      const uint32_t* __restrict__ keys_b, const float4* __restrict__ pts,
                                                      const uint2* __restrict__ rows, uint32_t n, float tol2,
                                                      uint32_t* __restrict__ parent) {
    const uint32_t s = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t* __restrict__ keys = pick(st, keys_a, keys_b);
    const uint32_t dx = static_cast<uint32_t>(st->div_b[0]), dy = static_cast<uint32_t>(st->div_b[1]);
    const uint32_t key = keys[s];
    const float4 me = pts[s];
    const uint32_t my = __float_as_uint(me.w);
    const uint32_t row = key / dx, cx = key - row * dx;
    const uint32_t cz = row / dy, cy = row - cz * dy;
    const uint32_t x_lo = cx ? cx - 1u : 0u, x_hi = (cx + 1u < dx) ? cx + 1u : dx - 1u;
    // the rows at or before mine in key order: (z - 1; y - 1, y, y + 1), (z; y - 1), and my own row up to myself
#pragma unroll 1
    for (int q = 0; q < 5; ++q) {
        const int oz = q < 3 ? -1 : 0, oy = q < 3 ? q - 1 : q - 4;
        if ((oz < 0 && cz == 0u) || (oy < 0 && cy == 0u) || (oy > 0 && cy + 1u >= dy)) continue;
        const uint32_t r = (cy + static_cast<uint32_t>(oy)) + dy * (cz + static_cast<uint32_t>(oz));
        const uint2 rg = rows[r];
        for_row_cells(keys, rg.x, q == 4 ? s : rg.y, r, dx, x_lo, x_hi, [&](uint32_t t) {
            const float4 p = pts[t];
            if (d2_of(me, p) < tol2) cl_unite(parent, my, __float_as_uint(p.w));
        });
    }
}

// One add per wave for the lanes that share the first active lane's root (a component that holds most of the cloud would
// otherwise serialise every add on one word); the other lanes add for themselves.
__global__ __launch_bounds__(CM_BLOCK) void k_cl_roots(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ out_cnt,
                                                       uint32_t n, uint32_t* __restrict__ root, uint32_t* __restrict__ size,
                                                       uint32_t* __restrict__ npts) {
    const uint32_t i = blockIdx.x * CM_BLOCK + threadIdx.x;
    const bool has = i < n;
    uint32_t r = 0xFFFFFFFFu, cnt = 0;
    if (has) {
        r = i;
        for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
        root[i] = r;
        cnt = out_cnt ? out_cnt[i] : 0u;
    }
    const unsigned long long act = __ballot(has);
    if (act == 0ull) return;
    const int lead = __ffsll(static_cast<long long>(act)) - 1;
    const uint32_t r0 = static_cast<uint32_t>(__shfl(static_cast<int>(r), lead));
    const bool same = has && r == r0;
    const uint32_t n_same = static_cast<uint32_t>(__popcll(__ballot(same)));
    const uint32_t c_same = wave_sum_u32(same ? cnt : 0u);
    if (has && !same) {
        atomicAdd(&size[r], 1u);
        if (cnt) atomicAdd(&npts[r], cnt);
    }
    if (static_cast<int>(threadIdx.x & 63) == lead) {
        atomicAdd(&size[r0], n_same);
        if (c_same) atomicAdd(&npts[r0], c_same);
    }
}

__device__ __forceinline__ bool cl_kept(uint32_t i, uint32_t root, uint32_t size, uint32_t min_size, uint32_t max_size) {
    return root == i && size >= min_size && size <= max_size;
}

// tile_sums[tile] = (kept roots, their voxels) of the tile's CM_TILE voxels
__global__ __launch_bounds__(CM_BLOCK) void k_cl_count(const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                                                       uint32_t n, uint32_t min_size, uint32_t max_size,
                                                       uint2* __restrict__ tile_sums) {
    __shared__ uint32_t lds[CM_WAVES];
    uint32_t k = 0, v = 0;
#pragma unroll 4
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = blockIdx.x * CM_TILE + r * CM_BLOCK + threadIdx.x;
        if (i < n && cl_kept(i, root[i], size[i], min_size, max_size)) { ++k; v += size[i]; }
    }
    k = block_sum<CM_WAVES>(k, lds);
    v = block_sum<CM_WAVES>(v, lds);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = make_uint2(k, v);
}

// One workgroup: exclusive prefix over the tiles, in place; words[0] = clusters, words[1] = clustered voxels.
__global__ __launch_bounds__(CM_BLOCK) void k_cl_scan(uint2* __restrict__ tile_sums, uint32_t n_tiles, uint32_t* __restrict__ words) {
    __shared__ uint32_t lds[CM_WAVES];
    uint32_t run_k = 0, run_v = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += CM_BLOCK) {
        const uint32_t t = t0 + threadIdx.x;
        const uint2 c = t < n_tiles ? tile_sums[t] : make_uint2(0u, 0u);
        uint32_t tot_k, tot_v;
        const uint32_t ek = block_excl_scan<CM_WAVES>(c.x, lds, &tot_k);
        const uint32_t ev = block_excl_scan<CM_WAVES>(c.y, lds, &tot_v);
        if (t < n_tiles) tile_sums[t] = make_uint2(run_k + ek, run_v + ev);
        run_k += tot_k;
        run_v += tot_v;
    }
    if (threadIdx.x == 0) { words[0] = run_k; words[1] = run_v; }
}

// num[i]: the cluster number of a kept root, CM_INVALID_KEY for every other voxel; the kept roots' table entries (AABB as
// empty integer images). Thread t owns the tile's voxels 16 t .. 16 t + 15, so the numbers ascend with the voxel index.
__global__ __launch_bounds__(CM_BLOCK) void k_cl_number(const uint32_t* __restrict__ root, const uint32_t* __restrict__ size,
                                                        const uint32_t* __restrict__ npts, const uint2* __restrict__ tile_excl,
                                                        uint32_t n, uint32_t min_size, uint32_t max_size,
                                                        uint32_t* __restrict__ num, CmClusterDev* __restrict__ clusters) {
    __shared__ uint32_t lds[CM_WAVES];
    const uint32_t first = blockIdx.x * CM_TILE + threadIdx.x * CM_ITEMS;
    uint32_t sz[CM_ITEMS];
    uint32_t kept = 0, k = 0, v = 0;
#pragma unroll
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = first + r;
        sz[r] = 0;
        if (i < n) {
            sz[r] = size[i];
            if (cl_kept(i, root[i], sz[r], min_size, max_size)) { kept |= 1u << r; ++k; v += sz[r]; }
        }
    }
    uint32_t tot;
    const uint2 base = tile_excl[blockIdx.x];
    uint32_t ck = base.x + block_excl_scan<CM_WAVES>(k, lds, &tot);
    uint32_t cv = base.y + block_excl_scan<CM_WAVES>(v, lds, &tot);
#pragma unroll
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = first + r;
        if (i >= n) break;
        uint32_t c = CM_INVALID_KEY;
        if ((kept >> r) & 1u) {
            c = ck++;
            CmClusterDev e;
            e.first = cv; e.n_voxels = sz[r]; e.n_points = npts[i]; e._pad = 0;
            e.lo[0] = e.lo[1] = e.lo[2] = 0xFFFFFFFFu;
            e.hi[0] = e.hi[1] = e.hi[2] = 0u;
            clusters[c] = e;
            cv += sz[r];
        }
        num[i] = c;
    }
}

__global__ __launch_bounds__(CM_BLOCK) void k_cl_labels(const float4* __restrict__ recs, const uint32_t* __restrict__ root,
                                                        const uint32_t* __restrict__ num, uint32_t n, uint32_t n_passes,
                                                        CmFrameState* __restrict__ st, uint32_t* __restrict__ labels,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ grp, CmClusterDev* __restrict__ clusters) {
    __shared__ uint32_t lh[CM_RADIX];
    const uint32_t tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0) {
        st->status = CM_DEV_OK;
        st->n_passes = n_passes;
        st->n_valid = 0;
        st->err = 0;
    }
    lh[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
#pragma unroll 2
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        uint32_t c = CM_INVALID_KEY;
        uint32_t o[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
        if (i < n) {
            c = num[root[i]];
            labels[i] = c;
            if (c != CM_INVALID_KEY) {
                atomicAdd(&lh[c & (CM_RADIX - 1)], 1u);
                const float4 p = recs[i];
                o[0] = o[3] = f2ord(p.x); o[1] = o[4] = f2ord(p.y); o[2] = o[5] = f2ord(p.z);
            }
        }
        keys[i] = c;
        // The lanes that share the first clustered lane's cluster fold their boxes inside the wave and that lane alone
        // goes to memory (a cluster that holds most of the cloud would otherwise send every lane to the same six words).
        const unsigned long long act = __ballot(c != CM_INVALID_KEY);
        if (act == 0ull) continue;                          // wave-uniform
        const int lead = __ffsll(static_cast<long long>(act)) - 1;
        const uint32_t c0 = static_cast<uint32_t>(__shfl(static_cast<int>(c), lead));
        const bool same = c == c0;
        uint32_t w[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) w[a] = same ? o[a] : (a < 3 ? 0xFFFFFFFFu : 0u);
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                w[a] = min(w[a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(w[a]), step)));
                w[3 + a] = max(w[3 + a], static_cast<uint32_t>(__shfl_xor(static_cast<int>(w[3 + a]), step)));
            }
        }
        if (lane == lead || (c != CM_INVALID_KEY && !same)) {
            CmClusterDev* e = &clusters[c];
            uint32_t v[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[a] = lane == lead ? w[a] : o[a];
            min_into(&e->lo[0], v[0]); min_into(&e->lo[1], v[1]); min_into(&e->lo[2], v[2]);
            max_into(&e->hi[0], v[3]); max_into(&e->hi[1], v[4]); max_into(&e->hi[2], v[5]);
        }
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    hist[static_cast<size_t>(tile) * CM_RADIX + threadIdx.x] = c;
    if (c) atomicAdd(&grp[static_cast<size_t>(tile / CM_GROUP) * CM_RADIX + threadIdx.x], c);
}

__global__ __launch_bounds__(CM_BLOCK) void k_cl_decode(CmClusterDev* __restrict__ clusters, uint32_t n_clusters) {
    const uint32_t t = blockIdx.x * CM_BLOCK + threadIdx.x;
    if (t >= n_clusters * 6u) return;
    uint32_t* w = &clusters[t / 6u].lo[0] + t % 6u;       // lo[3] and hi[3] are six consecutive words
    *w = __float_as_uint(ord2f(*w));
}

}  // namespace

void cmk_cl_bounds(hipStream_t s, const void* recs, uint32_t n, uint32_t* bounds) {
    const uint32_t blocks = (n + CM_TILE - 1) / CM_TILE;
    CM_LAUNCH(k_cl_bounds, blocks < 1024u ? blocks : 1024u, CM_BLOCK, s, reinterpret_cast<const float4*>(recs), n, bounds);
}
void cmk_cl_keys(hipStream_t s, const void* recs, uint32_t n, const CmClusterGridDev& g, uint32_t n_passes, CmFrameState* st,
                 uint32_t* keys, uint32_t* hist, uint32_t* grp, uint32_t n_tiles) {
    CM_LAUNCH(k_cl_keys, n_tiles, CM_BLOCK, s, reinterpret_cast<const float4*>(recs), n, g, n_passes, st, keys, hist, grp);
}
void cmk_cl_gather(hipStream_t s, const void* recs, const CmFrameState* st, const uint32_t* vals_a, const uint32_t* vals_b, uint32_t n,
                   void* pts, uint32_t* parent, uint32_t* size, uint32_t* npts) {
    CM_LAUNCH(k_cl_gather, (n + CM_BLOCK - 1) / CM_BLOCK, CM_BLOCK, s, reinterpret_cast<const float4*>(recs), st, vals_a, vals_b, n,
              reinterpret_cast<float4*>(pts), parent, size, npts);
}
void cmk_cl_hook(hipStream_t s, const CmFrameState* st, const uint32_t* keys_a, const uint32_t* keys_b, const void* pts,
                 const void* rows, uint32_t n, float tol2, uint32_t* parent) {
    CM_LAUNCH(k_cl_hook, (n + CM_BLOCK - 1) / CM_BLOCK, CM_BLOCK, s, st, keys_a, keys_b, reinterpret_cast<const float4*>(pts),
              reinterpret_cast<const uint2*>(rows), n, tol2, parent);
}
void cmk_cl_roots(hipStream_t s, const uint32_t* parent, const uint32_t* out_cnt, uint32_t n, uint32_t* root, uint32_t* size,
                  uint32_t* npts) {
    CM_LAUNCH(k_cl_roots, (n + CM_BLOCK - 1) / CM_BLOCK, CM_BLOCK, s, parent, out_cnt, n, root, size, npts);
}
void cmk_cl_count(hipStream_t s, const uint32_t* root, const uint32_t* size, uint32_t n, uint32_t min_size, uint32_t max_size,
                  void* tile_sums, uint32_t* words, uint32_t n_tiles) {
    CM_LAUNCH(k_cl_count, n_tiles, CM_BLOCK, s, root, size, n, min_size, max_size, reinterpret_cast<uint2*>(tile_sums));
    CM_LAUNCH(k_cl_scan, 1, CM_BLOCK, s, reinterpret_cast<uint2*>(tile_sums), n_tiles, words);
}
void cmk_cl_number(hipStream_t s, const uint32_t* root, const uint32_t* size, const uint32_t* npts, const void* tile_excl,
                   uint32_t n, uint32_t min_size, uint32_t max_size, uint32_t* num, void* clusters, uint32_t n_tiles) {
    CM_LAUNCH(k_cl_number, n_tiles, CM_BLOCK, s, root, size, npts, reinterpret_cast<const uint2*>(tile_excl), n, min_size, max_size,
              num, reinterpret_cast<CmClusterDev*>(clusters));
}
void cmk_cl_labels(hipStream_t s, const void* recs, const uint32_t* root, const uint32_t* num, uint32_t n, uint32_t n_passes,
                   CmFrameState* st, uint32_t* labels, uint32_t* keys, uint32_t* hist, uint32_t* grp, void* clusters,
                   uint32_t n_tiles) {
    CM_LAUNCH(k_cl_labels, n_tiles, CM_BLOCK, s, reinterpret_cast<const float4*>(recs), root, num, n, n_passes, st, labels, keys,
              hist, grp, reinterpret_cast<CmClusterDev*>(clusters));
}
void cmk_cl_decode(hipStream_t s, void* clusters, uint32_t n_clusters) {
    if (n_clusters == 0) return;
    CM_LAUNCH(k_cl_decode, (n_clusters * 6u + CM_BLOCK - 1) / CM_BLOCK, CM_BLOCK, s, reinterpret_cast<CmClusterDev*>(clusters),
              n_clusters);
}
