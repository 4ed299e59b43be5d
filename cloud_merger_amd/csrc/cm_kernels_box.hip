// cm_kernels_box.hip — oriented bounding boxes of the clusters (search-based L-shape fitting), for gfx950.
//
// A by-product computed on request after a frame (cm_result_cluster_boxes), never part of one. It reads the result records
// and the cluster tables of the call (cluster table, member lists) and writes into buffers of its own only (DESIGN.md §19;
// the semantics are in include/cloudmerge.h).
//
// A thread is a heading: thread a of a workgroup holds (cos, sin) of angle a, the four extremes of the members' projections
// and the chunk's sequential sum in registers, and nothing crosses lanes before the choice. The members are walked in chunks
// of CM_BOX_CHUNK, staged as (dx, dy) in 2 KB of LDS and read back as broadcasts.
//
//   k_box_fit       one workgroup per cluster. An invalid cluster gets its NaN entry. A cluster of up to `split` members is
//                   fitted here from start to finish: the extremes over all chunks, then the sums chunk by chunk, then the
//                   choice. A larger one is listed instead: a slot (atomic counter), a run of chunk rows (second counter),
//                   one work item per chunk, and the empty images of its extremes.
//   k_box_extremes  one workgroup per listed chunk: the chunk's extremes per angle into the cluster's images (atomicMin /
//                   atomicMax on order-preserving integer images, f2ord / ord2f of cm_search.hpp: order-free).
//   k_box_sums      one workgroup per listed chunk (CLOSENESS only): the chunk's sum per angle into the chunk's row.
//   k_box_choose    one workgroup per listed cluster: the rows added in ascending chunk order, then the choice.
//
// Which slot and which rows a large cluster gets depends on arrival order; nothing observable does: a row is read only
// through its cluster's list entry. min / max are order-free, every sum has the order the header defines, so an entry is the
// same bytes on either route.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

// The cluster table after k_cl_decode: cm_cluster.
struct BoxCluster {
    uint32_t first, n_voxels, n_points, _pad;
    float mn[3], mx[3];
};
static_assert(sizeof(BoxCluster) == sizeof(CmClusterDev), "the cluster table's entry");

struct BoxExt {
    float u0, u1, v0, v1;
};

__device__ __forceinline__ bool box_valid(const BoxCluster& cl) {
    const float ex = __fsub_rn(cl.mx[0], cl.mn[0]), ey = __fsub_rn(cl.mx[1], cl.mn[1]), ez = __fsub_rn(cl.mx[2], cl.mn[2]);
    return isfinite(ex) && isfinite(ey) && isfinite(ez) && ex < CM_BOX_MAX_EXTENT_DEV && ey < CM_BOX_MAX_EXTENT_DEV;
}

// Members p0 .. p0 + cnt - 1 of the list `idx` as (dx, dy) into sd. Every thread of the workgroup calls it.
__device__ __forceinline__ void box_stage(const float4* __restrict__ recs, const uint32_t* __restrict__ idx, uint32_t cnt,
                                          float mnx, float mny, float2* sd) {
    for (uint32_t t = threadIdx.x; t < cnt; t += blockDim.x) {
        const float4 p = recs[idx[t]];
        sd[t] = make_float2(__fsub_rn(p.x, mnx), __fsub_rn(p.y, mny));
    }
}

__device__ __forceinline__ void box_project(float2 d, float ca, float sa, float* u, float* v) {
    *u = __fadd_rn(__fmul_rn(d.x, ca), __fmul_rn(d.y, sa));
    *v = __fsub_rn(__fmul_rn(d.y, ca), __fmul_rn(d.x, sa));
}

__device__ __forceinline__ void box_chunk_extremes(const float2* sd, uint32_t cnt, float ca, float sa, BoxExt* e) {
    for (uint32_t p = 0; p < cnt; ++p) {
        float u, v;
        box_project(sd[p], ca, sa, &u, &v);
        e->u0 = fminf(e->u0, u); e->u1 = fmaxf(e->u1, u);
        e->v0 = fminf(e->v0, v); e->v1 = fmaxf(e->v1, v);
    }
}

// The chunk's terms added one after the other from 0.0, in list order.
__device__ __forceinline__ double box_chunk_sum(const float2* sd, uint32_t cnt, float ca, float sa, const BoxExt& e, float d_min) {
    double s = 0.0;
    for (uint32_t p = 0; p < cnt; ++p) {
        float u, v;
        box_project(sd[p], ca, sa, &u, &v);
        const float du = fminf(__fsub_rn(e.u1, u), __fsub_rn(u, e.u0));
        const float dv = fminf(__fsub_rn(e.v1, v), __fsub_rn(v, e.v0));
        const float d = fmaxf(fminf(du, dv), d_min);
        s = __dadd_rn(s, __ddiv_rn(1.0, static_cast<double>(d)));
    }
    return s;
}

__device__ __forceinline__ double box_area_score(const BoxExt& e) {
    return -static_cast<double>(__fmul_rn(__fsub_rn(e.u1, e.u0), __fsub_rn(e.v1, e.v0)));
}

__device__ __forceinline__ void box_write_invalid(CmBoxDev* out) {
    const float nan = __uint_as_float(0x7FC00000u);
    CmBoxDev b;
    b.center[0] = b.center[1] = b.center[2] = nan;
    b.size[0] = b.size[1] = b.size[2] = nan;
    b.yaw = nan;
    b.angle = 0;
    b.score = __longlong_as_double(0x7FF8000000000000ll);
    b.flags = 0;
    b._pad = 0;
    *out = b;
}

// The smallest angle with the largest score among the workgroup's active threads; that thread writes the entry. Every
// thread of the workgroup calls it.
__device__ __forceinline__ void box_choose(bool active, uint32_t a, double score, const BoxExt& e, float ca, float sa,
                                           const BoxCluster& cl, double step, CmBoxDev* out) {
    __shared__ double s_score[CM_WAVES];
    __shared__ uint32_t s_angle[CM_WAVES];
    double bs = active ? score : -__builtin_huge_val();
    uint32_t ba = active ? a : 0xFFFFFFFFu;
#pragma unroll
    for (int st = 1; st < 64; st <<= 1) {
        const double os = __shfl_xor(bs, st);
        const uint32_t oa = static_cast<uint32_t>(__shfl_xor(static_cast<int>(ba), st));
        if (os > bs || (os == bs && oa < ba)) { bs = os; ba = oa; }
    }
    const uint32_t wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    if ((threadIdx.x & 63u) == 0) { s_score[wave] = bs; s_angle[wave] = ba; }
    __syncthreads();
    bs = s_score[0]; ba = s_angle[0];
    for (uint32_t w = 1; w < n_waves; ++w) {
        const double os = s_score[w];
        const uint32_t oa = s_angle[w];
        if (os > bs || (os == bs && oa < ba)) { bs = os; ba = oa; }
    }
    if (!active || a != ba) return;
    const float su = __fsub_rn(e.u1, e.u0), sv = __fsub_rn(e.v1, e.v0), ez = __fsub_rn(cl.mx[2], cl.mn[2]);
    const float uc = __fadd_rn(e.u0, __fmul_rn(su, 0.5f)), vc = __fadd_rn(e.v0, __fmul_rn(sv, 0.5f));
    CmBoxDev b;
    b.center[0] = __fadd_rn(cl.mn[0], __fsub_rn(__fmul_rn(uc, ca), __fmul_rn(vc, sa)));
    b.center[1] = __fadd_rn(cl.mn[1], __fadd_rn(__fmul_rn(uc, sa), __fmul_rn(vc, ca)));
    b.center[2] = __fadd_rn(cl.mn[2], __fmul_rn(ez, 0.5f));
    b.size[0] = su; b.size[1] = sv; b.size[2] = ez;
    b.yaw = static_cast<float>(__dmul_rn(static_cast<double>(a), step));
    b.angle = a;
    b.score = score;
    b.flags = CM_BOX_VALID_DEV;
    b._pad = 0;
    *out = b;
}

// words: [0] listed clusters, [1] listed chunks (both zeroed before the launch). list: (cluster, first chunk row) per slot.
// work: (slot, chunk of the cluster) per chunk row. ext: n_angles x (u0, u1, v0, v1) images per slot.
__global__ __launch_bounds__(CM_BLOCK) void k_box_fit(const float4* __restrict__ recs, const BoxCluster* __restrict__ clusters,
                                                      const uint32_t* __restrict__ indices, const float2* __restrict__ dirs,
                                                      uint32_t n_angles, double step, uint32_t criterion, float d_min,
                                                      uint32_t split, CmBoxDev* __restrict__ boxes, uint32_t* __restrict__ words,
                                                      uint2* __restrict__ list, uint2* __restrict__ work, uint4* __restrict__ ext) {
    __shared__ float2 sd[CM_BOX_CHUNK_DEV];
    __shared__ uint32_t s_slot[2];
    const uint32_t k = blockIdx.x;
    const BoxCluster cl = clusters[k];
    if (!box_valid(cl)) {                                   // workgroup-uniform
        if (threadIdx.x == 0) box_write_invalid(&boxes[k]);
        return;
    }
    const uint32_t m = cl.n_voxels, n_chunks = (m + CM_BOX_CHUNK_DEV - 1) / CM_BOX_CHUNK_DEV;
    if (m > split) {
        if (threadIdx.x == 0) {
            const uint32_t slot = atomicAdd(&words[0], 1u), row = atomicAdd(&words[1], n_chunks);
            list[slot] = make_uint2(k, row);
            s_slot[0] = slot; s_slot[1] = row;
        }
        __syncthreads();
        const uint32_t slot = s_slot[0], row = s_slot[1];
        for (uint32_t ch = threadIdx.x; ch < n_chunks; ch += blockDim.x) work[row + ch] = make_uint2(slot, ch);
        for (uint32_t a = threadIdx.x; a < n_angles; a += blockDim.x)
            ext[static_cast<size_t>(slot) * n_angles + a] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);
        return;
    }
    const uint32_t a = threadIdx.x;
    const bool active = a < n_angles;
    const float2 cs = active ? dirs[a] : make_float2(1.0f, 0.0f);
    const uint32_t* idx = indices + cl.first;
    const float inf = __uint_as_float(0x7F800000u);
    BoxExt e = {inf, -inf, inf, -inf};
    for (uint32_t ch = 0; ch < n_chunks; ++ch) {
        const uint32_t p0 = ch * CM_BOX_CHUNK_DEV, cnt = min(m - p0, static_cast<uint32_t>(CM_BOX_CHUNK_DEV));
        if (ch) __syncthreads();
        box_stage(recs, idx + p0, cnt, cl.mn[0], cl.mn[1], sd);
        __syncthreads();
        box_chunk_extremes(sd, cnt, cs.x, cs.y, &e);
    }
    double score;
    if (criterion == CM_BOX_CLOSENESS_DEV) {
        score = 0.0;
        for (uint32_t ch = 0; ch < n_chunks; ++ch) {
            const uint32_t p0 = ch * CM_BOX_CHUNK_DEV, cnt = min(m - p0, static_cast<uint32_t>(CM_BOX_CHUNK_DEV));
            if (n_chunks > 1) {                             // (a single chunk is still staged)
                __syncthreads();
                box_stage(recs, idx + p0, cnt, cl.mn[0], cl.mn[1], sd);
                __syncthreads();
            }
            score = __dadd_rn(score, box_chunk_sum(sd, cnt, cs.x, cs.y, e, d_min));
        }
    } else {
        score = box_area_score(e);
    }
    box_choose(active, a, score, e, cs.x, cs.y, cl, step, &boxes[k]);
}

// The listed chunk of this workgroup: false beyond the list. Workgroup-uniform.
__device__ __forceinline__ bool box_work_item(const uint32_t* __restrict__ words, const uint2* __restrict__ list,
                                              const uint2* __restrict__ work, const BoxCluster* __restrict__ clusters,
                                              uint32_t* slot, uint32_t* p0, uint32_t* cnt, BoxCluster* cl) {
    if (blockIdx.x >= words[1]) return false;
    const uint2 w = work[blockIdx.x];
    *slot = w.x;
    *cl = clusters[list[w.x].x];
    *p0 = w.y * CM_BOX_CHUNK_DEV;
    *cnt = min(cl->n_voxels - *p0, static_cast<uint32_t>(CM_BOX_CHUNK_DEV));
    return true;
}

__global__ __launch_bounds__(CM_BLOCK) void k_box_extremes(const float4* __restrict__ recs, const BoxCluster* __restrict__ clusters,
                                                           const uint32_t* __restrict__ indices, const float2* __restrict__ dirs,
                                                           uint32_t n_angles, const uint32_t* __restrict__ words,
                                                           const uint2* __restrict__ list, const uint2* __restrict__ work,
                                                           uint32_t* __restrict__ ext) {
    __shared__ float2 sd[CM_BOX_CHUNK_DEV];
    uint32_t slot, p0, cnt;
    BoxCluster cl;
    if (!box_work_item(words, list, work, clusters, &slot, &p0, &cnt, &cl)) return;
    box_stage(recs, indices + cl.first + p0, cnt, cl.mn[0], cl.mn[1], sd);
    __syncthreads();
    const uint32_t a = threadIdx.x;
    if (a >= n_angles) return;
    const float2 cs = dirs[a];
    const float inf = __uint_as_float(0x7F800000u);
    BoxExt e = {inf, -inf, inf, -inf};
    box_chunk_extremes(sd, cnt, cs.x, cs.y, &e);
    uint32_t* w = ext + (static_cast<size_t>(slot) * n_angles + a) * 4;
    atomicMin(&w[0], f2ord(e.u0)); atomicMax(&w[1], f2ord(e.u1));
    atomicMin(&w[2], f2ord(e.v0)); atomicMax(&w[3], f2ord(e.v1));
}

__device__ __forceinline__ BoxExt box_load_ext(const uint4* __restrict__ ext, uint32_t slot, uint32_t n_angles, uint32_t a) {
    const uint4 w = ext[static_cast<size_t>(slot) * n_angles + a];
    return {ord2f(w.x), ord2f(w.y), ord2f(w.z), ord2f(w.w)};
}

__global__ __launch_bounds__(CM_BLOCK) void k_box_sums(const float4* __restrict__ recs, const BoxCluster* __restrict__ clusters,
                                                       const uint32_t* __restrict__ indices, const float2* __restrict__ dirs,
                                                       uint32_t n_angles, float d_min, const uint32_t* __restrict__ words,
                                                       const uint2* __restrict__ list, const uint2* __restrict__ work,
                                                       const uint4* __restrict__ ext, double* __restrict__ sums) {
    __shared__ float2 sd[CM_BOX_CHUNK_DEV];
    uint32_t slot, p0, cnt;
    BoxCluster cl;
    if (!box_work_item(words, list, work, clusters, &slot, &p0, &cnt, &cl)) return;
    box_stage(recs, indices + cl.first + p0, cnt, cl.mn[0], cl.mn[1], sd);
    __syncthreads();
    const uint32_t a = threadIdx.x;
    if (a >= n_angles) return;
    const float2 cs = dirs[a];
    const BoxExt e = box_load_ext(ext, slot, n_angles, a);
    sums[static_cast<size_t>(blockIdx.x) * n_angles + a] = box_chunk_sum(sd, cnt, cs.x, cs.y, e, d_min);
}

__global__ __launch_bounds__(CM_BLOCK) void k_box_choose(const BoxCluster* __restrict__ clusters, const float2* __restrict__ dirs,
                                                         uint32_t n_angles, double step, uint32_t criterion,
                                                         const uint32_t* __restrict__ words, const uint2* __restrict__ list,
                                                         const uint4* __restrict__ ext, const double* __restrict__ sums,
                                                         CmBoxDev* __restrict__ boxes) {
    const uint32_t slot = blockIdx.x;
    if (slot >= words[0]) return;
    const uint2 item = list[slot];
    const BoxCluster cl = clusters[item.x];
    const uint32_t n_chunks = (cl.n_voxels + CM_BOX_CHUNK_DEV - 1) / CM_BOX_CHUNK_DEV;
    const uint32_t a = threadIdx.x;
    const bool active = a < n_angles;
    float2 cs = make_float2(1.0f, 0.0f);
    BoxExt e = {0.0f, 0.0f, 0.0f, 0.0f};
    double score = 0.0;
    if (active) {
        cs = dirs[a];
        e = box_load_ext(ext, slot, n_angles, a);
        if (criterion == CM_BOX_CLOSENESS_DEV) {
            for (uint32_t ch = 0; ch < n_chunks; ++ch) score = __dadd_rn(score, sums[static_cast<size_t>(item.y + ch) * n_angles + a]);
        } else {
            score = box_area_score(e);
        }
    }
    box_choose(active, a, score, e, cs.x, cs.y, cl, step, &boxes[item.x]);
}

}  // namespace

// One thread per heading, whole waves: CM_BOX_MAX_ANGLES_DEV <= CM_BLOCK.
static uint32_t box_block(uint32_t n_angles) { return (n_angles + 63u) / 64u * 64u; }
static_assert(CM_BOX_MAX_ANGLES_DEV <= CM_BLOCK, "a workgroup holds every heading");

void cmk_box_fit(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, uint32_t n_clusters,
                 const void* dirs, uint32_t n_angles, double step, uint32_t criterion, float d_min, uint32_t split, void* boxes,
                 uint32_t* words, void* list, void* work, void* ext) {
    if (n_clusters == 0) return;
    CM_LAUNCH(k_box_fit, n_clusters, box_block(n_angles), s, reinterpret_cast<const float4*>(recs),
              reinterpret_cast<const BoxCluster*>(clusters), indices, reinterpret_cast<const float2*>(dirs), n_angles, step, criterion,
              d_min, split, reinterpret_cast<CmBoxDev*>(boxes), words, reinterpret_cast<uint2*>(list), reinterpret_cast<uint2*>(work),
              reinterpret_cast<uint4*>(ext));
}
void cmk_box_extremes(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, const void* dirs,
                      uint32_t n_angles, const uint32_t* words, const void* list, const void* work, void* ext, uint32_t max_chunks) {
    if (max_chunks == 0) return;
    CM_LAUNCH(k_box_extremes, max_chunks, box_block(n_angles), s, reinterpret_cast<const float4*>(recs),
              reinterpret_cast<const BoxCluster*>(clusters), indices, reinterpret_cast<const float2*>(dirs), n_angles, words,
              reinterpret_cast<const uint2*>(list), reinterpret_cast<const uint2*>(work), reinterpret_cast<uint32_t*>(ext));
}
void cmk_box_sums(hipStream_t s, const void* recs, const void* clusters, const uint32_t* indices, const void* dirs, uint32_t n_angles,
                  float d_min, const uint32_t* words, const void* list, const void* work, const void* ext, double* sums,
                  uint32_t max_chunks) {
    if (max_chunks == 0) return;
    CM_LAUNCH(k_box_sums, max_chunks, box_block(n_angles), s, reinterpret_cast<const float4*>(recs),
              reinterpret_cast<const BoxCluster*>(clusters), indices, reinterpret_cast<const float2*>(dirs), n_angles, d_min, words,
              reinterpret_cast<const uint2*>(list), reinterpret_cast<const uint2*>(work), reinterpret_cast<const uint4*>(ext), sums);
}
void cmk_box_choose(hipStream_t s, const void* clusters, const void* dirs, uint32_t n_angles, double step, uint32_t criterion,
                    const uint32_t* words, const void* list, const void* ext, const double* sums, void* boxes, uint32_t max_large) {
    if (max_large == 0) return;
    CM_LAUNCH(k_box_choose, max_large, box_block(n_angles), s, reinterpret_cast<const BoxCluster*>(clusters),
              reinterpret_cast<const float2*>(dirs), n_angles, step, criterion, words, reinterpret_cast<const uint2*>(list),
              reinterpret_cast<const uint4*>(ext), sums, reinterpret_cast<CmBoxDev*>(boxes));
}
