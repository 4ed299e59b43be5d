// cm_kernels_v3.hip — the voxel finish of the bucket path, second generation (gfx950).
//
// Same contract as k2_local (cm_kernels_v2.hip): `rec` is grouped by H = key >> low_bits, ascending, stable;
// workgroup t owns the buckets that START inside records [t*LT, (t+1)*LT) and turns them into pcl::VoxelGrid
// centroids (ascending voxel index, a voxel's points added in stable order starting
// from 0.0f, kept iff count >= min_points_per_voxel). What changed, and why (VERDICT r1 "next" item 1):
//
//   * no ticket and no look-back. A tile does not need to know where its centroids go: it writes them at
//     stage[t*LT + a + j] — the owned ranges [t*LT + a, ...) of the tiles partition the array, so these places
//     are disjoint — leaves (a, kept) in tile_info and adds `kept` to the total of its group of 64 tiles.
//     k3_compact then copies every tile's centroids to out[prefix(t) ...] (11 MB at cfg2; it also reports the
//     frame). A tile never waits for another one; which workgroup runs when no longer matters.
//   * the per-voxel sums are fused into the voxel list. k2_local built a voxel table, scanned it a second time for the
//     kept voxels and then let one lane per kept voxel walk its points through dependent L2 loads. Here a thread
//     takes a block of consecutive sorted positions, finds the heads in it, tests each head for min_pts with one
//     key look-up, fetches the records of its kept voxels together (one L2 latency) and adds them up in registers;
//     only a voxel that runs past the end of its block costs further (pipelined) loads. One scan, no voxel tables.
//     (Measured and rejected: accumulating with LDS float atomics. ds_add_f32 does add the lanes of an instruction
//     in lane order with round-to-nearest adds — scripts/micro/lds_fadd_order.hip, 633 344 sums, no difference to a
//     sequential chain — but it takes ~200-250 cycles per wave instruction against 4 for ds_add_u32
//     (scripts/micro/lds_atomic_rate.hip) and holds the CU's LDS pipe meanwhile: k3_local 89 us against 39.)
//   * the order the global passes left is checked: H must not decrease from one record to the
//     next; a violation raises CM_DEV_ERR_UNSORTED and the frame is handed back (cm_launch.cpp wait_frame).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"

namespace {

// Sum of a float over the wave in a fixed order (the DPP ladder of wave_incl_scan_u32: rows of 16, then across rows),
// the same in every lane. Deterministic; NOT the sequential order — used for long runs only (see the long-run jobs).
__device__ __forceinline__ float wave_sum_f32_fixed(float v) {
#define CM3_FADD(ctrl, rmask) v = __fadd_rn(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rmask, 0xf, false)))
    CM3_FADD(0x111, 0xf); CM3_FADD(0x112, 0xf); CM3_FADD(0x114, 0xf); CM3_FADD(0x118, 0xf);
    CM3_FADD(0x142, 0xa); CM3_FADD(0x143, 0xc);
#undef CM3_FADD
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

#define SCAL(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))

struct Job3 {                      // a voxel that runs far past its owner's block: finished by a whole wave
    uint32_t p, key, kid, cnt;     // next sorted position, the voxel's key, its number among the tile's kept voxels, points so far
    float sx, sy, sz, sw;          // sums so far
};
#define CM3_EXT_SEQ 16u            // positions past its block a thread still adds one after the other
#define CM3_RUN_MAX (1u << 20)     // a voxel with more points than this goes back to the general path (parallel tree sums)

// Phase timing of the finish (scripts/phase_times3.py; cm_common.hpp).
CM_PHASE_DECLARE(g_phase_k3);

// ------------------------------------------------------------------------------------------------
// k3_local
// ------------------------------------------------------------------------------------------------
template <int LT, int LCAP, int LBLOCK, int WPS, bool PARTIAL, bool QUANT, bool BALLOT, bool SUB>
__global__ __launch_bounds__(LBLOCK, WPS) void k3_local(const CmFrameDev* __restrict__ fd,
                                                      CmFrameState* __restrict__ st,
                                                      uint32_t* __restrict__ host_state,
                                                      const float4* __restrict__ rec,
                                                      uint2* __restrict__ tile_info,
                                                      uint32_t* __restrict__ grp_cnt,
                                                      float4* __restrict__ stage,
                                                      uint32_t* __restrict__ stage_key,
                                                      uint32_t* __restrict__ stage_cnt,
                                                      uint32_t low_bits,
                                                      const uint32_t* __restrict__ spl, const uint32_t* __restrict__ bofs,
                                                      uint32_t n_buckets, uint32_t* __restrict__ spl_next,
                                                      const uint32_t* __restrict__ big_list, uint32_t sub_shift,
                                                      const unsigned char* __restrict__ dig) {
    // SUB (QUANT, shared bins: cm_device.h cm_quant_sub_shift): the global pass grouped the records by bucket >> sub_shift, so
    // bucket t's records lie among those of bin t >> sub_shift = records [bofs[bin], bofs[bin + 1]), in stable order, each
    // with the low bits of its bucket number as a byte beside it (dig). The workgroup reads the bin's bytes, notes the places
    // of its own records (sp: the "slot" of a record is its number among them) and counts the records of the buckets BELOW
    // its own: that is where its records would start had the pass grouped by bucket, and where its centroids are staged.
    // The 2^sub_shift workgroups of a bin are neighbours on one XCD (its lines come out of that XCD's L2 after the first read).
    // big_list (QUANT): word 0 = how many buckets hold more than CM4_CAP records, then their numbers (k4_colscan). The usual
    // launch (big_list == nullptr) leaves those alone; a second launch of the LARGE shape (1024 threads, room for CM4_CAP_BIG
    // records) takes them, workgroup i the i-th of the list: a bucket that doubled or tripled since the last frame costs a
    // slower workgroup, not a handed-back frame.
    // QUANT (cm_kernels_v4.hip): the records are grouped by quantile bucket — workgroup t takes bucket t, records
    // [bofs[t], bofs[t+1]) with indices in [spl[t], spl[t+1]): no bucket boundaries to look for, no tail to follow.
    // spl_next: where the next frame's splitters go (every tile writes the quantiles that fall into its sorted range).
    constexpr int LWAVES = LBLOCK / 64, LITEMS = (LCAP + LBLOCK - 1) / LBLOCK, EXT0 = LBLOCK < 256 ? LBLOCK : 256;
    // (SUB: 9-bit digits — with the slots' places (sp) beside them 1024 counters per wave would leave room for three
    // workgroups per CU instead of four)
    constexpr int WB = SUB ? 9 : 10, BINS = 1 << WB, HWORDS = BINS / 2;          // two 16-bit counters per LDS word
    constexpr uint32_t MAXJ = LWAVES * HWORDS * 4 / sizeof(Job3);                  // jobs that fit where the counters were
    static_assert(LT == 4 * LBLOCK && LCAP <= 0x7FFE && HWORDS <= LBLOCK && LWAVES * HWORDS * 2 >= LCAP, "tile geometry");
    static_assert(LITEMS % 4 == 0 && HWORDS >= 64, "the returning adds go out in groups of four; a slot without a record adds to word `lane`");
    __shared__ uint32_t sk[LCAP];                      // key of every slot
    __shared__ uint16_t si[LCAP];                      // slots in sorted order
    __shared__ uint32_t whist[LWAVES][HWORDS];         // digit counts per wave
    __shared__ uint32_t lds[2 * LWAVES];
    __shared__ uint32_t s_a, s_keyprev, s_bad, s_njobs;
    __shared__ uint16_t sp[SUB ? LCAP : 1];            // (SUB) slot -> place in the bin
    static_assert(!SUB || QUANT, "shared bins are a variant of the quantile finish");
    Job3* jobs = reinterpret_cast<Job3*>(&whist[0][0]);         // (the counters are dead once the sort is over: 512 jobs fit)

    if (QUANT && big_list && blockIdx.x >= big_list[0]) return;        // (the large shape's launch: usually nothing to do — leave at once)
    PH_START();
    // (values that are the same in every lane are put into scalar registers by hand — the compiler cannot tell for what
    // comes out of LDS or global memory — so that the loops below branch and count on the scalar unit)
    const int lane = threadIdx.x & 63;
    const uint32_t w = SCAL(threadIdx.x >> 6);
    if (st->status != CM_DEV_OK || st->outside) return;          // (k3_compact reports)
    if (QUANT && st->quant_abort) return;
    const uint32_t n = SCAL(st->n_valid);
    const uint32_t n_lt = QUANT ? n_buckets : (n + LT - 1) / LT;
    uint32_t tile_ = blockIdx.x;
    if (SUB) {                                                   // workgroups 8j + x run on XCD x: bin (j >> shift) * 8 + x, bucket j % 2^shift of it
        const uint32_t x = blockIdx.x & 7u, j = blockIdx.x >> 3;
        tile_ = (((((j >> sub_shift) << 3) + x) << sub_shift) + (j & ((1u << sub_shift) - 1u)));
    }
    if (QUANT && big_list) {
        if (tile_ >= SCAL(big_list[0])) return;
        tile_ = SCAL(big_list[1 + tile_]);
    }
    const uint32_t tile = tile_;
    if (tile >= n_lt) return;
    const BoxGrid b = box_grid_of(fd);
    const uint32_t L = QUANT ? 1u : low_bits;                    // (QUANT: only "there is something left to sort")
    const uint32_t min_pts = SCAL((!PARTIAL && fd->min_pts > 1) ? fd->min_pts : 1u);

    // ---- load: the nominal tile, the key before it, and the first records after it
    const uint32_t bin = SUB ? tile >> sub_shift : tile;
    uint32_t base = QUANT ? SCAL(bofs[bin]) : tile * LT;
    const uint32_t rbase = base;                                 // slot s is record rbase + s (SUB: rbase + sp[s])
    const float4* __restrict__ recb = rec + rbase;               // (a scalar base: the slot is a 32-bit offset of the load)
    const uint32_t q_end = QUANT ? SCAL(bofs[bin + 1]) : 0u;
    bool q_big = QUANT && !SUB && (q_end - base) > static_cast<uint32_t>(LCAP);
    if (QUANT && q_big && !big_list && (q_end - base) <= CM4_CAP_BIG) return;     // (the large shape's launch takes this bucket)
    uint32_t nom = QUANT ? (q_big ? 0u : q_end - base) : min(static_cast<uint32_t>(LT), n - base);
    const uint32_t key_end = QUANT ? (fd->box_key_bits < 32u ? (1u << fd->box_key_bits) : 0xFFFFFFFFu) : 0u;
    const uint32_t q_lo = QUANT ? SCAL(spl[tile]) : 0u;
    const uint32_t q_hi = QUANT ? min(SCAL(spl[tile + 1]), key_end) : 0u;
    bool q_bad = false;
    if (SUB) {
        // dig[p] (k4_scatter): which of its bin's buckets record p belongs to. Sixteen places per thread and round, in order:
        // the kept records keep the bin's (stable) order. Nothing but these bytes is read of the other buckets' records.
        const uint32_t sub = tile & ((1u << sub_shift) - 1u);
        uint32_t kept = 0, below_t = 0;
        for (uint32_t off = rbase & ~15u; off < q_end; off += 16 * LBLOCK) {
            const uint32_t p0 = off + 16 * threadIdx.x;
            uint4 d = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (p0 < q_end) d = *reinterpret_cast<const uint4*>(dig + p0);
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
            uint32_t mm = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t p = p0 + i, v = (dw[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                const bool valid = p >= rbase && p < q_end;
                mm |= (valid && v == sub) ? (1u << i) : 0u;
                below_t += (valid && v < sub) ? 1u : 0u;
            }
            uint32_t tot;
            uint32_t pos = kept + block_excl_scan<LWAVES>(static_cast<uint32_t>(__builtin_popcount(mm)), lds, &tot);
            while (mm) {
                const uint32_t i = static_cast<uint32_t>(__builtin_ctz(mm));
                mm &= mm - 1u;
                if (pos < static_cast<uint32_t>(LCAP)) sp[pos] = static_cast<uint16_t>(p0 + i - rbase);
                ++pos;
            }
            kept += SCAL(tot);
        }
        uint32_t below;
        (void)block_excl_scan<LWAVES>(below_t, lds, &below);
        base = rbase + SCAL(below);
        q_big = kept > static_cast<uint32_t>(LCAP);          // (no large shape behind this one: the frame is handed back)
        nom = q_big ? 0u : kept;
        __syncthreads();
    }
    if (QUANT) {
        // (a bucket holds about 1950 records: four rounds of the workgroup, then — rarely — up to four more)
        constexpr int HALF = LITEMS / 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && nom <= static_cast<uint32_t>(HALF * LBLOCK)) break;     // (uniform)
            float4 r4[HALF];
            // (a wave whose slots of the half's last round all hold a record — one scalar compare — runs the half straight
            // through: no test per lane, the loads and then the stores one behind the other)
            if ((h * HALF + HALF - 1) * LBLOCK + w * 64u + 64u <= nom) {
                uint32_t pl[HALF];
#pragma unroll
                for (int r = 0; r < HALF; ++r) {
                    const uint32_t q = (h * HALF + r) * LBLOCK + threadIdx.x;
                    pl[r] = SUB ? sp[q] : q;
                }
#pragma unroll
                for (int r = 0; r < HALF; ++r) r4[r] = recb[pl[r]];
#pragma unroll
                for (int r = 0; r < HALF; ++r) {
                    const uint32_t k = key_of(b, r4[r]);
                    sk[(h * HALF + r) * LBLOCK + threadIdx.x] = k;
                    q_bad = q_bad | (k < q_lo) | (k >= q_hi);    // (the scatter put a record into a bucket that is not its own)
                }
            } else {
#pragma unroll
                for (int r = 0; r < HALF; ++r) {
                    const uint32_t q = (h * HALF + r) * LBLOCK + threadIdx.x;
                    r4[r] = (q < nom) ? rec[rbase + (SUB ? sp[q < nom ? q : 0u] : q)] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int r = 0; r < HALF; ++r) {
                    const uint32_t q = (h * HALF + r) * LBLOCK + threadIdx.x;
                    if (q < nom) {
                        const uint32_t k = key_of(b, r4[r]);
                        sk[q] = k;
                        q_bad = q_bad || k < q_lo || k >= q_hi;
                    }
                }
            }
        }
        if (threadIdx.x == 0) { s_keyprev = 0u; s_a = 0u; s_bad = 0u; s_njobs = 0u; }
    } else {
        float4 r4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t q = r * LBLOCK + threadIdx.x;
            r4[r] = (q < nom) ? rec[base + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const uint32_t j0 = base + LT + threadIdx.x;
        const bool has_e = threadIdx.x < EXT0 && nom == LT && j0 < n;
        const float4 e4 = has_e ? rec[j0] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (threadIdx.x == 0 && base > 0) pv = rec[base - 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t q = r * LBLOCK + threadIdx.x;
            if (q < nom) sk[q] = key_of(b, r4[r]);
        }
        if (has_e) sk[LT + threadIdx.x] = key_of(b, e4);
        if (threadIdx.x == 0) { s_keyprev = base > 0 ? key_of(b, pv) : 0u; s_a = 0xFFFFFFFFu; s_bad = 0u; s_njobs = 0u; }
    }
    __syncthreads();
    PH(g_phase_k3, 0);

    // ---- a: first bucket start in the nominal tile; H must not decrease anywhere (free check of the global passes)
    bool bad_order = q_bad;
    if (!QUANT) {
        uint32_t best = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 3; r >= 0; --r) {
            const uint32_t q = r * LBLOCK + threadIdx.x;
            if (q < nom) {
                const uint32_t kp = (q == 0) ? s_keyprev : sk[q - 1];
                const uint32_t hq = sk[q] >> L, hp = kp >> L;
                if ((base + q == 0) || (hq != hp)) best = q;
                bad_order = bad_order || (base + q > 0 && hq < hp);
            }
        }
        if (best != 0xFFFFFFFFu) atomicMin(&s_a, best);
    }
    const uint32_t h_last = QUANT ? 0u : SCAL(sk[nom - 1] >> L);
    // ---- tail of the last bucket past the nominal end (a prefix of what follows: H is ascending)
    const bool in_e = !QUANT && threadIdx.x < EXT0 && nom == LT && (base + LT + threadIdx.x) < n;
    const bool m0 = in_e && (sk[LT + threadIdx.x] >> L) == h_last;
    bad_order = bad_order || (in_e && (sk[LT + threadIdx.x] >> L) < h_last);
    uint32_t ext = QUANT ? 0u : SCAL(__syncthreads_count(m0));         // also orders the atomicMin above
    const uint32_t a = SCAL(s_a);
    // With no bits left to sort (L == 0: a bucket is ONE voxel, its records already in their final order) a voxel need not
    // fit: what LDS cannot hold is read straight from HBM when its sum is finished ("open tail", the long-run jobs below).
    const bool may_open = L == 0 && (min_pts - 1u) < static_cast<uint32_t>(LCAP - LT);
    bool too_big = q_big, tail_open = false;
    if (!QUANT && ext == EXT0 && a != 0xFFFFFFFFu) {
        for (uint32_t off = EXT0;; off += LBLOCK) {
            const uint32_t j = base + LT + off + threadIdx.x;
            const uint32_t pos = LT + off + threadIdx.x;
            bool mm = false;
            if (j < n) {
                const float4 r4 = rec[j];
                const uint32_t k = key_of(b, r4);
                mm = (k >> L) == h_last;
                bad_order = bad_order || (k >> L) < h_last;
                if (mm && pos < LCAP) sk[pos] = k;
            }
            const uint32_t c = SCAL(__syncthreads_count(mm));
            ext += c;
            if (LT + ext > LCAP) {
                if (may_open) { tail_open = true; ext = LCAP - LT; } else too_big = true;
                break;
            }
            if (c < LBLOCK) break;
        }
    }
    if (bad_order) s_bad = 1u;
    const uint32_t m = (a == 0xFFFFFFFFu || too_big) ? 0u : nom + ext - a;
    if (too_big && threadIdx.x == 0) host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_BUCKET;

    PH(g_phase_k3, 1);
    // ---- sort the owned slots [a, a+m) by key: LSD over the bits in which the keys of this tile can differ, up to
    // 10 per pass, stable; only the slot numbers move. Ranking: returning LDS adds on per-wave counters.
    if (m && L == 0) {                                         // already in key order: the sorted position IS the slot
        for (uint32_t e = threadIdx.x; e < m; e += LBLOCK) si[e] = static_cast<uint16_t>(a + e);
        __syncthreads();
    }
    if (m && L != 0) {
        const uint32_t h_first = QUANT ? 0u : SCAL(sk[a] >> L);
        const uint32_t kbase = QUANT ? q_lo : h_first << L;
        const unsigned long long span = QUANT ? static_cast<unsigned long long>(q_hi - q_lo)
                                              : static_cast<unsigned long long>(h_last - h_first + 1u) << L;
        const uint32_t nb = span > 1ull ? 64u - static_cast<uint32_t>(__builtin_clzll(span - 1ull)) : 0u;
        const uint32_t npass = nb ? (nb + WB - 1u) / WB : 1u;
        const uint32_t width = nb ? (nb + npass - 1u) / npass : 0u;
        const uint32_t dmask = (1u << width) - 1u;
        const uint32_t rounds = (m + LBLOCK - 1) / LBLOCK;
        // Wave w ranks the positions [w * 64 * rounds, (w + 1) * 64 * rounds): round r, lane l is position e0 + r * 64 + l and
        // holds a record while r * 64 + l < cnt_w. The passes are compiled for R = 4 and R = LITEMS rounds (a bucket of the
        // usual size takes four) as straight-line code: a thread's reads of si, then of sk, then its returning adds — in
        // ascending r: the order of a lane's own records on one counter IS their stable rank — go out one behind the other
        // and are waited for once. A wave whose R rounds are all full (a scalar compare) tests nothing per lane; in any
        // other wave a slot without a record reads a clamped position and adds zero to a word of its own lane (the LDS
        // serialises the adds of a wave that meet on one word).
        const uint32_t e0 = w * (64u * rounds);
        const uint32_t cnt_w = e0 < m ? min(m - e0, 64u * rounds) : 0u;
        auto sort_passes = [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            const bool all_full = R < LITEMS && cnt_w == 64u * R;             // (uniform; the long form always tests)
            for (uint32_t p = 0; p < npass; ++p) {
                const uint32_t wp = nb > p * width ? min(width, nb - p * width) : 0u;     // bits this pass really sorts
                const uint32_t words = wp ? ((1u << wp) + 1u) / 2u : 1u;
                uint32_t ed[R], rk[R];                     // slot (16 bits) | digit << 16; rank among the wave's records of the digit
                auto digits = [&](auto fc) {
                    constexpr bool FULL = decltype(fc)::value;
                    uint32_t kk[R];
                    uint32_t ln = lane;                            // (opaque: what depends on the lane alone is formed in every pass —
                    asm volatile("" : "+v"(ln));                   //  hoisted out of the pass loop it stays live across it and spills)
                    // (these opaque copies, here and in the two phases below, only steer LLVM's hoisting and register
                    // allocation: after any change of the toolchain check scripts/kernel_resources.sh again — 64 VGPRs, no scratch)
                    if (p == 0) {
#pragma unroll
                        for (int r = 0; r < R; ++r) ed[r] = a + (FULL ? e0 + r * 64 + ln : min(e0 + r * 64 + ln, m - 1u));
                    } else {
#pragma unroll
                        for (int r = 0; r < R; ++r) ed[r] = si[FULL ? e0 + r * 64 + ln : min(e0 + r * 64 + ln, m - 1u)];
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) kk[r] = sk[ed[r]];
#pragma unroll
                    for (int r = 0; r < R; ++r) ed[r] |= (((kk[r] - kbase) >> (p * width)) & dmask) << 16;
                };
                if (all_full) digits(std::true_type{}); else digits(std::false_type{});
#pragma unroll
                for (int q = 0; q < LWAVES * HWORDS / LBLOCK; ++q) {
                    const uint32_t flat = q * LBLOCK + threadIdx.x;       // row = flat / HWORDS, column = flat % HWORDS
                    if ((flat & (HWORDS - 1)) < words) (&whist[0][0])[flat] = 0;
                }
                __syncthreads();
                auto ranks = [&](auto fc) {
                    constexpr bool FULL = decltype(fc)::value;
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));
                    if (BALLOT) {
#pragma unroll
                        for (int r = 0; r < R; ++r) {                      // (cm_common.hpp: no returning adds; one record after the other)
                            rk[r] = wave_rank_ballot(whist[w], ed[r] >> 16, wp, FULL || r * 64 + ln < cnt_w, static_cast<int>(ln));
                            asm volatile("" : "+v"(rk[r]));
                        }
                    } else {
#pragma unroll
                        for (int r0 = 0; r0 < R; r0 += 4) {                // (four returns in flight, as k4_scatter)
                            uint32_t got[4];
#pragma unroll
                            for (int r = r0; r < r0 + 4; ++r) {
                                const bool has = FULL || r * 64 + ln < cnt_w;
                                got[r - r0] = atomicAdd(&whist[w][has ? ed[r] >> 17 : ln], (has ? 1u : 0u) << (ed[r] & 0x10000u ? 16u : 0u));
                            }
                            asm volatile("" : "+v"(got[0]), "+v"(got[1]), "+v"(got[2]), "+v"(got[3]));     // (all four asked for before one is used)
#pragma unroll
                            for (int r = r0; r < r0 + 4; ++r) {
                                rk[r] = (got[r - r0] >> (ed[r] & 0x10000u ? 16u : 0u)) & 0xFFFFu;
                                asm volatile("" : "+v"(rk[r]));          // (formed here: the raw returns need not stay alive)
                            }
                        }
                    }
                };
                if (all_full) ranks(std::true_type{}); else ranks(std::false_type{});
                __syncthreads();
                // thread t < words: digits 2t and 2t+1. Totals over the waves, exclusive prefix over the digits (one barrier: the
                // wave totals alternate between two sets of words from pass to pass), then every wave's counter becomes the
                // first sorted position of its items of that digit — 16 bits each, positions stay below LCAP.
                uint32_t cw[LWAVES], t0 = 0, t1 = 0;
                if (threadIdx.x < words) {
#pragma unroll
                    for (int q = 0; q < LWAVES; ++q) { cw[q] = whist[q][threadIdx.x]; t0 += cw[q] & 0xFFFFu; t1 += cw[q] >> 16; }
                }
                uint32_t db;
                {
                    uint32_t* wl = lds + (p & 1u) * LWAVES;
                    const uint32_t incl = wave_incl_scan_u32(t0 + t1, lane);
                    if (lane == 63) wl[w] = incl;
                    __syncthreads();
                    uint32_t woff = 0;
#pragma unroll
                    for (int q = 0; q < LWAVES; ++q) woff += (q < w) ? wl[q] : 0u;
                    db = woff + incl - (t0 + t1);
                }
                if (threadIdx.x < words) {
                    uint32_t r0 = db, r1 = db + t0;
#pragma unroll
                    for (int q = 0; q < LWAVES; ++q) {
                        whist[q][threadIdx.x] = r0 | (r1 << 16);
                        r0 += cw[q] & 0xFFFFu; r1 += cw[q] >> 16;
                    }
                }
                __syncthreads();
                auto place = [&](auto fc) {
                    constexpr bool FULL = decltype(fc)::value;
                    uint32_t first[R];
                    uint32_t ln = lane;
                    asm volatile("" : "+v"(ln));
#pragma unroll
                    for (int r = 0; r < R; ++r) first[r] = whist[w][ed[r] >> 17];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t pos = ((first[r] >> (ed[r] & 0x10000u ? 16u : 0u)) & 0xFFFFu) + rk[r];
                        if (FULL || r * 64 + ln < cnt_w) si[pos] = static_cast<uint16_t>(ed[r]);
                    }
                };
                if (all_full) place(std::true_type{}); else place(std::false_type{});
                __syncthreads();
            }
        };
        if (LITEMS > 4 && rounds <= 4u) sort_passes(std::integral_constant<int, 4>{});
        else sort_passes(std::integral_constant<int, LITEMS>{});
    }
    if (s_bad && threadIdx.x == 0) host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_UNSORTED;
    PH(g_phase_k3, 2);

    // ---- the next frame's splitters (cm_kernels_v4.hip): sorted position e of this tile is record base + a + e of the whole
    // frame in index order; splitter j of bn is the index at record j * Q, Q = ceil(n / bn) (buckets of Q records; the last
    // ones may stay empty). Each is written by the one tile whose range holds it; tile 0 also writes the fixed ends (splitter
    // 0 = index 0, 0xFFFFFFFF from the first bucket without a record on). All of it is wave-uniform 32-bit arithmetic.
    if (!PARTIAL && spl_next) {
        // (a tile whose last voxel runs on beyond its LDS — L = 0 frames only — cannot say which index sits at the positions
        // out there: the frame then leaves no splitters)
        if (tail_open && threadIdx.x == 0) st->spl_incomplete = 1u;
        // (u32 / u32 by a float reciprocal and a correction step: a handful of instructions where the compiler's exact
        // division takes twenty-odd, three times per tile — it showed as 5 us on the fixed-grid finish)
        auto fdiv = [](uint32_t x, uint32_t y) {
            uint32_t q = static_cast<uint32_t>(static_cast<float>(x) * __frcp_rn(static_cast<float>(y)));
            while (static_cast<unsigned long long>(q) * y > x) --q;
            while (static_cast<unsigned long long>(q + 1u) * y <= x) ++q;
            return q;
        };
        const uint32_t bn = SCAL(cm_quant_buckets(n));
        const uint32_t Q = bn ? SCAL(fdiv(n + bn - 1u, bn)) : 1u;
        if (bn && m) {
            const uint32_t g0 = base + a, g1 = g0 + m;
            const uint32_t j_lo = SCAL(fdiv(g0 + Q - 1u, Q));
            for (uint32_t j = j_lo + threadIdx.x; j * Q < g1; j += LBLOCK)          // (g1 <= n: only buckets that hold records)
                spl_next[j] = j ? sk[si[j * Q - g0]] : 0u;
        }
        if (tile == 0) {
            const uint32_t used = bn ? fdiv(n + Q - 1u, Q) : 0u;                     // buckets that hold records (<= bn)
            for (uint32_t j = used + threadIdx.x; j <= CM4_MAX_BUCKETS; j += LBLOCK) spl_next[j] = 0xFFFFFFFFu;
        }
    }

    // ---- voxels. Thread t takes the sorted positions [t*per, (t+1)*per). A head is a position whose key differs from
    // the one before it; its voxel is kept when the position min_pts - 1 further on still has its key (A.4 step 7).
    // A thread owns the voxels whose head lies in its block: it adds their points one after the other, in sorted (=
    // stable) order, starting from 0.0f — pcl's CentroidPoint sum (A.4 step 8) — running past the end of its block
    // where its last voxel does, and skips the positions at the start of its block that continue an earlier thread's
    // voxel. The records of a block are fetched together (they sit in L2: this workgroup has just read them).
    uint32_t c_t = 0;
    {
        const uint32_t per = (m + LBLOCK - 1) / LBLOCK;        // sorted positions per thread (<= LITEMS)
        const uint32_t i0 = threadIdx.x * per;
        auto emit = [&](uint32_t kid, uint32_t key, float sx, float sy, float sz, float sw, uint32_t cn) {
            const size_t o = static_cast<size_t>(base) + a + kid;
            if (PARTIAL) {                                     // cm_partial_entry: key, count, sx, sy | sz, si, 0, 0
                stage[2 * o] = make_float4(__uint_as_float(key), __uint_as_float(cn), sx, sy);
                stage[2 * o + 1] = make_float4(sz, sw, 0.f, 0.f);
            } else {                                           // sums and count; k3_compact divides while it packs
                stage[o] = make_float4(sx, sy, sz, sw);
                stage_cnt[o] = cn;
                if (stage_key) stage_key[o] = key;
            }
        };
        uint32_t kid = 0, cn = 0, ckey = 0;
        float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
        bool on = false;
        // Compiled for R = 4 and R = LITEMS positions per thread, as the sort: the slots and keys of a block (and the key before
        // it) are fetched together, heads, keep and the load mask are bit arithmetic on those registers, and the records of
        // the kept voxels are asked for one behind the other. A thread holds nv of its R positions (all of them in a wave
        // whose whole range lies below m: a scalar compare, and then nothing is clamped or tested); position nv counts as a
        // head, so a run of the block ends there. min_pts: a head at j is kept when the d = min_pts - 1 positions behind it are
        // in the block and none of them is a head; only the block's LAST head can run on past the block, and only for that
        // one the key d positions on is looked up in LDS (the keys are sorted: it is the head's key iff all between are).
        auto voxels = [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            const bool all_full = R < LITEMS && per == static_cast<uint32_t>(R) && (w * 64u + 64u) * R <= m;   // (uniform)
            uint32_t k[R], sl[R];
            uint32_t heads = 0, kheads = 0, ldm = 0;
            float4 r4[R];
            auto front = [&](auto fc) {
                constexpr bool FULL = decltype(fc)::value;
                const uint32_t nv = FULL ? static_cast<uint32_t>(R) : (i0 < m ? min(m - i0, per) : 0u);
                const uint32_t slp = si[i0 ? min(i0 - 1u, m - 1u) : 0u];
#pragma unroll
                for (int j = 0; j < R; ++j) sl[j] = si[FULL ? i0 + j : min(i0 + j, m - 1u)];
                const uint32_t kp = sk[slp];
#pragma unroll
                for (int j = 0; j < R; ++j) k[j] = sk[sl[j]];
                uint32_t klast = 0;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const bool hd = (FULL || static_cast<uint32_t>(j) < nv) && (j ? k[j] != k[j ? j - 1 : 0] : (i0 == 0 || k[0] != kp));
                    heads |= (hd ? 1u : 0u) << j;
                    klast = hd ? k[j] : klast;
                }
                kheads = heads;
                if (min_pts > 1) {                             // (uniform)
                    const uint32_t d = min_pts - 1u;
                    const uint32_t hb = heads | (1u << nv), dm = d >= 16u ? 0xFFFFu : (1u << d) - 1u;
                    kheads = 0;
#pragma unroll
                    for (int j = 0; j < R; ++j) kheads |= (((heads >> j) & 1u) && ((hb >> (j + 1)) & dm) == 0u ? 1u : 0u) << j;
                    const uint32_t jl = heads ? 31u - static_cast<uint32_t>(__builtin_clz(heads)) : 0u;
                    const bool look = heads && !((kheads >> jl) & 1u) && d < m - (i0 + jl);
                    const uint32_t kd = sk[si[look ? i0 + jl + d : 0u]];
                    kheads |= (look && kd == klast ? 1u : 0u) << jl;
                }
                // which of the block's positions belong to a kept voxel with its head in the block: those records are loaded
                uint32_t on_ = 0;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    on_ = ((heads >> j) & 1u) ? (kheads >> j) & 1u : on_;
                    ldm |= ((FULL || static_cast<uint32_t>(j) < nv) ? on_ : 0u) << j;
                }
                uint32_t pl[R];
#pragma unroll
                for (int j = 0; j < R; ++j) pl[j] = SUB ? sp[sl[j]] : sl[j];
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if ((ldm >> j) & 1u) r4[j] = recb[pl[j]];
            };
            if (m) { if (all_full) front(std::true_type{}); else front(std::false_type{}); }
            kid = block_excl_scan<LWAVES>(static_cast<uint32_t>(__builtin_popcount(kheads)), lds, &c_t);
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if ((heads >> j) & 1u) {
                    if (on) emit(kid++, ckey, sx, sy, sz, sw, cn);
                    on = (kheads >> j) & 1u;
                    sx = sy = sz = sw = 0.f; cn = 0;
                    ckey = R <= 4 ? k[j] : sk[si[i0 + j]];     // (the long form reads it again: eight keys or slots kept alive cost registers)
                }
                if ((ldm >> j) & 1u) {
                    sx = __fadd_rn(sx, r4[j].x); sy = __fadd_rn(sy, r4[j].y); sz = __fadd_rn(sz, r4[j].z); sw = __fadd_rn(sw, r4[j].w);
                    ++cn;
                }
            }
        };
        if (LITEMS > 4 && per <= 4u) voxels(std::integral_constant<int, 4>{});
        else voxels(std::integral_constant<int, LITEMS>{});
        PH(g_phase_k3, 3);
        if (on) {
            // the last voxel may go on past the block: four positions at a time, loads first — up to CM3_EXT_SEQ positions
            // one after the other (stable order, bit for bit pcl's sum); a voxel longer than that is finished by a wave
            uint32_t p = i0 + per;
            bool more = p < m || (tail_open && p == m);
            uint32_t steps = 0;
            while (more && p < m && steps < CM3_EXT_SEQ / 4u) {
                uint16_t s4[4];
                float4 e4[4];
                uint32_t nmatch = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s4[u] = 0;
                    if (nmatch == static_cast<uint32_t>(u) && p + u < m) {
                        s4[u] = si[p + u];
                        if (sk[s4[u]] == ckey) ++nmatch;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (static_cast<uint32_t>(u) < nmatch) e4[u] = rec[rbase + (SUB ? sp[s4[u]] : s4[u])];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (static_cast<uint32_t>(u) < nmatch) {
                        sx = __fadd_rn(sx, e4[u].x); sy = __fadd_rn(sy, e4[u].y); sz = __fadd_rn(sz, e4[u].z); sw = __fadd_rn(sw, e4[u].w);
                        ++cn;
                    }
                }
                p += nmatch;
                more = nmatch == 4 && (p < m || tail_open);
                ++steps;
            }
            if (more) {                                        // (p < m, or p == m with the tail open)
                const uint32_t jn = atomicAdd(&s_njobs, 1u);
                Job3 jb;
                jb.p = p; jb.key = ckey; jb.kid = kid++; jb.cnt = cn; jb.sx = sx; jb.sy = sy; jb.sz = sz; jb.sw = sw;
                if (MAXJ >= static_cast<uint32_t>(LBLOCK) || jn < MAXJ) jobs[jn] = jb;
                else host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_BUCKET;    // (more long voxels than job slots: the frame is handed back)
            } else {
                emit(kid++, ckey, sx, sy, sz, sw, cn);
            }
        }

        PH(g_phase_k3, 4);
        // ---- long voxels. A wave sums 64 positions per chunk, eight chunks (512 positions) per step: every record of a step
        // asked for at once, a chunk's sum formed in a fixed tree order and added to the running sum chunk after chunk:
        // deterministic, within 1e-4 m of pcl's one-after-the-other sum (closer to the exact mean, in fact), not
        // bit-identical to it. Normally wave w takes jobs w, w + LWAVES, ... (first chunks four jobs at a time); with fewer jobs than waves in a tile
        // whose voxels average 512 points or more (coarse grids: a tile's records are a voxel or two of thousands of
        // points, and the tiles behind it have nothing of their own to do) all waves share every job — wave w takes the
        // steps w, w + LWAVES, ... of it — and their partial sums are added in wave order.
        __syncthreads();
        const uint32_t njobs = min(SCAL(s_njobs), MAXJ);
        const bool coop = !(njobs >= static_cast<uint32_t>(LWAVES) || m < 512u * max(c_t, 1u));   // (uniform)
        Job3* part = jobs + 64;                                // (coop: fewer than LWAVES jobs — room for the waves' partial sums)
        // one chunk: the 64 positions from p on that belong to the run of jkey (in: which lanes hold one of its records)
        auto load_chunk = [&](uint32_t p, uint32_t jkey, float4& r4, bool& in) {
            const uint32_t q = p + lane;
            in = false;
            r4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (L == 0) {                                      // sorted position q is record base + a + q, in LDS or not
                const unsigned long long idx = static_cast<unsigned long long>(base) + a + q;
                if (idx < n) { r4 = rec[idx]; in = true; }
            } else if (q < m) {
                const uint32_t sl_ = si[q];
                if (sk[sl_] == jkey) { r4 = rec[rbase + (SUB ? sp[sl_] : sl_)]; in = true; }
            }
        };
        // Opening round: most long voxels are not that long (dense ground cells: tens of points), and a wave that takes
        // its jobs one after the other pays a round trip to L2 for each. The first chunk of four jobs is asked for
        // together; a job that ends inside it is finished here, the others go on below from their second chunk (the
        // chunks of a job are added in the same order either way: same sums, bit for bit).
        constexpr uint32_t JOB_DONE = 0xFFFFFFFFu;
        if (!coop && L != 0) {                                 // (L == 0: dense frames, jobs of thousands of points — no short ones to gain on)
            constexpr int JB = 4;
            for (uint32_t j0 = w; j0 < njobs; j0 += LWAVES * JB) {
                float4 r4[JB];
                bool in[JB];
                uint32_t jk[JB];
#pragma unroll
                for (int u = 0; u < JB; ++u) {
                    const uint32_t jn = j0 + u * LWAVES;
                    in[u] = false; r4[u] = make_float4(0.f, 0.f, 0.f, 0.f); jk[u] = 0;
                    if (jn < njobs) {                          // (uniform)
                        jk[u] = SCAL(jobs[jn].key);
                        const uint32_t q = SCAL(jobs[jn].p) + lane;
                        if (q < m) {
                            const uint32_t sl_ = si[q];
                            if (sk[sl_] == jk[u]) { r4[u] = rec[rbase + (SUB ? sp[sl_] : sl_)]; in[u] = true; }
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < JB; ++u) {
                    const uint32_t jn = j0 + u * LWAVES;
                    if (jn >= njobs) break;                    // (uniform)
                    const unsigned long long bal = __ballot(in[u]);
                    const Job3 jb = jobs[jn];
                    const float ax = __fadd_rn(jb.sx, wave_sum_f32_fixed(r4[u].x)), ay = __fadd_rn(jb.sy, wave_sum_f32_fixed(r4[u].y));
                    const float az = __fadd_rn(jb.sz, wave_sum_f32_fixed(r4[u].z)), aw = __fadd_rn(jb.sw, wave_sum_f32_fixed(r4[u].w));
                    const uint32_t cnj = SCAL(jb.cnt) + static_cast<uint32_t>(__popcll(bal));
                    if (lane == 0) {
                        if (bal != ~0ull) {                    // the run ended inside this chunk: done
                            emit(SCAL(jb.kid), jk[u], ax, ay, az, aw, cnj);
                            jobs[jn].p = JOB_DONE;
                        } else {
                            Job3 nx = jb;
                            nx.p = jb.p + 64u; nx.cnt = cnj; nx.sx = ax; nx.sy = ay; nx.sz = az; nx.sw = aw;
                            jobs[jn] = nx;
                        }
                    }
                }
            }
        }
        for (uint32_t jn = coop ? 0u : w; jn < njobs; jn += coop ? 1u : static_cast<uint32_t>(LWAVES)) {
            const Job3 jb = jobs[jn];
            if (SCAL(jb.p) == JOB_DONE) continue;              // (finished in the opening round; uniform)
            const uint32_t jkey = SCAL(jb.key);
            uint32_t p = SCAL(jb.p) + (coop ? w * (64u * 8u) : 0u), cnj = coop ? 0u : SCAL(jb.cnt);
            const uint32_t stride = coop ? LWAVES * 64u * 8u : 64u * 8u;
            float ax = coop ? 0.f : jb.sx, ay = coop ? 0.f : jb.sy, az = coop ? 0.f : jb.sz, aw = coop ? 0.f : jb.sw;
            bool ended = false;
            while (!ended) {                                   // the steps p, p + stride, ... of the run until it ends
                constexpr int JU = 8;
                float4 r4[JU];
                bool in[JU];
#pragma unroll
                for (int u = 0; u < JU; ++u) load_chunk(p + u * 64, jkey, r4[u], in[u]);
#pragma unroll
                for (int u = 0; u < JU; ++u) {
                    if (ended) break;                          // (uniform)
                    if (L == 0) in[u] = in[u] && key_of(b, r4[u]) == jkey;
                    const unsigned long long bal = __ballot(in[u]);
                    if (!in[u]) r4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    ax = __fadd_rn(ax, wave_sum_f32_fixed(r4[u].x)); ay = __fadd_rn(ay, wave_sum_f32_fixed(r4[u].y));
                    az = __fadd_rn(az, wave_sum_f32_fixed(r4[u].z)); aw = __fadd_rn(aw, wave_sum_f32_fixed(r4[u].w));
                    cnj += static_cast<uint32_t>(__popcll(bal));
                    ended = bal != ~0ull;                      // the run ended inside this chunk (or before this step)
                }
                p += stride;
                if (cnj > CM3_RUN_MAX) break;
            }
            if (!coop) {
                if (cnj > CM3_RUN_MAX && lane == 0) host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_BUCKET;
                if (lane == 0) emit(SCAL(jb.kid), jkey, ax, ay, az, aw, cnj);
            } else {                                           // (every wave is here: jn and njobs are the same for all)
                if (lane == 0) { Job3 pr; pr.p = 0; pr.key = 0; pr.kid = 0; pr.cnt = cnj; pr.sx = ax; pr.sy = ay; pr.sz = az; pr.sw = aw; part[w] = pr; }
                __syncthreads();
                if (threadIdx.x == 0) {
                    float tx = jb.sx, ty = jb.sy, tz = jb.sz, tw = jb.sw;
                    uint32_t tc = jb.cnt;
#pragma unroll
                    for (int q = 0; q < LWAVES; ++q) {
                        tx = __fadd_rn(tx, part[q].sx); ty = __fadd_rn(ty, part[q].sy); tz = __fadd_rn(tz, part[q].sz); tw = __fadd_rn(tw, part[q].sw);
                        tc += part[q].cnt;
                    }
                    if (tc > CM3_RUN_MAX) host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_BUCKET;
                    emit(jb.kid, jkey, tx, ty, tz, tw, tc);
                }
                __syncthreads();
            }
        }
    }
    PH(g_phase_k3, 5);
    if (threadIdx.x == 0) {
        tile_info[tile] = make_uint2(QUANT ? base : (a == 0xFFFFFFFFu ? 0u : a), c_t);   // (QUANT: a == 0; where the tile's centroids start)
        if (c_t) atomicAdd(&grp_cnt[tile >> 6], c_t);
    }
}

// ------------------------------------------------------------------------------------------------
// k3_compact: tile t's kept voxels go from stage[t*LT + a ...] to out[prefix(t) ...]; the frame's state record
// goes to the host (what k2_local's last tile did).
// ------------------------------------------------------------------------------------------------
template <int LT, bool PARTIAL>
__global__ __launch_bounds__(256) void k3_compact(const CmFrameState* __restrict__ st, CmFrameState* __restrict__ st_next,
                                                  uint32_t* __restrict__ host_state, const uint2* __restrict__ tile_info,
                                                  const uint32_t* __restrict__ grp_cnt, const float4* __restrict__ stage,
                                                  const uint32_t* __restrict__ stage_key, const uint32_t* __restrict__ stage_cnt,
                                                  float4* __restrict__ out, uint32_t* __restrict__ out_key,
                                                  uint32_t* __restrict__ out_cnt, uint32_t n_buckets) {
    // n_buckets != 0: the finish ran one workgroup per quantile bucket (k3_local<QUANT>): tile_info[t].x is the absolute start
    __shared__ uint32_t lds[4];
    if (blockIdx.x == 0 && st_next && threadIdx.x < sizeof(CmFrameState) / 4)
        reinterpret_cast<uint32_t*>(st_next)[threadIdx.x] = 0;
    if (st->status != CM_DEV_OK || st->outside) {
        if (blockIdx.x == 0) report_state(host_state, st, st->status, 0u, true);
        return;
    }
    const uint32_t n = st->n_valid;
    if (n == 0) {
        if (blockIdx.x == 0) report_state(host_state, st, CM_DEV_EMPTY, 0u, true);
        return;
    }
    const uint32_t n_lt = n_buckets ? n_buckets : (n + LT - 1) / LT;
    const uint32_t tile = blockIdx.x;
    if (n_buckets && st->quant_abort) {                          // (k4_colscan gave the frame back; its error word is in place)
        if (blockIdx.x == 0) report_state(host_state, st, st->status, 0u, true);
        return;
    }
    // The kernels behind pass 0 may have been launched for fewer records than the frame's slots (a crop box that dropped
    // most points of the last frame: cm_launch.cpp launch_bucket): more records than that, and the frame is handed back.
    if (tile == 0 && threadIdx.x == 0 && n_lt > gridDim.x) host_state[offsetof(CmFrameState, err) / 4] = CM_DEV_ERR_GRID;
    if (tile >= n_lt) return;
    const uint2 info = tile_info[tile];
    if (info.y == 0 && tile != n_lt - 1) return;               // nothing to move (the last tile still reports)
    const uint32_t g = tile >> 6;
    uint32_t s = 0;
    for (uint32_t q = threadIdx.x; q < g; q += 256) s += grp_cnt[q];
    for (uint32_t q = (g << 6) + threadIdx.x; q < tile; q += 256) s += tile_info[q].y;
    s = wave_sum_u32(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    const uint32_t prefix = lds[0] + lds[1] + lds[2] + lds[3];
    if (tile == n_lt - 1) report_state(host_state, st, CM_DEV_OK, prefix + info.y, true);
    const size_t src = n_buckets ? static_cast<size_t>(info.x) : static_cast<size_t>(tile) * LT + info.x;
    for (uint32_t q = threadIdx.x; q < info.y; q += 256) {
        if (PARTIAL) {
            out[2 * (static_cast<size_t>(prefix) + q)] = stage[2 * (src + q)];
            out[2 * (static_cast<size_t>(prefix) + q) + 1] = stage[2 * (src + q) + 1];
        } else {
            const float4 sm = stage[src + q];
            const uint32_t cn = stage_cnt[src + q];
            const float c = static_cast<float>(cn);
            const float rc = __frcp_rn(c);                      // RN(1/c), shared by the four quotients
            out[prefix + q] = make_float4(centroid_div_rc(sm.x, c, rc), centroid_div_rc(sm.y, c, rc), centroid_div_rc(sm.z, c, rc),
                                          centroid_div_rc(sm.w, c, rc));
            if (out_key) { out_key[prefix + q] = stage_key[src + q]; out_cnt[prefix + q] = cn; }
        }
    }
}

}  // namespace
#ifdef CM_PHASE_TIMING
extern "C" __attribute__((visibility("default"))) void cm_debug_phases3(unsigned long long* out, int reset) {
    phase_readout(HIP_SYMBOL(g_phase_k3), out, reset);
}
#endif

void cmk3_local(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* host_state, const void* rec, void* tile_info,
                uint32_t* grp_cnt, void* stage, uint32_t* stage_key, uint32_t* stage_cnt, bool partial, uint32_t low_bits,
                uint32_t n_padded, const uint32_t* spl, const uint32_t* bofs, uint32_t n_buckets, uint32_t* spl_next, bool ballot,
                uint32_t sub_shift, const unsigned char* dig) {
    // 2048-record tiles, room for 4032 (bucket tails of up to 1984 records), 512 threads at no more than 64 registers:
    // 40 912 bytes of LDS — four workgroups per CU, all eight wave slots of every SIMD (44 us at cfg2; with room for 4096 the
    // fourth workgroup does not fit the CU's 160 KiB: 47 us). n_buckets != 0: one workgroup per quantile bucket (cm_kernels_v4.hip).
    // ballot: the LDS sort ranks by ballots instead of returning adds (cm_common.hpp wave_rank_ballot).
    static_assert(CM4_CAP == 4032, "k4_colscan's capacity check is this kernel's LCAP");
    // sub_shift != 0 (shared bins): 2^sub_shift buckets per bin, the workgroups of a bin side by side on one XCD — eight bins
    // (one per XCD) times 2^sub_shift workgroups per step of the grid; 40.5 KB of LDS (the slots' places in the bin, 9-bit digits): four per CU
    const dim3 grid(n_buckets ? (sub_shift ? ((((n_buckets + (1u << sub_shift) - 1u) >> sub_shift) + 7u) / 8u * 8u) << sub_shift : n_buckets)
                              : n_padded / 2048);
#define CM3_LOCAL_(PART, QUANT, BAL, SUB, SK, SC, SPL, BOFS, NB, NEXT)                                                              \
    hipLaunchKernelGGL((k3_local<2048, 4032, 512, 8, PART, QUANT, BAL, SUB>), grid, dim3(512), 0, s, fd, st, host_state,            \
                       reinterpret_cast<const float4*>(rec), reinterpret_cast<uint2*>(tile_info), grp_cnt,                          \
                       reinterpret_cast<float4*>(stage), SK, SC, low_bits, SPL, BOFS, NB, NEXT, nullptr, sub_shift, dig)
#define CM3_LOCAL(PART, QUANT, BAL, SK, SC, SPL, BOFS, NB, NEXT) CM3_LOCAL_(PART, QUANT, BAL, false, SK, SC, SPL, BOFS, NB, NEXT)
    if (n_buckets && sub_shift) { if (ballot) CM3_LOCAL_(false, true, true, true, stage_key, stage_cnt, spl, bofs, n_buckets, spl_next);
                                  else CM3_LOCAL_(false, true, false, true, stage_key, stage_cnt, spl, bofs, n_buckets, spl_next); }
    else if (n_buckets) { if (ballot) CM3_LOCAL(false, true, true, stage_key, stage_cnt, spl, bofs, n_buckets, spl_next);
                     else CM3_LOCAL(false, true, false, stage_key, stage_cnt, spl, bofs, n_buckets, spl_next); }
    else if (partial) { if (ballot) CM3_LOCAL(true, false, true, nullptr, nullptr, nullptr, nullptr, 0u, nullptr);
                        else CM3_LOCAL(true, false, false, nullptr, nullptr, nullptr, nullptr, 0u, nullptr); }
    else { if (ballot) CM3_LOCAL(false, false, true, stage_key, stage_cnt, nullptr, nullptr, 0u, spl_next);
           else CM3_LOCAL(false, false, false, stage_key, stage_cnt, nullptr, nullptr, 0u, spl_next); }
#undef CM3_LOCAL
#undef CM3_LOCAL_
}

// The buckets of a quantile frame that hold more than CM4_CAP records (big_list: k4_colscan), one workgroup of the large shape each.
void cmk3_local_big(hipStream_t s, const CmFrameDev* fd, CmFrameState* st, uint32_t* host_state, const void* rec, void* tile_info,
                    uint32_t* grp_cnt, void* stage, uint32_t* stage_key, uint32_t* stage_cnt, const uint32_t* spl, const uint32_t* bofs,
                    uint32_t n_buckets, uint32_t* spl_next, const uint32_t* big_list, bool ballot) {
#define CM3_BIG(BAL) hipLaunchKernelGGL((k3_local<4096, CM4_CAP_BIG, 1024, 4, false, true, BAL, false>), dim3(CM4_MAX_BIG), dim3(1024), 0, s, fd, st,   \
                                        host_state, reinterpret_cast<const float4*>(rec), reinterpret_cast<uint2*>(tile_info), grp_cnt,         \
                                        reinterpret_cast<float4*>(stage), stage_key, stage_cnt, 0u, spl, bofs, n_buckets, spl_next, big_list, 0u, nullptr)
    if (ballot) CM3_BIG(true); else CM3_BIG(false);
#undef CM3_BIG
}

void cmk3_compact(hipStream_t s, const CmFrameState* st, CmFrameState* st_next, uint32_t* host_state, const void* tile_info,
                  const uint32_t* grp_cnt, const void* stage, const uint32_t* stage_key, const uint32_t* stage_cnt, void* out,
                  uint32_t* out_key, uint32_t* out_cnt, bool partial, uint32_t n_padded, uint32_t n_buckets) {
    const dim3 grid(n_buckets ? n_buckets : n_padded / 2048);
    if (partial)
        hipLaunchKernelGGL((k3_compact<2048, true>), grid, dim3(256), 0, s, st, st_next, host_state,
                           reinterpret_cast<const uint2*>(tile_info), grp_cnt, reinterpret_cast<const float4*>(stage),
                           nullptr, nullptr, reinterpret_cast<float4*>(out), nullptr, nullptr, 0u);
    else
        hipLaunchKernelGGL((k3_compact<2048, false>), grid, dim3(256), 0, s, st, st_next, host_state,
                           reinterpret_cast<const uint2*>(tile_info), grp_cnt, reinterpret_cast<const float4*>(stage),
                           stage_key, stage_cnt, reinterpret_cast<float4*>(out), out_key, out_cnt, n_buckets);
}
