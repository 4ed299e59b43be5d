// cm_cast_math.hpp — the arithmetic of one ray of the cast layer (cm_map_cast_*; steps 3 to 6 of its semantics in
// include/cloudmerge.h): the exact quotient without an integer division, the line's cell at an arbitrary step,
// the last step inside the window found up front, the skip count of a squared distance and the two walks. The localisation
// layer's beam model (cm_map_mcl_beam_configure) walks the same line from a particle's cell towards a beam's end
// cell and `over` steps past it: the forms with a reach of L + over serve it, and the cast layer's walks are those forms with
// over = 0. Plain C++ for the
// host (cm_cast_directions' callers, host/cast_tests.cpp, which runs both walks against a walk by `/` on the CPU) and, with
// CM_CAST_FN set to __device__ __forceinline__ and CM_CAST_RCP to the hardware reciprocal, for cm_kernels_cast.hip: integers
// apart from the one fp32 product of cm_cast_quot, whose result is corrected, so both sides give the same bits.
// tests/cast_ref.py restates the quotient and the skip rule.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef CM_CAST_FN
#define CM_CAST_FN inline
#endif
#ifndef CM_CAST_RCP
#define CM_CAST_RCP(d) (1.0f / (d))
#endif

// floor(n / d) for n < 2^24, d >= 1 and n / d < 2^21; rd is 1 / (float)d to within one unit in the last place. (float)n and
// (float)d are exact, the product is off by less than 2^21 * (2^-23 + 2^-24) = 0.375, so its integer part is the quotient or
// one beside it: one correction step either way. tests/test_map_cast.py sweeps the same arithmetic with rd moved one unit up
// and down.
CM_CAST_FN uint32_t cm_cast_quot(uint32_t n, uint32_t d, float rd) {
    uint32_t q = static_cast<uint32_t>(static_cast<float>(n) * rd);
    const int32_t r = static_cast<int32_t>(n) - static_cast<int32_t>(q * d);
    if (r < 0) --q;
    else if (r >= static_cast<int32_t>(d)) ++q;
    return q;
}

// The skip count of a cell from its dist2: 0 on an occupied cell; otherwise j* = the smallest j >= 1 with 2 j^2 >= dist2,
// capped at cap (a smaller skip is always sound). CM_MAP_DIST_NONE gives the cap.
CM_CAST_FN uint32_t cm_cast_step_of(uint32_t d2, uint32_t cap) {
    if (d2 == 0u) return 0u;
    if (d2 > 2u * (cap - 1u) * (cap - 1u)) return cap;                   // (j* >= cap)
    uint32_t j = static_cast<uint32_t>(sqrtf(static_cast<float>(d2) * 0.5f));   // (d2 < 2^24: exact; j is j* or one beside it)
    while (2u * j * j < d2) ++j;
    while (j > 1u && 2u * (j - 1u) * (j - 1u) >= d2) --j;
    return j < 1u ? 1u : j;
}

// One ray's line from (dx, dy), L = max(|dx|, |dy|) >= 1 (1 / 2L does not exist for L = 0: such a ray never comes here). The
// cast layer's direction entries have |dx|, |dy| <= 1024; the beam model's lines have |dx|, |dy| <= CM_CAST_MAX_D = 1450 and
// are followed CM_CAST_MAX_OVER = 64 steps past L. The driving axis, the one with |d| = L, moves one cell per step:
// rdiv(k * L, L) = k, for k > L too. The other moves rdiv(k * am, L) = (2 k am + L) div 2 L.
#define CM_CAST_MAX_D 1450u
#define CM_CAST_MAX_OVER 64u
struct CmCastLine {
    int32_t sx, sy;                    // signs of dx, dy (+1 for 0: the quotient is 0 then)
    uint32_t am, L;                    // the minor |d| and L
    float r2L;                         // 1 / (2 L)
    bool xdrive;                       // |dx| >= |dy|
};

CM_CAST_FN CmCastLine cm_cast_line(int32_t dx, int32_t dy) {
    CmCastLine ln;
    const uint32_t adx = static_cast<uint32_t>(dx < 0 ? -dx : dx), ady = static_cast<uint32_t>(dy < 0 ? -dy : dy);
    ln.sx = dx < 0 ? -1 : 1;
    ln.sy = dy < 0 ? -1 : 1;
    ln.xdrive = adx >= ady;
    ln.L = ln.xdrive ? adx : ady;
    ln.am = ln.xdrive ? ady : adx;
    ln.r2L = CM_CAST_RCP(static_cast<float>(2u * ln.L));
    return ln;
}

// The cell of step k minus the origin cell, k <= L + over: the operand 2 k am + L is at most 2 * 1024 * 1024 + 1024 < 2^22 for
// the cast layer and 2 * (1450 + 64) * 1450 + 1450 = 4 392 050 < 2^24 for the beam model; the quotient is at most k + 1 < 2^21.
CM_CAST_FN void cm_cast_cell(const CmCastLine& ln, uint32_t k, int32_t* jx, int32_t* jy) {
    const int32_t qm = static_cast<int32_t>(cm_cast_quot(2u * k * ln.am + ln.L, 2u * ln.L, ln.r2L)), kk = static_cast<int32_t>(k);
    *jx = ln.sx * (ln.xdrive ? kk : qm);
    *jy = ln.sy * (ln.xdrive ? qm : kk);
}

// The last step k <= L + over whose cell lies inside the nx x ny window, from the origin cell (ox, oy) inside it. Membership
// is monotone in k per axis. The driving axis allows k <= m, m its cells to the edge. The minor axis allows
// (2 k am + L) div 2 L <= m, that is 2 k am < (2 m + 1) L, that is k <= ((2 m + 1) L - 1) div 2 am. At k = L + over the minor
// axis has moved (2 (L + over) am + L) div 2 L <= am + over cells (am <= L), so only m < am + over can bind; then
// (2 m + 1) L - 1 < 2 (am + over) L <= 2 * 1514 * 1450 = 4 390 600 < 2^24 (2^21 with over = 0 and L <= 1024) and the quotient
// is below (am + over + 1) L / am <= 66 * 1450 < 2^17. am = 0 never binds: the minor axis does not move.
CM_CAST_FN uint32_t cm_cast_last_inside(const CmCastLine& ln, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, uint32_t over = 0u) {
    const uint32_t mx = ln.sx > 0 ? nx - 1u - ox : ox, my = ln.sy > 0 ? ny - 1u - oy : oy;
    const uint32_t md = ln.xdrive ? mx : my, mm = ln.xdrive ? my : mx;
    const uint32_t reach = ln.L + over;
    uint32_t K = reach < md ? reach : md;
    if (mm < ln.am + over && ln.am != 0u) {
        const uint32_t d = 2u * ln.am;
        const uint32_t km = cm_cast_quot((2u * mm + 1u) * ln.L - 1u, d, CM_CAST_RCP(static_cast<float>(d)));
        K = K < km ? K : km;
    }
    return K;
}

// A record as two words: k | status << 16, then (uint16_t)jx | (uint16_t)jy << 16 (cm_cast_ray, little endian).
struct CmCastWords {
    uint32_t a, b;
};

CM_CAST_FN CmCastWords cm_cast_record(const CmCastLine& ln, uint32_t k, uint32_t status) {
    int32_t jx, jy;
    cm_cast_cell(ln, k, &jx, &jy);
    CmCastWords w;
    w.a = k | (status << 16);
    w.b = (static_cast<uint32_t>(jx) & 0xFFFFu) | (static_cast<uint32_t>(jy) << 16);
    return w;
}

// The outcome of a walk with a reach of L + over, one word: k | status << 16 with cm_cast_ray's status values. 1 HIT: the first
// occupied cell is at step k. 0 MAX: no occupied cell through step k = L + over. 2 OFF_MAP: step k is the last one inside the
// window, k < L + over, and no occupied cell through it.
//
// The default walk, N rays of one origin at a time: from step k a ray jumps steps[cell] steps; 0 there is an occupied cell. No
// step beyond the last one inside the window is looked at, so every read lies in the table. The N byte loads of a round do not
// depend on one another, which is what a caller with several rays per lane wants: the chain of dependent loads is the bound
// (DESIGN.md §30, §32). A ray with live[i] false is not walked and its out[i] is left alone.
template <int N>
CM_CAST_FN void cm_cast_reach_skip_n(const CmCastLine (&ln)[N], const bool (&live)[N], uint32_t over, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny,
                                     const unsigned char* steps, uint32_t (&out)[N]) {
    uint32_t k[N], K[N];
    bool go[N], any = false;
    for (int i = 0; i < N; ++i) {
        k[i] = 0u;
        K[i] = 0u;
        go[i] = live[i];
        if (go[i]) {
            K[i] = cm_cast_last_inside(ln[i], ox, oy, nx, ny, over);
            any = true;
        }
    }
    while (any) {
        uint32_t t[N];
        for (int i = 0; i < N; ++i) {
            t[i] = 1u;
            if (go[i]) {
                int32_t jx, jy;
                cm_cast_cell(ln[i], k[i], &jx, &jy);
                t[i] = steps[(oy + static_cast<uint32_t>(jy)) * nx + (ox + static_cast<uint32_t>(jx))];
            }
        }
        any = false;
        for (int i = 0; i < N; ++i) {
            if (!go[i]) continue;
            if (t[i] == 0u) {
                out[i] = k[i] | (1u << 16);
                go[i] = false;
                continue;
            }
            k[i] += t[i];
            if (k[i] > K[i]) {
                out[i] = K[i] | ((K[i] == ln[i].L + over ? 0u : 2u) << 16);
                go[i] = false;
                continue;
            }
            any = true;
        }
    }
}

// The plain walk of N rays of one origin: cell by cell, the window tested at every step, the image read.
template <int N>
CM_CAST_FN void cm_cast_reach_plain_n(const CmCastLine (&ln)[N], const bool (&live)[N], uint32_t over, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny,
                                      const signed char* image, uint32_t (&out)[N]) {
    bool go[N], any = false;
    for (int i = 0; i < N; ++i) {
        go[i] = live[i];
        any = any || go[i];
    }
    for (uint32_t k = 0u; any; ++k) {
        int32_t v[N];
        bool in[N];
        for (int i = 0; i < N; ++i) {
            v[i] = 0;
            in[i] = false;
            if (go[i]) {
                int32_t jx, jy;
                cm_cast_cell(ln[i], k, &jx, &jy);
                const uint32_t cx = ox + static_cast<uint32_t>(jx), cy = oy + static_cast<uint32_t>(jy);  // (wraps below 0: above nx)
                in[i] = cx < nx && cy < ny;
                if (in[i]) v[i] = image[cy * nx + cx];
            }
        }
        any = false;
        for (int i = 0; i < N; ++i) {
            if (!go[i]) continue;
            go[i] = false;
            if (!in[i]) out[i] = (k - 1u) | (2u << 16);                // (k >= 1: the origin is inside)
            else if (v[i] == 100) out[i] = k | (1u << 16);
            else if (k == ln[i].L + over) out[i] = k;
            else go[i] = any = true;
        }
    }
}

CM_CAST_FN uint32_t cm_cast_reach_skip(const CmCastLine& ln, uint32_t over, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const unsigned char* steps) {
    const CmCastLine l1[1] = {ln};
    const bool live[1] = {true};
    uint32_t out[1] = {0u};
    cm_cast_reach_skip_n<1>(l1, live, over, ox, oy, nx, ny, steps, out);
    return out[0];
}

CM_CAST_FN uint32_t cm_cast_reach_plain(const CmCastLine& ln, uint32_t over, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const signed char* image) {
    const CmCastLine l1[1] = {ln};
    const bool live[1] = {true};
    uint32_t out[1] = {0u};
    cm_cast_reach_plain_n<1>(l1, live, over, ox, oy, nx, ny, image, out);
    return out[0];
}

// The cast layer's two walks (steps 4 and 5 of its semantics): a reach of L, the outcome as a record.
CM_CAST_FN CmCastWords cm_cast_walk_skip(int32_t dx, int32_t dy, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const unsigned char* steps) {
    const CmCastLine ln = cm_cast_line(dx, dy);
    const uint32_t w = cm_cast_reach_skip(ln, 0u, ox, oy, nx, ny, steps);
    return cm_cast_record(ln, w & 0xFFFFu, w >> 16);
}

CM_CAST_FN CmCastWords cm_cast_walk_plain(int32_t dx, int32_t dy, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const signed char* image) {
    const CmCastLine ln = cm_cast_line(dx, dy);
    const uint32_t w = cm_cast_reach_plain(ln, 0u, ox, oy, nx, ny, image);
    return cm_cast_record(ln, w & 0xFFFFu, w >> 16);
}
