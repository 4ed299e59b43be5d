// cm_cast_math.hpp — the arithmetic of one ray of the cast layer (cm_map_cast_*; steps 3 to 6 of its semantics in
// include/cloudmerge.h): the exact quotient without an integer division, the line's cell at an arbitrary step,
// the last step inside the window found up front, the skip count of a squared distance and the two walks. Plain C++ for the
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

// One ray's line from its direction entry (dx, dy), |dx|, |dy| <= 1024, L = max(|dx|, |dy|) >= 1. The driving axis, the one
// with |d| = L, moves one cell per step: rdiv(k * L, L) = k. The other moves rdiv(k * am, L) = (2 k am + L) div 2 L.
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

// The cell of step k minus the origin cell, k <= L: 2 k am + L <= 2 * 1024 * 1024 + 1024 < 2^22.
CM_CAST_FN void cm_cast_cell(const CmCastLine& ln, uint32_t k, int32_t* jx, int32_t* jy) {
    const int32_t qm = static_cast<int32_t>(cm_cast_quot(2u * k * ln.am + ln.L, 2u * ln.L, ln.r2L)), kk = static_cast<int32_t>(k);
    *jx = ln.sx * (ln.xdrive ? kk : qm);
    *jy = ln.sy * (ln.xdrive ? qm : kk);
}

// The last step whose cell lies inside the nx x ny window, from the origin cell (ox, oy) inside it. Membership is monotone in
// k per axis. The driving axis allows k <= m, m its cells to the edge. The minor axis allows (2 k am + L) div 2 L <= m, that is
// 2 k am < (2 m + 1) L, that is k <= ((2 m + 1) L - 1) div 2 am; only m < am can bind, and then (2 m + 1) L - 1 < 2 am L <= 2^21.
CM_CAST_FN uint32_t cm_cast_last_inside(const CmCastLine& ln, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny) {
    const uint32_t mx = ln.sx > 0 ? nx - 1u - ox : ox, my = ln.sy > 0 ? ny - 1u - oy : oy;
    const uint32_t md = ln.xdrive ? mx : my, mm = ln.xdrive ? my : mx;
    uint32_t K = ln.L < md ? ln.L : md;
    if (mm < ln.am) {
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

// The default walk: from step k the ray jumps steps[cell] steps; 0 there is an occupied cell. No step beyond the last one
// inside the window is looked at, so every read lies in the table. Status values are cm_cast_ray's: 0 MAX, 1 HIT, 2 OFF_MAP.
CM_CAST_FN CmCastWords cm_cast_walk_skip(int32_t dx, int32_t dy, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const unsigned char* steps) {
    const CmCastLine ln = cm_cast_line(dx, dy);
    const uint32_t K = cm_cast_last_inside(ln, ox, oy, nx, ny);
    uint32_t k = 0u;
    while (k <= K) {
        int32_t jx, jy;
        cm_cast_cell(ln, k, &jx, &jy);
        const uint32_t t = steps[(oy + static_cast<uint32_t>(jy)) * nx + (ox + static_cast<uint32_t>(jx))];
        if (t == 0u) return cm_cast_record(ln, k, 1u);
        k += t;
    }
    return K == ln.L ? cm_cast_record(ln, K, 0u) : cm_cast_record(ln, K, 2u);
}

// The plain walk: steps 4 and 5 of the semantics cell by cell, the window tested at every step, the image read.
CM_CAST_FN CmCastWords cm_cast_walk_plain(int32_t dx, int32_t dy, uint32_t ox, uint32_t oy, uint32_t nx, uint32_t ny, const signed char* image) {
    const CmCastLine ln = cm_cast_line(dx, dy);
    for (uint32_t k = 0u; k <= ln.L; ++k) {
        int32_t jx, jy;
        cm_cast_cell(ln, k, &jx, &jy);
        const uint32_t cx = ox + static_cast<uint32_t>(jx), cy = oy + static_cast<uint32_t>(jy);      // (wraps below 0: above nx)
        if (cx >= nx || cy >= ny) return cm_cast_record(ln, k - 1u, 2u);          // (k >= 1: the origin is inside)
        if (image[cy * nx + cx] == 100) return cm_cast_record(ln, k, 1u);
    }
    return cm_cast_record(ln, ln.L, 0u);
}
