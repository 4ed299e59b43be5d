// cm_sor_sum.hpp — exact sums of non-negative fp32 terms for the statistical outlier stage, shared by the
// device (cm_kernels_sor.hip) and the host: plain C++, no HIP. tests/test_sor.py builds it on the CPU and compares it with
// Python's math.fsum.
//
// A term's bits split into its biased exponent e (the bin) and its significand m (24 bits with the implicit one; a
// subnormal's 23 bits as they are): value = m * 2^(max(e, 1) - 150). Bins hold sum(m) as uint64: 2^30 terms x 2^24 < 2^64,
// and integer adds are exact in any order. cm_sor_bins_to_double forms the exact sum of sum_e bins[e] * 2^(max(e, 1) - 150)
// as a 352-bit integer in units of 2^-149 and rounds it once to the nearest double (ties to even). A term of +inf (e = 255)
// makes the sum +inf.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define CM_SOR_HD __host__ __device__
#else
#define CM_SOR_HD
#endif

#define CM_SOR_BINS 256
#define CM_SOR_LIMBS 11

// The bin and the significand of a non-negative fp32 term.
CM_SOR_HD inline void cm_sor_split(float v, uint32_t* bin, uint32_t* sig) {
    union { float f; uint32_t u; } b;
    b.f = v;
    const uint32_t e = (b.u >> 23) & 0xFFu;
    *bin = e;
    *sig = (b.u & 0x7FFFFFu) | (e ? 0x800000u : 0u);
}

CM_SOR_HD inline double cm_sor_bins_to_double(const unsigned long long* bins) {
    if (bins[255]) return __builtin_inf();
    uint32_t limb[CM_SOR_LIMBS];
    for (int l = 0; l < CM_SOR_LIMBS; ++l) limb[l] = 0u;
    for (int e = 0; e < 255; ++e) {
        const unsigned long long v = bins[e];
        if (!v) continue;
        const int sh = (e ? e : 1) - 1;                 // bit position of the term's unit 2^(max(e,1) - 150) above 2^-149
        const int li = sh >> 5, off = sh & 31;
        uint32_t w[3];
        w[0] = static_cast<uint32_t>(v << off);
        w[1] = static_cast<uint32_t>(off ? (v >> (32 - off)) : (v >> 32));
        w[2] = off ? static_cast<uint32_t>(v >> (64 - off)) : 0u;
        unsigned long long carry = 0;
        for (int l = li; l < CM_SOR_LIMBS; ++l) {
            const unsigned long long t = static_cast<unsigned long long>(limb[l]) + (l - li < 3 ? w[l - li] : 0u) + carry;
            limb[l] = static_cast<uint32_t>(t);
            carry = t >> 32;
            if (l - li >= 2 && !carry) break;
        }
    }
    int top = -1;                                       // highest set bit
    for (int l = CM_SOR_LIMBS - 1; l >= 0 && top < 0; --l)
        if (limb[l])
            for (int b = 31; b >= 0; --b)
                if ((limb[l] >> b) & 1u) { top = 32 * l + b; break; }
    if (top < 0) return 0.0;
    auto bit = [&](int pos) -> unsigned long long {
        return pos < 0 ? 0ull : static_cast<unsigned long long>((limb[pos >> 5] >> (pos & 31)) & 1u);
    };
    const int lo = top - 63;                            // the 64-bit window [lo, top]; below it only whether anything is set
    unsigned long long w = 0;
    for (int b = 0; b < 64; ++b) w |= bit(lo + b) << b;
    bool sticky = false;
    for (int pos = 0; pos < lo && !sticky; ++pos) sticky = bit(pos) != 0;
    unsigned long long mant = w >> 11;
    const unsigned long long rem = w & 0x7FFull;
    if (rem > 0x400ull || (rem == 0x400ull && (sticky || (mant & 1ull)))) ++mant;
    int ex = top - 52 - 149;                            // value = mant * 2^ex
    if (mant == (1ull << 53)) { mant >>= 1; ++ex; }
    // (mant < 2^53 converts exactly; the scale is a power of two well inside the normal range: the product is exact)
    double r = static_cast<double>(mant);
    for (; ex > 0; --ex) r *= 2.0;
    for (; ex < 0; ++ex) r *= 0.5;
    return r;
}
