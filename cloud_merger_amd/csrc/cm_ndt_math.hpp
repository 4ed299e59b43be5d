// cm_ndt_math.hpp — the exponential of NDT's weights (cm_result_ndt_align), spelled out operation for operation
// so that the kernel, the host and the CPU tests compute the same bits: the device's exp is not libm's. Plain C++; the three
// rounded operations go through macros, which cm_kernels_ndt.hip sets to the _rn intrinsics before including this file and
// which default to the plain operators (build without contraction, -ffp-contract=off, as the library is). tests/ndt_ref.py
// restates it; tests/test_ndt.py builds it with g++ into a stand-alone driver and compares the two bit for bit.
//
//   cm_exp_neg(x), x >= 0: exp(-x). x >= 700 or NaN: +0.0. t = -x; k = rint(t * log2(e)); rr = (t - k * ln2_hi) - k * ln2_lo
//   (fdlibm's split of ln 2: k * ln2_hi is exact for |k| < 2^11); p = sum_{n=0..13} rr^n / n! by Horner from n = 13 down,
//   p = p * rr + c_n with two roundings per step, c_n = 1.0 / double(n!); the result is ldexp(p, k). |rr| <= 0.3466, so the
//   series' remainder is below 2^-58 of p; k >= -1010, so the result is a normal number. exp_neg(0) is exactly 1.0.
#pragma once
#include <cmath>

#ifndef CM_NDT_FN
#define CM_NDT_FN inline
#endif
#ifndef CM_NDT_MUL
#define CM_NDT_MUL(a, b) ((a) * (b))
#define CM_NDT_ADD(a, b) ((a) + (b))
#define CM_NDT_SUB(a, b) ((a) - (b))
#endif

#define CM_NDT_EXP_CUT 700.0

CM_NDT_FN double cm_exp_neg(double x) {
    if (!(x < CM_NDT_EXP_CUT)) return 0.0;                 // (NaN lands here too)
    const double t = -x;
    const double k = rint(CM_NDT_MUL(t, 0x1.71547652b82fep+0));
    const double rr = CM_NDT_SUB(CM_NDT_SUB(t, CM_NDT_MUL(k, 0x1.62e42fee00000p-1)), CM_NDT_MUL(k, 1.90821492927058770002e-10));
    double p = 1.0 / 6227020800.0;                         // 1 / 13!
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 479001600.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 39916800.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 3628800.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 362880.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 40320.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 5040.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 720.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 120.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 24.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 6.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0 / 2.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0);
    p = CM_NDT_ADD(CM_NDT_MUL(p, rr), 1.0);
    return ldexp(p, static_cast<int>(k));
}
