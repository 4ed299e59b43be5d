// cm_align_solve.hpp — the host side of one point-to-plane ICP iteration (cm_result_align): the 6x6 solve and
// the pose update. Plain C++, no HIP; tests/test_align.py builds it on the CPU and compares it with numpy.linalg.solve, and
// tests/align_ref.py restates it operation for operation. Build without contraction (-ffp-contract=off), as the library is.
//
//   cm_align_solve   H x = -g by LDL^T without pivoting. H: the lower triangle row by row (21 entries). false — singular —
//                    when a pivot is <= CM_ALIGN_PIVOT_MIN * max_i H_ii or NaN; x is then left alone.
//   cm_align_update  x = (w, v), a twist about p0:  R' = Rodrigues(w) R,  t' = Rodrigues(w) (t - p0) + p0 + v  on the
//                    row-major 3x4 pose. Rodrigues(w) = I + sin(th) K + 2 sin^2(th / 2) K^2, K the cross matrix of w / th,
//                    th = |w|; th == 0 is the identity exactly.
#pragma once
#include <cmath>

#ifndef CM_ALIGN_PIVOT_MIN
#define CM_ALIGN_PIVOT_MIN 1e-9
#endif

inline bool cm_align_solve(const double H[21], const double g[6], double x[6]) {
    double A[6][6], L[6][6], d[6], y[6];
    for (int i = 0, t = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j, ++t) A[i][j] = H[t];
    double top = A[0][0];
    for (int i = 1; i < 6; ++i) top = A[i][i] > top ? A[i][i] : top;
    const double thr = CM_ALIGN_PIVOT_MIN * top;
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
        if (!(dj > thr)) return false;                     // (a NaN pivot or threshold lands here too)
        d[j] = dj;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = s / dj;
        }
    }
    for (int i = 0; i < 6; ++i) {                          // L y = -g
        double s = -g[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; --i) {                         // L^T x = y / d
        double s = y[i] / d[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    return true;
}

// |w| and |v| of a twist, as the convergence test reads them.
inline double cm_align_norm3(const double* a) { return std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

inline void cm_align_update(double pose[12], const double x[6], const double p0[3]) {
    const double th = cm_align_norm3(x);
    double W[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (th > 0.0) {
        const double k0 = x[0] / th, k1 = x[1] / th, k2 = x[2] / th;
        const double s = std::sin(th), h = std::sin(th * 0.5), c1 = (2.0 * h) * h;
        const double K[3][3] = {{0.0, -k2, k1}, {k2, 0.0, -k0}, {-k1, k0, 0.0}};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
                W[i][j] = (W[i][j] + s * K[i][j]) + c1 * kk;
            }
    }
    double R[3][3], u[3];
    for (int i = 0; i < 3; ++i) u[i] = pose[4 * i + 3] - p0[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i][j] = (W[i][0] * pose[j] + W[i][1] * pose[4 + j]) + W[i][2] * pose[8 + j];
    }
    for (int i = 0; i < 3; ++i) {
        const double wu = (W[i][0] * u[0] + W[i][1] * u[1]) + W[i][2] * u[2];
        for (int j = 0; j < 3; ++j) pose[4 * i + j] = R[i][j];
        pose[4 * i + 3] = (wu + p0[i]) + x[3 + i];
    }
}
