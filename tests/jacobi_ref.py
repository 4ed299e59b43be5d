"""jacobi3 (cm_common.hpp) restated in numpy float64, vectorised over matrices: the eigen-decomposition shared by the ground
stage's plane refit, the per-voxel covariance and the normals.

Every numpy elementwise operation, division and np.sqrt on float64 is one correctly rounded IEEE operation and numpy never
contracts a multiply-add, so the result is the kernel's bit for bit as long as the order below is the kernel's: the pairs
(0,1), (0,2), (1,2); 12 sweeps; a rotation skipped where |a_pq| < 1e-300 (a mask: np.where keeps the old values, so a NaN
a_pq is rotated, as the kernel's comparison has it); the three update loops (columns p and q of a, rows p and q of a, columns
p and q of v), each reading both old values before it writes. tests/ground_ref.py::jacobi3 is the same thing on Python
floats, one matrix at a time; tests/test_jacobi_ref.py holds the two together."""
import numpy as np

PAIRS = ((0, 1), (0, 2), (1, 2))
SWEEPS = 12
SKIP_BELOW = 1e-300


def jacobi3(a, sweeps=SWEEPS):
    """a: (n, 3, 3) symmetric float64. Returns (a, v): the rotated matrices (the eigenvalues on the diagonal, unsorted) and
    the eigenvectors as the columns of v[n]."""
    a = np.array(a, dtype=np.float64, copy=True).reshape(-1, 3, 3)
    n = len(a)
    v = np.zeros((n, 3, 3))
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = a[:, p, q].copy()
                skip = np.abs(apq) < SKIP_BELOW
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                old_a, old_v = a.copy(), v.copy()
                c_, s_ = c[:, None], s[:, None]
                akp, akq = a[:, :, p].copy(), a[:, :, q].copy()            # columns p, q
                a[:, :, p] = c_ * akp - s_ * akq
                a[:, :, q] = s_ * akp + c_ * akq
                apk, aqk = a[:, p, :].copy(), a[:, q, :].copy()            # rows p, q
                a[:, p, :] = c_ * apk - s_ * aqk
                a[:, q, :] = s_ * apk + c_ * aqk
                vkp, vkq = v[:, :, p].copy(), v[:, :, q].copy()
                v[:, :, p] = c_ * vkp - s_ * vkq
                v[:, :, q] = s_ * vkp + c_ * vkq
                a[skip] = old_a[skip]
                v[skip] = old_v[skip]
    return a, v


def sym3(c6, tri):
    """(n, 6) lower-triangle entries in the order `tri` of (i, j) pairs -> (n, 3, 3) symmetric matrices"""
    c6 = np.asarray(c6, np.float64)
    m = np.empty((len(c6), 3, 3))
    for q, (i, j) in enumerate(tri):
        m[:, i, j] = c6[:, q]
        m[:, j, i] = c6[:, q]
    return m
