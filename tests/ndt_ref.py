"""Restatement of cm_result_ndt_align (include/cloudmerge.h) in numpy: explicit per-operation fp64, no BLAS
products anywhere, every three-term form written out in full (the kernel leaves the exact zeros out).

exp_neg() restates cm_ndt_math.hpp operation for operation. The voxel lookup is a Python dict on the absolute cell
(c0, c1, c2) -> result index, built from cm_result_copy_cells — not a search over keys. The covariance table is an input:
tests/voxel_cov_ref.py's or the device's (each test says which). The transform, the cross-point sum, the solve, the pose
update and the loop are §16's: tests/align_ref.py's transform, tree_sum, solve, update and norm3, unchanged."""
import math

import numpy as np

from tests.align_ref import IDENTITY, norm3, pivot, solve, transform, tree_sum, update

F32 = np.float32
F64 = np.float64
NONE = 0xFFFFFFFF
MAX_ITER = 64
CONVERGED, MAX_ITER_HIT, FEW, SINGULAR = 1, 2, 4, 8
COV_VALID = 1
CORR_DTYPE = np.dtype([("idx", "<u4"), ("n_used", "<u4"), ("score", "<f8")])
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = 1.90821492927058770002e-10                       # fdlibm's ln2_lo
EXP_CUT = 700.0
COEF = [F64(1.0) / F64(math.factorial(n)) for n in range(14)]
# the candidates' offsets in order: c, c - e0, c + e0, c - e1, c + e1, c - e2, c + e2
OFFSETS = np.array([[0, 0, 0], [-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.int64)
TRI = ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))     # cm_voxel_cov's order of the lower triangle


def exp_neg(x):
    """cm_exp_neg on an array of x >= 0 (or NaN)."""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        live = x < EXP_CUT                                  # (NaN: not live)
        t = -np.where(live, x, 0.0)
        k = np.rint(t * LOG2E)
        rr = (t - k * LN2_HI) - k * LN2_LO
        p = np.full(x.shape, COEF[13])
        for n in range(12, -1, -1):
            p = p * rr + COEF[n]
        return np.where(live, np.ldexp(p, k.astype(np.int64)), 0.0)


def gauss(leaf, outlier_ratio):
    """(d1, d2) of step 0 with this interpreter's log and exp (the tests take d2 from the call and compare)."""
    leaf = np.asarray(leaf, F32).astype(F64)
    res3 = (leaf[0] * leaf[1]) * leaf[2]
    p = float(F32(outlier_ratio))
    c1, c2 = 10.0 * (1.0 - p), p / res3
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def voxel_dict(cells):
    """{(c0, c1, c2) absolute: result index}."""
    return {(int(c[0]), int(c[1]), int(c[2])): k for k, c in enumerate(np.asarray(cells).reshape(-1, 3).tolist())}


def point_cells(qf, leaf, min_b, div_b):
    """Step 2's head: (near, c) — whether a point has voxels at all, and its cell relative to the grid (int64)."""
    inv = F32(1.0) / np.asarray(leaf, F32)
    fb, fd = np.asarray(min_b, np.int64).astype(F32), np.asarray(div_b, np.int64).astype(F32)
    with np.errstate(all="ignore"):
        v = np.floor(qf * inv[None, :]) - fb[None, :]       # fp32 throughout
        assert v.dtype == F32
        near = np.isfinite(qf).all(axis=1) & ((v >= F32(-1.0)) & (v <= fd[None, :])).all(axis=1)
        c = np.where(near[:, None], v, 0).astype(np.int64)
    return near, c


def _dot3(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def evaluate(src, tgt, cells, table, T, d2, leaf, min_b, div_b, neighborhood=7, p0=None, lookup=None):
    """E(T). tgt: the result's records (n_out, 3) fp32; cells: their absolute cells; table: VOXEL_COV_DTYPE entries.
    Returns corr, H, g, score, n_corr, p0, terms (n, 28) per point, used (n, 7) result index of every used voxel or -1,
    and cut: how many used pairs had d2h * m >= 700."""
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    p0 = pivot(tgt) if p0 is None and len(tgt) else (np.zeros(3) if p0 is None else np.asarray(p0, F64))
    lookup = voxel_dict(cells) if lookup is None else lookup
    min_b, div_b = np.asarray(min_b, np.int64), np.asarray(div_b, np.int64)
    d2h = F64(d2) * 0.5
    q64, qf = transform(src, T)
    n = len(q64)
    near, c = point_cells(qf, leaf, min_b, div_b)
    acc = np.zeros((n, 28))
    used_idx = np.full((n, 7), -1, np.int64)
    cut = 0
    with np.errstate(all="ignore"):
        a = q64 - p0
    zero, one = np.zeros(n), np.ones(n)
    cols = [(zero, -a[:, 2], a[:, 1]), (a[:, 2], zero, -a[:, 0]), (-a[:, 1], a[:, 0], zero),
            (one, zero, zero), (zero, one, zero), (zero, zero, one)]
    for j in range(neighborhood):
        cand = c + OFFSETS[j]
        ok = near & ((cand >= 0) & (cand < div_b[None, :])).all(axis=1)         # per axis, as integers
        rows = np.nonzero(ok)[0]
        k = np.full(n, -1, np.int64)
        if len(rows) and len(tgt):
            uniq, inverse = np.unique(cand[rows] + min_b[None, :], axis=0, return_inverse=True)
            found = np.array([lookup.get((int(u[0]), int(u[1]), int(u[2])), -1) for u in uniq.tolist()], np.int64)
            k[rows] = found[np.ravel(inverse)]
        hit = k >= 0
        kk = np.where(hit, k, 0)
        if len(tgt):
            hit &= (table["flags"][kk] & COV_VALID) != 0
        else:
            hit[:] = False
        if not hit.any():
            continue
        with np.errstate(all="ignore"):
            b = table["mean"][kk].astype(F64) - p0
            r = a - b
            ic = table["icov"][kk].astype(F64)
            B = [[None] * 3 for _ in range(3)]
            for q, (i, jj) in enumerate(TRI):
                B[i][jj] = ic[:, q]
                B[jj][i] = ic[:, q]
            rv = (r[:, 0], r[:, 1], r[:, 2])
            u = [_dot3(B[i], rv) for i in range(3)]
            m = _dot3(rv, u)
            use = hit & np.isfinite(m) & (m >= 0.0)
            arg = d2h * m
            w = exp_neg(np.where(use, arg, 0.0))
            cut += int((use & (arg >= EXP_CUT)).sum())
            y = [[_dot3(B[i], cols[v]) for i in range(3)] for v in range(6)]
            t = 0
            for uu in range(6):
                for v in range(uu + 1):
                    acc[:, t] = np.where(use, acc[:, t] + w * _dot3(cols[uu], y[v]), acc[:, t])
                    t += 1
            for uu in range(6):
                acc[:, 21 + uu] = np.where(use, acc[:, 21 + uu] + w * _dot3(cols[uu], u), acc[:, 21 + uu])
            acc[:, 27] = np.where(use, acc[:, 27] + w, acc[:, 27])
        used_idx[:, j] = np.where(use, k, -1)
    n_used = (used_idx >= 0).sum(axis=1)
    corr = np.zeros(n, CORR_DTYPE)
    corr["idx"] = np.where(used_idx[:, 0] >= 0, used_idx[:, 0], NONE)
    corr["n_used"] = n_used
    corr["score"] = acc[:, 27]
    s = tree_sum(acc) if n else np.zeros(28)
    return dict(corr=corr, H=s[:21].copy(), g=s[21:27].copy(), score=float(s[27]), n_corr=int((n_used > 0).sum()), p0=p0,
                terms=acc, used=used_idx, cut=cut)


def align(src, tgt, cells, table, d2, leaf, min_b, div_b, guess=None, neighborhood=7, max_iterations=30, trans_eps=1e-6,
          rot_eps=1e-6, min_correspondences=6):
    """The loop (§16's). Returns the final evaluation's dict with pose (3, 4), iterations and flags added."""
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    T = IDENTITY.copy() if guess is None else np.asarray(guess, F64).reshape(3, 4).copy()
    p0 = pivot(tgt) if len(tgt) else np.zeros(3)
    lookup = voxel_dict(cells)
    ev = lambda: evaluate(src, tgt, cells, table, T, d2, leaf, min_b, div_b, neighborhood, p0, lookup)
    flags, it = 0, 0
    while it < max_iterations:
        e = ev()
        if e["n_corr"] < min_correspondences:
            break
        x = solve(e["H"], e["g"])
        if x is None:
            flags |= SINGULAR
            break
        T = update(T, x, p0)
        it += 1
        if norm3(x[:3]) < rot_eps and norm3(x[3:]) < trans_eps:
            flags |= CONVERGED
            break
    if max_iterations and it == max_iterations and not flags & CONVERGED:
        flags |= MAX_ITER_HIT
    e = ev()
    if e["n_corr"] < min_correspondences:
        flags |= FEW
    e.update(pose=T, iterations=it, flags=flags)
    return e
