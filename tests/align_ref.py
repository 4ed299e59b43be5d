"""Restatement of cm_result_align (include/cloudmerge.h) in numpy: explicit per-operation fp64, no BLAS
products anywhere.

match_brute is the definition of step 2: the fp32 d2 of every (source, target) pair, the smallest (d2, j) below float(r*r).
match_tree is the same answer for large inputs: a kd-tree's 12 nearest within r (1 + 1e-5) in fp64, their d2 recomputed in
fp32, the lexicographic best of them — and brute force for every source point whose candidate list is full and whose last
fp64 distance does not clear the chosen d2 by a relative 1e-5 (a tie might then be missing). terms() restates step 3 on
the target's normals table — an input: the table is cm_result_normals', pinned by tests/test_normals.py —, tree_sum() step
4 by reshaping to (blocks, 4, 64), solve() and update() the host's LDL^T and pose update operation for operation
(cm_align_solve.hpp), align() the loop."""
import math

import numpy as np

from tests.normals_ref import d2_f32

F32 = np.float32
F64 = np.float64
NONE = 0xFFFFFFFF
PIVOT_MIN = 1e-9
MAX_ITER = 64
CONVERGED, MAX_ITER_HIT, FEW, SINGULAR = 1, 2, 4, 8
NORMAL_VALID = 1
CORR_DTYPE = np.dtype([("idx", "<u4"), ("d2", "<f4")])
IDENTITY = np.eye(3, 4)


def pivot(tgt):
    tgt = np.asarray(tgt, F32).reshape(-1, 3)
    mn, mx = tgt.min(axis=0).astype(F64), tgt.max(axis=0).astype(F64)
    return mn + (mx - mn) * 0.5


def transform(src, T):
    """Step 1: (q64, qf)."""
    T = np.asarray(T, F64).reshape(3, 4)
    x, y, z = (np.asarray(src, F32)[:, a].astype(F64) for a in range(3))
    with np.errstate(all="ignore"):
        q64 = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)
        return q64, q64.astype(F32)


def _r2(r):
    return F32(r) * F32(r)


def _rows_brute(qf, tgt, r2, rows):
    idx = np.full(len(rows), NONE, np.uint32)
    d2 = np.zeros(len(rows), F32)
    if len(tgt) == 0:
        return idx, d2
    block = max(1, (1 << 22) // len(tgt))
    for s in range(0, len(rows), block):
        q = qf[rows[s:s + block]]
        d = d2_f32(q[:, None, :], tgt[None, :, :])
        with np.errstate(invalid="ignore"):
            ok = (d < r2) & np.isfinite(q).all(axis=1)[:, None]
        j = np.where(ok, d, F32(np.inf)).argmin(axis=1)                  # the first of equal minima: the smallest index
        hit = ok.any(axis=1)
        idx[s:s + block] = np.where(hit, j, NONE)
        d2[s:s + block] = np.where(hit, d[np.arange(len(q)), j], 0)
    return idx, d2


def match_brute(qf, tgt, r):
    qf, tgt = np.ascontiguousarray(qf, F32), np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    return _rows_brute(qf, tgt, _r2(r), np.arange(len(qf)))


def match_tree(qf, tgt, r, kq=12, stats=None):
    from scipy.spatial import cKDTree
    qf, tgt = np.ascontiguousarray(qf, F32), np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    n, r2 = len(qf), _r2(r)
    idx = np.full(n, NONE, np.uint32)
    d2 = np.zeros(n, F32)
    fin = np.isfinite(qf).all(axis=1)
    rows = np.nonzero(fin)[0]
    if len(tgt) < kq + 1 or not len(rows):
        return match_brute(qf, tgt, r)
    dist, cand = cKDTree(tgt.astype(F64)).query(qf[rows].astype(F64), k=kq, distance_upper_bound=float(r) * (1 + 1e-5))
    found = np.isfinite(dist)                                              # (a missing candidate: distance inf, index n)
    cand = np.where(found, cand, 0).astype(np.int64)
    d = d2_f32(qf[rows][:, None, :], tgt[cand])
    with np.errstate(invalid="ignore"):
        ok = found & (d < r2)
    key_d = np.where(ok, d, F32(np.inf))
    key_j = np.where(ok, cand, len(tgt))
    best = np.lexsort((key_j, key_d), axis=-1)[:, 0]
    ar = np.arange(len(rows))
    hit = ok[ar, best]
    bd = d[ar, best]
    # sure: the list is not full (everything within the radius was seen), or what lies beyond it is clearly farther than
    # the chosen pair
    full = found.all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        clear = hit & (dist[:, -1] ** 2 > bd.astype(F64) * (1 + 1e-5))
    sure = ~full | clear
    idx[rows] = np.where(hit, cand[ar, best], NONE)
    d2[rows] = np.where(hit, bd, 0)
    redo = rows[~sure]
    if stats is not None:
        stats["brute_rows"] = len(redo)
    if len(redo):
        idx[redo], d2[redo] = _rows_brute(qf, tgt, r2, redo)
    return idx, d2


def terms(q64, tgt, normals, idx, p0):
    """Step 3: (n, 28) terms — zeros where there are none — and the mask of the rows that have them."""
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    n = len(q64)
    t = np.zeros((n, 28))
    has = idx != NONE
    j = np.where(has, idx, 0).astype(np.int64)
    if len(tgt):
        has &= (normals["flags"][j] & NORMAL_VALID) != 0
    else:
        has[:] = False
    rows = np.nonzero(has)[0]
    if not len(rows):
        return t, has
    j = j[rows]
    a = q64[rows] - p0
    b = tgt[j].astype(F64) - p0
    nn = normals["normal"][j].astype(F64)
    e = a - b
    res = (nn[:, 0] * e[:, 0] + nn[:, 1] * e[:, 1]) + nn[:, 2] * e[:, 2]
    J = [a[:, 1] * nn[:, 2] - a[:, 2] * nn[:, 1], a[:, 2] * nn[:, 0] - a[:, 0] * nn[:, 2], a[:, 0] * nn[:, 1] - a[:, 1] * nn[:, 0],
         nn[:, 0], nn[:, 1], nn[:, 2]]
    k = 0
    for u in range(6):
        for v in range(u + 1):
            t[rows, k] = J[u] * J[v]
            k += 1
    for u in range(6):
        t[rows, 21 + u] = J[u] * res
    t[rows, 27] = res * res
    return t, has


def tree_sum(t):
    """Step 4 on (n, m) terms: (m,) sums."""
    t = np.asarray(t, F64)
    n, m = t.shape
    nb = (n + 255) // 256
    v = np.zeros((nb * 256, m))
    v[:n] = t
    v = v.reshape(nb, 4, 64, m)
    s = 32
    while s >= 1:
        v = v[:, :, :s] + v[:, :, s:2 * s]
        s //= 2
    w = v[:, :, 0]
    blk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    acc = np.add.accumulate(np.concatenate([np.zeros((1, m)), blk]), axis=0)     # one after the other, from 0.0
    return acc[-1]


def evaluate(src, tgt, normals, T, r, p0=None, tree=True, order=None):
    """E(T). order: a permutation of the source under which the sums are formed instead (to see what the order does)."""
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    p0 = pivot(tgt) if p0 is None and len(tgt) else (np.zeros(3) if p0 is None else np.asarray(p0, F64))
    q64, qf = transform(src, T)
    idx, d2 = (match_tree if tree else match_brute)(qf, tgt, r)
    t, has = terms(q64, tgt, normals, idx, p0)
    s = tree_sum(t if order is None else t[order])
    corr = np.zeros(len(idx), CORR_DTYPE)
    corr["idx"], corr["d2"] = idx, d2
    return dict(corr=corr, H=s[:21].copy(), g=s[21:27].copy(), sse=float(s[27]), n_corr=int(has.sum()), p0=p0)


def solve(H21, g):
    """H x = -g by LDL^T without pivoting, as cm_align_solve does it. None: singular."""
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i + 1):
            A[i, j] = H21[k]
            k += 1
    top = A[0, 0]
    for i in range(1, 6):
        top = A[i, i] if A[i, i] > top else top
    thr = F64(PIVOT_MIN) * top
    L, d, y, x = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j, j]
            for k in range(j):
                dj = dj - (L[j, k] * L[j, k]) * d[k]
            if not dj > thr:
                return None
            d[j] = dj
            for i in range(j + 1, 6):
                s = A[i, j]
                for k in range(j):
                    s = s - (L[i, k] * L[j, k]) * d[k]
                L[i, j] = s / dj
        for i in range(6):
            s = -F64(g[i])
            for k in range(i):
                s = s - L[i, k] * y[k]
            y[i] = s
        for i in range(5, -1, -1):
            s = y[i] / d[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s
    return x


def norm3(a):
    return float(np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))


def update(T, x, p0):
    """The twist x = (w, v) about p0 applied to the (3, 4) pose T, as cm_align_update does it."""
    T = np.asarray(T, F64).reshape(3, 4)
    x = np.asarray(x, F64)
    th = norm3(x)
    W = np.eye(3)
    if th > 0.0:
        k0, k1, k2 = x[0] / th, x[1] / th, x[2] / th
        s, h = F64(math.sin(th)), F64(math.sin(th * 0.5))
        c1 = (2.0 * h) * h
        K = np.array([[0.0, -k2, k1], [k2, 0.0, -k0], [-k1, k0, 0.0]])
        for i in range(3):
            for j in range(3):
                kk = (K[i, 0] * K[0, j] + K[i, 1] * K[1, j]) + K[i, 2] * K[2, j]
                W[i, j] = (W[i, j] + s * K[i, j]) + c1 * kk
    u = T[:, 3] - p0
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = (W[i, 0] * T[0, j] + W[i, 1] * T[1, j]) + W[i, 2] * T[2, j]
        wu = (W[i, 0] * u[0] + W[i, 1] * u[1]) + W[i, 2] * u[2]
        out[i, 3] = (wu + p0[i]) + x[3 + i]
    return out


def align(src, tgt, normals, r, guess=None, max_iterations=30, trans_eps=1e-6, rot_eps=1e-6, min_correspondences=6, tree=True,
          order=None):
    """The loop. Returns the final evaluation's dict with pose (3, 4), iterations, flags, rms added."""
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 3)
    T = IDENTITY.copy() if guess is None else np.asarray(guess, F64).reshape(3, 4).copy()
    p0 = pivot(tgt) if len(tgt) else np.zeros(3)
    flags, it = 0, 0
    while it < max_iterations:
        e = evaluate(src, tgt, normals, T, r, p0, tree, order)
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
    e = evaluate(src, tgt, normals, T, r, p0, tree, order)
    if e["n_corr"] < min_correspondences:
        flags |= FEW
    e.update(pose=T, iterations=it, flags=flags, rms=math.sqrt(e["sse"] / e["n_corr"]) if e["n_corr"] else 0.0)
    return e
