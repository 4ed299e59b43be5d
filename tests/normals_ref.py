"""Restatement of cm_result_normals (include/cloudmerge.h) in numpy.

neighbours_brute is the definition: the fp32 d2 of every pair, np.lexsort on (j, d2), the m - 1 first others. neighbours_tree
is the same answer for large inputs: a kd-tree's k + 8 nearest in fp64, their d2 recomputed in fp32, the lexicographic m - 1 of
them — and brute force for every point whose (k + 8)-th fp64 distance does not clear its chosen last d2 by a relative 1e-5
(the candidate set might then miss a tie). planes() restates steps 3 to 5 on those neighbourhoods: the sequential fp64 sums,
the covariance, and numpy.linalg.eigh of it: the independent cross-check of the device's normals, within tolerances and away
from small eigenvalue gaps. planes_exact() restates nrm_plane (cm_kernels_normals.hip) in the kernel's own order with the shared
Jacobi (tests/jacobi_ref.py): normal, curvature and flags of every entry bit for bit, degenerate and invalid ones included."""
import numpy as np

from tests import jacobi_ref

F32 = np.float32
VALID = 1
VOXEL_NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("curvature", "<f4"), ("r2_k", "<f4"), ("n_neighbors", "<u4"),
                               ("last", "<u4"), ("flags", "<u4")])


def d2_f32(a, b):
    """(dx*dx + dy*dy) + dz*dz in fp32, every operation rounded on its own (numpy contracts nothing)."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = a.astype(F32) - b.astype(F32)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _rows_brute(xyz, rows, m):
    """For every point of `rows`: its m - 1 nearest others by (d2, j), and their d2."""
    n = len(xyz)
    idx = np.empty((len(rows), m - 1), np.int64)
    d2 = np.empty((len(rows), m - 1), F32)
    jj = np.arange(n, dtype=np.int64)
    block = max(1, (1 << 22) // max(n, 1))
    for s in range(0, len(rows), block):
        r = np.asarray(rows[s:s + block], np.int64)
        d = d2_f32(xyz[r][:, None, :], xyz[None, :, :])
        order = np.lexsort((np.broadcast_to(jj, d.shape), d), axis=-1)[:, :m]
        keep = order != r[:, None]                                     # the point itself is in no list
        sel = np.argsort(~keep, axis=1, kind="stable")[:, :m - 1]
        o = np.take_along_axis(order, sel, 1)
        idx[s:s + block] = o
        d2[s:s + block] = np.take_along_axis(d, o, 1)
    return idx, d2


def neighbours_brute(xyz, k):
    xyz = np.ascontiguousarray(xyz, F32)
    n = len(xyz)
    return _rows_brute(xyz, np.arange(n), min(k, n))


def neighbours_tree(xyz, k, extra=8, stats=None):
    from scipy.spatial import cKDTree
    xyz = np.ascontiguousarray(xyz, F32)
    n = len(xyz)
    m = min(k, n)
    kq = min(k + extra, n)
    if m < 2 or kq < m + 1 or not np.isfinite(xyz).all():
        return neighbours_brute(xyz, k)
    p = xyz.astype(np.float64)
    dist, cand = cKDTree(p).query(p, k=kq)
    cand = cand.astype(np.int64)
    me = np.arange(n, dtype=np.int64)[:, None]
    is_self = cand == me
    d = d2_f32(xyz[:, None, :], xyz[cand])
    d_sort = np.where(is_self, F32(-1), d)                             # the point itself first, then dropped
    order = np.lexsort((cand, d_sort), axis=-1)
    cand, d = np.take_along_axis(cand, order, 1), np.take_along_axis(d, order, 1)
    idx, d2 = cand[:, 1:m].copy(), d[:, 1:m].copy()
    # sure only where the point itself was among the candidates and everything outside them is clearly farther
    with np.errstate(over="ignore", invalid="ignore"):
        sure = is_self.any(axis=1) & np.isfinite(d2[:, -1])
        if kq < n:
            sure &= dist[:, -1] ** 2 > d2[:, -1].astype(np.float64) * (1.0 + 1e-5)
    redo = np.nonzero(~sure)[0]
    if stats is not None:
        stats["brute_rows"] = len(redo)
    if len(redo):
        idx[redo], d2[redo] = _rows_brute(xyz, redo, m)
    return idx, d2


def planes(xyz, idx, viewpoint=(0.0, 0.0, 0.0)):
    """Steps 3 to 5 on the neighbourhoods idx (n, m - 1), in list order. Returns a dict: C (n, 3, 3) — the covariance exactly
    as specified —, evals (n, 3) ascending and normal (n, 3) from numpy.linalg.eigh, curvature, valid."""
    xyz = np.ascontiguousarray(xyz, F32)
    n = len(xyz)
    m = idx.shape[1] + 1
    p = xyz.astype(np.float64)
    s = np.zeros((n, 3))
    S = np.zeros((n, 3, 3))
    for q in range(m - 1):                                             # one neighbour after the other, every operation rounded
        e = p[idx[:, q]] - p
        s = s + e
        for a in range(3):
            for b in range(a + 1):
                S[:, a, b] = S[:, a, b] + e[:, a] * e[:, b]
    mu = s / float(m)
    Cm = np.zeros((n, 3, 3))
    for a in range(3):
        for b in range(a + 1):
            Cm[:, a, b] = S[:, a, b] / float(m) - mu[:, a] * mu[:, b]
            Cm[:, b, a] = Cm[:, a, b]
    with np.errstate(all="ignore"):
        fin = np.isfinite(Cm).all(axis=(1, 2))
        w, v = np.linalg.eigh(np.where(fin[:, None, None], Cm, 0.0))
        normal = v[:, :, 0].copy()
        vp = np.asarray(viewpoint, F32).astype(np.float64) - p
        flip = (normal * vp).sum(axis=1) < 0
        normal[flip] = -normal[flip]
        curv = np.abs(w[:, 0] / (w[:, 0] + w[:, 1] + w[:, 2]))
        valid = fin & (m >= 3) & (w[:, 2] > 0) & np.isfinite(curv)
    return dict(C=Cm, evals=w, normal=normal, curvature=curv, valid=valid, to_viewpoint=vp)


QNAN = np.uint32(0x7FC00000)


def planes_exact(xyz, idx, viewpoint=(0.0, 0.0, 0.0)):
    """nrm_plane on the neighbourhoods idx (n, m - 1) in list order, every step one rounded fp64 operation in the kernel's
    order: the differences double(p) - double(c) and their sequential sums; mu = s / m, C = S / m - mu mu^T; jacobi3; the
    select chain for the smallest eigenvalue (strict <: the first of equals keeps its column); hi = max; the eigenvector
    divided by sqrt((e0^2 + e1^2) + e2^2); cv = |lo / ((l0 + l1) + l2)|; the flip when ((e0 wx + e1 wy) + e2 wz) < 0 with
    w = double(viewpoint) - double(c); valid iff m >= 3, hi > 0 and hi, lo, e, cv finite; the quiet NaN 0x7FC00000 in
    normal and curvature where not. Returns a dict: normal (n, 3) and curvature (n,) float32, flags uint32 — the bits of
    the table — and diag (n, 3: the eigenvalues as jacobi3 left them), dot (the flip's sum), w."""
    xyz = np.ascontiguousarray(xyz, F32)
    n = len(xyz)
    kk = idx.shape[1]
    m = kk + 1
    normal = np.full((n, 3), QNAN, np.uint32).view(F32)
    curv = np.full(n, QNAN, np.uint32).view(F32)
    flags = np.zeros(n, np.uint32)
    out = dict(normal=normal, curvature=curv, flags=flags, diag=np.zeros((n, 3)), dot=np.zeros(n), w=np.zeros((n, 3)))
    if m < 3 or n == 0:
        return out
    p = xyz.astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.zeros((n, 3))
        S = {ab: np.zeros(n) for ab in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))}
        for q in range(kk):
            e = p[idx[:, q]] - p
            s = s + e
            for (a, b) in S:
                S[(a, b)] = S[(a, b)] + e[:, a] * e[:, b]
        dm = float(m)
        mu = s / dm
        Cm = np.empty((n, 3, 3))
        for (a, b), v in S.items():
            Cm[:, a, b] = v / dm - mu[:, a] * mu[:, b]
            Cm[:, b, a] = Cm[:, a, b]
        A, V = jacobi_ref.jacobi3(Cm)
        l0, l1, l2 = A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]
        z1 = l1 < l0
        lo = np.where(z1, l1, l0)
        ev = np.where(z1[:, None], V[:, :, 1], V[:, :, 0])
        z2 = l2 < lo
        lo = np.where(z2, l2, lo)
        ev = np.where(z2[:, None], V[:, :, 2], ev)
        hi = np.fmax(np.fmax(l0, l1), l2)
        ln = np.sqrt((ev[:, 0] * ev[:, 0] + ev[:, 1] * ev[:, 1]) + ev[:, 2] * ev[:, 2])
        ev = ev / ln[:, None]
        cv = np.abs(lo / ((l0 + l1) + l2))
        w = np.asarray(viewpoint, F32).astype(np.float64) - p
        dot = (ev[:, 0] * w[:, 0] + ev[:, 1] * w[:, 1]) + ev[:, 2] * w[:, 2]
        ev = np.where((dot < 0.0)[:, None], -ev, ev)
        ok = (hi > 0.0) & np.isfinite(hi) & np.isfinite(lo) & np.isfinite(ev).all(axis=1) & np.isfinite(cv)
        normal[ok] = ev[ok].astype(F32)
        curv[ok] = cv[ok].astype(F32)
    flags[ok] = VALID
    out.update(diag=np.stack([l0, l1, l2], axis=1), dot=dot, w=w, column=np.where(z2, 2, np.where(z1, 1, 0)))
    return out


def table(xyz, k, viewpoint=(0.0, 0.0, 0.0), tree=True, stats=None, exact=True):
    """(entries, planes): the table as cm_result_normals defines it — normal and curvature from eigh, rounded to fp32, so
    only n_neighbors, r2_k, last and flags are meant for bit comparison — and the fp64 figures behind it; with exact, also
    planes["exact"]: planes_exact() of the same neighbourhoods, whose normal, curvature and flags are the table's bits."""
    xyz = np.ascontiguousarray(xyz, F32)
    n = len(xyz)
    out = np.zeros(n, VOXEL_NORMAL_DTYPE)
    if n == 0:
        return out, None
    idx, d2 = (neighbours_tree(xyz, k, stats=stats) if tree else neighbours_brute(xyz, k))
    pl = planes(xyz, idx, viewpoint)
    m = idx.shape[1] + 1
    out["n_neighbors"] = m
    out["r2_k"] = d2[:, -1] if m > 1 else 0
    out["last"] = idx[:, -1] if m > 1 else np.arange(n)
    ok = pl["valid"]
    out["flags"] = np.where(ok, VALID, 0)
    out["normal"] = np.where(ok[:, None], pl["normal"], np.nan).astype(F32)
    out["curvature"] = np.where(ok, pl["curvature"], np.nan).astype(F32)
    pl["idx"], pl["d2"] = idx, d2
    if exact:
        pl["exact"] = planes_exact(xyz, idx, viewpoint)
    return out, pl
