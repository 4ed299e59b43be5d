"""numpy restatement of statistical outlier removal (cm_set_statistical_outlier, include/cloudmerge.h).

pcl::StatisticalOutlierRemoval::applyFilterIndices as the header states it, on the stage's input P (the fused cloud in
(sensor, point) order, as cm_merged_copy returns it with the stage off):
  d2 = (dx*dx + dy*dy) + dz*dz in fp32 over every other index; the k smallest; sqrtf of each (correctly rounded: numpy's
  float32 sqrt); added in ascending order one after the other in fp64 from 0; d_i = float32(sum / k);
  S = fsum(d_i), Q = fsum(float32(d_i * d_i)); mean = S / n, var = (Q - S*S/n) / (n - 1), stddev = sqrt(var),
  threshold = mean + std_mul * stddev; removed iff d_i > threshold. n <= k: d_i NaN, nothing removed, threshold +inf.

The k nearest neighbours come from an exact search without scipy: the points are bucketed in cubic cells, every point takes
the candidates of the 27 cells around its own, and a point whose k-th distance is not provably inside that block (or that
has fewer than k candidates) is searched again by brute force over the whole cloud. knn_d2_brute has no cells at all: every
pair, the point's own index left out. The probe frames (tests/sor_edge_frames.py) are judged by it, and the bucketed search
is checked against it there (tests/test_sor_edges.py). exact_sums gives S and Q as exact rationals."""
import math
from fractions import Fraction

import numpy as np


def _d2(q, p):
    """fp32 squared distances, (dx*dx + dy*dy) + dz*dz; q (m, 3) against p (m, 3) or broadcastable."""
    ex = (q[..., 0] - p[..., 0]).astype(np.float32)
    ey = (q[..., 1] - p[..., 1]).astype(np.float32)
    ez = (q[..., 2] - p[..., 2]).astype(np.float32)
    return ((ex * ex + ey * ey) + ez * ez).astype(np.float32)


def _brute(xyz, idx, k, chunk=64):
    """The k smallest d2 of the points idx against all others, ascending (float32, (len(idx), k))."""
    out = np.empty((len(idx), k), np.float32)
    for a in range(0, len(idx), chunk):
        sel = idx[a:a + chunk]
        d = _d2(xyz[sel][:, None, :], xyz[None, :, :])
        d[np.arange(len(sel)), sel] = np.inf                   # not the point itself (duplicates elsewhere do count)
        part = np.partition(d, k - 1, axis=1)[:, :k]
        out[a:a + len(sel)] = np.sort(part, axis=1)
    return out


def knn_d2(xyz, k, cell=None, chunk=20_000):
    """(n, k) float32: the k smallest squared distances of every point to the others, ascending."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    n = len(xyz)
    if cell is None:
        ext = float(np.max(xyz.max(0).astype(np.float64) - xyz.min(0).astype(np.float64))) if n else 1.0
        cell = max(ext / max(n, 1) ** (1 / 3) * 2.0, 1e-3)
    fl = np.floor(xyz.astype(np.float64) / cell)
    if n and float(np.prod(fl.max(0) - fl.min(0) + 3.0)) >= 2.0 ** 62:
        # (a cloud whose extent in cells overflows the int64 cell keys — one wider than FLT_MAX at any cell: every pair)
        return _brute(xyz, np.arange(n), k) if n > k else np.full((n, k), np.inf, np.float32)
    ijk = fl.astype(np.int64)
    ijk -= ijk.min(0)
    dims = ijk.max(0) + 3
    key = ((ijk[:, 2] + 1) * dims[1] + (ijk[:, 1] + 1)) * dims[0] + (ijk[:, 0] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ucell, start, cnt = np.unique(skey, return_index=True, return_counts=True)
    offs = [(dx + dy * dims[0] + dz * dims[0] * dims[1]) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    out = np.full((n, k), np.inf, np.float32)
    have = np.zeros(n, np.int64)
    for a in range(0, n, chunk):
        q = np.arange(a, min(n, a + chunk))
        qs, qc = [], []
        for o in offs:
            nk = key[q] + o
            pos = np.clip(np.searchsorted(ucell, nk), 0, len(ucell) - 1)
            hit = ucell[pos] == nk
            qs.append(np.where(hit, start[pos], 0))
            qc.append(np.where(hit, cnt[pos], 0))
        qs, qc = np.stack(qs, 1), np.stack(qc, 1)                # (m, 27)
        tot = qc.sum(1)
        have[q] = tot - 1
        rep_q = np.repeat(q, tot)
        flat_s, flat_c = qs.ravel(), qc.ravel()
        seg = np.repeat(flat_s - np.concatenate([[0], np.cumsum(flat_c)[:-1]]), flat_c)
        cand = order[np.arange(len(seg)) + seg]
        keep = cand != rep_q
        rep_q, cand = rep_q[keep], cand[keep]
        d = _d2(xyz[rep_q], xyz[cand])
        o2 = np.lexsort((d, rep_q))
        rep_q, d = rep_q[o2], d[o2]
        first = np.searchsorted(rep_q, q)
        for j in range(k):
            pos = first + j
            ok = (pos < len(rep_q)) & (pos < np.searchsorted(rep_q, q, side="right"))
            out[q[ok], j] = d[pos[ok]]
    # complete: k candidates and the k-th within one cell (the block's nearest face), with a margin for rounding
    bound = np.float32((cell * (1 - 1e-5)) ** 2)
    redo = np.nonzero((have < k) | ~(out[:, k - 1] <= bound))[0] if n > k else np.zeros(0, np.int64)
    if len(redo):
        out[redo] = _brute(xyz, redo, k)
    return out


def knn_d2_brute(xyz, k, chunk=128):
    """(n, k) float32: knn_d2 by brute force over every pair — no cells, no bounds, only the point's own index left out."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    n = len(xyz)
    out = np.empty((n, k), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, n, chunk):
            sel = np.arange(a, min(n, a + chunk))
            d = _d2(xyz[sel][:, None, :], xyz[None, :, :])
            d[np.arange(len(sel)), sel] = np.inf
            out[sel] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def distances(xyz, k, cell=None, brute=False):
    """d_i (float32) of every point; NaN everywhere when n <= k. brute: the k nearest from knn_d2_brute."""
    n = len(xyz)
    if n <= k:
        return np.full(n, np.nan, np.float32)
    d2 = knn_d2_brute(xyz, k) if brute else knn_d2(xyz, k, cell)
    r = np.sqrt(d2)                                              # float32, correctly rounded
    s = np.zeros(n)
    for j in range(k):
        s = s + r[:, j].astype(np.float64)
    return (s / k).astype(np.float32)


def stats(d, k, std_mul):
    """(mean, stddev, threshold) of the d_i as the header defines them (std_mul: rounded to fp32 first)."""
    d = np.asarray(d, np.float32)
    n = len(d)
    if n <= k:
        return math.nan, math.nan, math.inf
    S = math.fsum(d.astype(np.float64).tolist())
    Q = math.fsum((d * d).astype(np.float32).astype(np.float64).tolist())
    mean = S / n
    var = (Q - S * S / n) / (n - 1)
    sd = math.sqrt(var) if var >= 0 else math.nan
    return mean, sd, mean + float(np.float32(std_mul)) * sd


def exact_sums(d):
    """(S, Q) of finite d_i as exact rationals: sum d_i and sum fp32(d_i * d_i); None in place of a sum with an infinite term."""
    d = np.asarray(d, np.float32)
    with np.errstate(over="ignore"):
        sq = (d * d).astype(np.float32)
    S = None if np.isinf(d).any() else sum((Fraction(float(v)) for v in d), Fraction(0))
    Q = None if np.isinf(sq).any() else sum((Fraction(float(v)) for v in sq), Fraction(0))
    return S, Q


def keep_mask(d, threshold):
    """True: kept. A NaN threshold (or d_i) keeps the point."""
    d = np.asarray(d, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~(d > threshold)


def sor(xyz, k, std_mul, cell=None, brute=False):
    """(d, (mean, stddev, threshold), keep) of the cloud."""
    d = distances(xyz, k, cell, brute)
    st = stats(d, k, std_mul)
    return d, st, keep_mask(d, st[2])
