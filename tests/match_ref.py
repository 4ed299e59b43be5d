"""A numpy restatement of the scan matching layer (include/cloudmerge.h, cm_map_match_evaluate), steps 1-8, written from the
header and independently of the kernels: the field table with the spelled-out exponential of tests/ndt_ref.py, the field as a table lookup of dist2, the candidate matrices in np.float32 with every operation rounded on
its own, D_k as sets of window cells, the volume by shifting a padded field under every cell of D_k, the best entry by a sort
key, the sub-cell offset in Python floats (IEEE double) and the pose. It takes the cloud A (cm_merged_copy) as an (n, 4)
float32 array, dist2 as the cost layer holds it ((ny, nx) uint32), the map's parameters and anchor, the heading table
(cm_traj_directions) and the prior pose."""
import math

import numpy as np

from tests import ndt_ref as nr

F32 = np.float32
MAX_RADIUS_CELLS = 64
MAX_SHIFT = 64
MAX_ANGLES = 127
MAX_CANDIDATES = 1 << 22
SUBCELL = 1
DIST_NONE = 0xFFFFFFFF
LIMIT = F32(1073741824.0)


def params(sigma=0.1, max_dist=0.3, n_a=2, a_stride=8, wx=3, wy=2, flags=0):
    return dict(sigma=sigma, max_dist=max_dist, n_a=n_a, a_stride=a_stride, wx=wx, wy=wy, flags=flags)


def radius(cell, max_dist):
    return int(math.ceil(float(F32(max_dist)) / float(F32(cell))))


def refusal(q, cell):
    """Why cm_map_match_configure refuses q over a map of this cell, or None."""
    for k in ("sigma", "max_dist"):
        v = F32(q[k])
        if not (np.isfinite(v) and v > 0):
            return k
    if radius(cell, q["max_dist"]) > MAX_RADIUS_CELLS:
        return "radius"
    if q["n_a"] > MAX_ANGLES or q["a_stride"] == 0 or q["n_a"] * q["a_stride"] > 1024:
        return "angles"
    if q["wx"] > MAX_SHIFT or q["wy"] > MAX_SHIFT:
        return "shift"
    if (2 * q["n_a"] + 1) * (2 * q["wx"] + 1) * (2 * q["wy"] + 1) > MAX_CANDIDATES:
        return "candidates"
    if q["flags"] & ~SUBCELL:
        return "flags"
    return None


def table(cell, sigma, max_dist):
    """Step 1: R * R + 1 bytes."""
    c, sg, md = float(F32(cell)), float(F32(sigma)), float(F32(max_dist))
    R = radius(cell, max_dist)
    two_s2 = (2.0 * sg) * sg
    lut = np.zeros(R * R + 1, np.uint8)
    lut[0] = 255
    for d2 in range(1, R * R + 1):
        m = math.sqrt(float(d2)) * c
        lut[d2] = 0 if m > md else int(math.floor(255.0 * nr.exp_neg((m * m) / two_s2)))
    return lut


def field(dist2, lut):
    """Step 2: (ny, nx) uint8."""
    d = np.asarray(dist2, np.uint32).astype(np.int64)
    inside = d < len(lut)
    return np.where(inside, lut[np.where(inside, d, 0)], 0).astype(np.uint8)


def candidates(P, q, tab):
    """Step 3: (2 n_a + 1, 2, 3) float32, rows 0 and 1 of every candidate's linear part."""
    P = np.asarray(P, F32).reshape(3, 4)
    out = np.zeros((2 * q["n_a"] + 1, 2, 3), F32)
    for kk in range(2 * q["n_a"] + 1):
        k = kk - q["n_a"]
        c, s = F32(tab[(k * q["a_stride"]) & 4095, 0]), F32(tab[(k * q["a_stride"]) & 4095, 1])
        for j in range(3):
            out[kk, 0, j] = F32(F32(c * P[0, j]) - F32(s * P[1, j]))
            out[kk, 1, j] = F32(F32(s * P[0, j]) + F32(c * P[1, j]))
    return out


def cells_of(A, Q, t, mq, anchor):
    """Step 4 for one candidate: the sorted distinct window cell indices ix + iy * nx."""
    nx, ny = mq["nx"], mq["ny"]
    A = np.asarray(A, F32).reshape(-1, 4)
    inv = F32(1.0) / F32(mq["cell"])
    x, y, z = A[:, 0], A[:, 1], A[:, 2]
    with np.errstate(all="ignore"):
        wx = ((Q[0, 0] * x + Q[0, 1] * y) + Q[0, 2] * z) + F32(t[0])
        wy = ((Q[1, 0] * x + Q[1, 1] * y) + Q[1, 2] * z) + F32(t[1])
        assert wx.dtype == F32 and wy.dtype == F32
        cx, cy = np.floor(wx * inv), np.floor(wy * inv)
        ok = (cx > -LIMIT) & (cx < LIMIT) & (cy > -LIMIT) & (cy < LIMIT)
        ok &= (F32(mq["z_band"][0]) <= z) & (z <= F32(mq["z_band"][1]))
    gx = np.where(ok, cx, 0).astype(np.int64) - anchor[0]
    gy = np.where(ok, cy, 0).astype(np.int64) - anchor[1]
    ok &= (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny)
    return np.unique((gx + gy * nx)[ok])


def volume(D, L, q):
    """Step 5: (2 n_a + 1, 2 wy + 1, 2 wx + 1) uint32 from the cell sets D[kk] and the field L."""
    ny, nx = L.shape
    wx, wy = q["wx"], q["wy"]
    pad = np.zeros((ny + 2 * wy, nx + 2 * wx), np.int64)
    pad[wy:wy + ny, wx:wx + nx] = L
    vol = np.zeros((len(D), 2 * wy + 1, 2 * wx + 1), np.int64)
    for kk, cells in enumerate(D):
        for c in cells.tolist():
            ix, iy = c % nx, c // nx
            vol[kk] += pad[iy:iy + 2 * wy + 1, ix:ix + 2 * wx + 1]      # entry [j + wy, i + wx] is L(c + (i, j))
    assert vol.max(initial=0) < 1 << 32
    return vol.astype(np.uint32)


def best_of(vol, q):
    """Step 6: the entry index."""
    n_a, wx, wy = q["n_a"], q["wx"], q["wy"]
    best, key = None, None
    for e, s in enumerate(vol.reshape(-1).tolist()):
        i, j, k = e % (2 * wx + 1) - wx, (e // (2 * wx + 1)) % (2 * wy + 1) - wy, e // ((2 * wx + 1) * (2 * wy + 1)) - n_a
        cand = (-s, i * i + j * j, abs(k), e)
        if key is None or cand < key:
            best, key = e, cand
    return best


def sub_of(lo, mid, hi):
    """Step 7 along one axis; lo or hi None: that neighbour does not exist."""
    if lo is None or hi is None:
        return 0.0
    den = int(lo) - 2 * int(mid) + int(hi)
    if den >= 0:
        return 0.0
    return min(0.5, max(-0.5, 0.5 * float(int(lo) - int(hi)) / float(den)))


def match(A, dist2, mq, anchor, q, P, tab):
    """Steps 1-8: (volume, result dictionary). The result holds the cm_match_result fields and D, the cell sets."""
    assert refusal(q, mq["cell"]) is None
    P = np.asarray(P, F32).reshape(3, 4)
    L = field(dist2, table(mq["cell"], q["sigma"], q["max_dist"]))
    Q = candidates(P, q, tab)
    D = [cells_of(A, Q[kk], (P[0, 3], P[1, 3]), mq, anchor) for kk in range(len(Q))]
    vol = volume(D, L, q)
    n_a, wx, wy = q["n_a"], q["wx"], q["wy"]
    best = best_of(vol, q)
    kk, jj, ii = best // ((2 * wx + 1) * (2 * wy + 1)), (best // (2 * wx + 1)) % (2 * wy + 1), best % (2 * wx + 1)
    k, j, i = kk - n_a, jj - wy, ii - wx
    sub = [0.0, 0.0]
    if q["flags"] & SUBCELL:
        sub[0] = sub_of(vol[kk, jj, ii - 1] if ii > 0 else None, vol[kk, jj, ii], vol[kk, jj, ii + 1] if ii < 2 * wx else None)
        sub[1] = sub_of(vol[kk, jj - 1, ii] if jj > 0 else None, vol[kk, jj, ii], vol[kk, jj + 1, ii] if jj < 2 * wy else None)
    pose = np.zeros((3, 4), F32)
    pose[:2, :3] = Q[kk]
    cell = float(F32(mq["cell"]))
    pose[0, 3] = F32(P[0, 3] + F32((float(i) + sub[0]) * cell))
    pose[1, 3] = F32(P[1, 3] + F32((float(j) + sub[1]) * cell))
    pose[2] = P[2]
    res = dict(best=best, k=k, i=i, j=j, score=int(vol[kk, jj, ii]), n_cells=len(D[kk]), max_score=255 * len(D[kk]),
               yaw=F32(float(k * q["a_stride"]) * (6.283185307179586 / 4096.0)), sub=tuple(sub), pose=pose, D=D, L=L)
    return vol, res
