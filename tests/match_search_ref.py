"""A plain Python restatement of the search layer (include/cloudmerge.h, cm_map_match_search), written from the header and
independently of the kernels. Steps 1 to 4 are tests/match_ref.py's (table, field, candidates, cells_of); here are the refusals,
the pyramid by its definition (a maximum over 2^h x 2^h cells of the zero-extended field, not level by level), a node's bound as
a sum over the cell set, the roots, the descent for B, the level loop with its counts, the capacities, and the best entry by a
sort key over the live leaves. exhaustive() is the plain steps 5 and 6 over the wide range, with nothing pruned: what the
search must equal."""
import numpy as np

from tests import match_ref as mf

F32 = np.float32
MAX_SHIFT = 1024
MAX_DEPTH = 7
MAX_NODES = 1 << 22
OVERFLOW_CELLS = -2
SUBCELL = 1


def params(sigma=0.1, max_dist=0.3, n_a=0, a_stride=8, wx=3, wy=2, depth=1, max_nodes=1 << 16, max_cells=1 << 16, flags=0):
    return dict(sigma=sigma, max_dist=max_dist, n_a=n_a, a_stride=a_stride, wx=wx, wy=wy, depth=depth, max_nodes=max_nodes, max_cells=max_cells,
                flags=flags)


def roots_along(w, depth):
    return -(-(2 * w + 1) // (1 << depth))


def n_roots(q):
    return (2 * q["n_a"] + 1) * roots_along(q["wx"], q["depth"]) * roots_along(q["wy"], q["depth"])


def refusal(q, cell, nx=1, ny=1):
    """Why cm_map_match_search_configure refuses q over a map of this cell and window, or None."""
    for k in ("sigma", "max_dist"):
        v = F32(q[k])
        if not (np.isfinite(v) and v > 0):
            return k
    if mf.radius(cell, q["max_dist"]) > mf.MAX_RADIUS_CELLS:
        return "radius"
    if q["n_a"] > mf.MAX_ANGLES or q["a_stride"] == 0 or q["n_a"] * q["a_stride"] > 1024:
        return "angles"
    if q["wx"] > MAX_SHIFT or q["wy"] > MAX_SHIFT:
        return "shift"
    if q["depth"] > MAX_DEPTH:
        return "depth"
    if not 1 <= q["max_nodes"] <= MAX_NODES:
        return "max_nodes"
    if not 1 <= q["max_cells"] <= MAX_NODES:
        return "max_cells"
    if n_roots(q) > q["max_nodes"]:
        return "roots"
    if nx > 65535 or ny > 65535:
        return "window"
    if q["flags"] & ~SUBCELL:
        return "flags"
    return None


def level(L, h):
    """Step 6a: (ny + 2^h - 1, nx + 2^h - 1) uint8, entry [y + 2^h - 1, x + 2^h - 1] = max of L over [x, x + 2^h) x [y, y + 2^h)."""
    ny, nx = L.shape
    s = 1 << h
    pad = np.zeros((ny + 2 * (s - 1), nx + 2 * (s - 1)), np.uint8)
    pad[s - 1:s - 1 + ny, s - 1:s - 1 + nx] = L
    rows = np.zeros((pad.shape[0], nx + s - 1), np.uint8)          # the maximum over a square: over a first, then over b
    for a in range(s):
        np.maximum(rows, pad[:, a:a + nx + s - 1], out=rows)
    out = np.zeros((ny + s - 1, nx + s - 1), np.uint8)
    for b in range(s):
        np.maximum(out, rows[b:b + ny + s - 1], out=out)
    return out


class Scorer:
    """U of a node: the level's table under the candidate's cells, shifted; 0 outside the storage."""

    def __init__(self, L, D, depth):
        self.ny, self.nx = L.shape
        self.levels = [level(L, h) for h in range(depth + 1)]
        self.xy = [(np.asarray(c, np.int64) % self.nx, np.asarray(c, np.int64) // self.nx) for c in D]
        self.n = 0                                     # nodes scored, for the tests' own curiosity

    def U(self, h, kk, i0, j0):
        self.n += 1
        t = self.levels[h]
        off = (1 << h) - 1
        x, y = self.xy[kk][0] + i0 + off, self.xy[kk][1] + j0 + off
        ok = (x >= 0) & (x < t.shape[1]) & (y >= 0) & (y < t.shape[0])
        return int(t[y[ok], x[ok]].astype(np.int64).sum())


def children(node, q):
    h, kk, i0, j0 = node
    s = 1 << (h - 1)
    return [(h - 1, kk, i0 + a * s, j0 + b * s) for b in (0, 1) for a in (0, 1) if i0 + a * s <= q["wx"] and j0 + b * s <= q["wy"]]


def order(node):
    return (node[1], node[3], node[2])                 # ascending (k + n_a, j0, i0)


def first_largest(nodes, us):
    """The node of the largest U, ties to the first in node order."""
    return min(zip(nodes, us), key=lambda t: (-t[1], order(t[0])))[0]


def new_info(q):
    return dict(depth=q["depth"], n_roots=n_roots(q), bound=0, scored=[0] * 8, live=[0] * 8, n_probe=0, overflow_level=-1)


def search(D, L, q):
    """Steps 5 and 6 by 6a-6f: (status, best, info, scores) with status "ok" or "capacity", best = (kk, jj, ii) or None, scores
    a dictionary of the live leaves' S."""
    info = new_info(q)
    if any(len(d) > q["max_cells"] for d in D):
        info["overflow_level"] = OVERFLOW_CELLS
        return "capacity", None, info, None
    sc = Scorer(L, D, q["depth"])
    wx, wy, depth = q["wx"], q["wy"], q["depth"]
    roots = [(depth, kk, -wx + (a << depth), -wy + (b << depth)) for kk in range(len(D)) for b in range(roots_along(wy, depth))
             for a in range(roots_along(wx, depth))]
    assert len(roots) == info["n_roots"] and roots == sorted(roots, key=order)
    u_roots = [sc.U(*n) for n in roots]
    # 6d: the descent
    node = first_largest(roots, u_roots)
    u_node = u_roots[roots.index(node)]
    n_probe = 1
    while node[0] > 0:
        ch = children(node, q)
        us = [sc.U(*n) for n in ch]
        n_probe += len(ch)
        node = first_largest(ch, us)
        u_node = us[ch.index(node)]
    B = max(u_node, sc.U(0, q["n_a"], 0, 0))
    info["bound"], info["n_probe"] = B, n_probe
    # 6e: the level loop
    info["scored"][depth] = len(roots)
    live = [(n, u) for n, u in zip(roots, u_roots) if u >= B]
    info["live"][depth] = len(live)
    for h in range(depth, 0, -1):
        ch = [c for n, _ in live for c in children(n, q)]
        info["scored"][h - 1] = len(ch)
        if len(ch) > q["max_nodes"]:
            info["overflow_level"] = h - 1
            return "capacity", None, info, None
        live = [(c, u) for c, u in ((c, sc.U(*c)) for c in ch) if u >= B]
        info["live"][h - 1] = len(live)
    best = min(live, key=lambda t: (-t[1], t[0][2] ** 2 + t[0][3] ** 2, abs(t[0][1] - q["n_a"]), order(t[0])))[0]
    scores = {(n[1], n[3] + wy, n[2] + wx): u for n, u in live}
    return "ok", (best[1], best[3] + wy, best[2] + wx), info, scores


def leaf(D, L, kk, i, j):
    """S(k, i, j) by step 5."""
    ny, nx = L.shape
    c = np.asarray(D[kk], np.int64)
    x, y = c % nx + i, c // nx + j
    ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
    return int(L[y[ok], x[ok]].astype(np.int64).sum())


def exhaustive(D, L, q):
    """The plain steps 5 and 6 over the wide range: (best (kk, jj, ii), its score). One shifted gather per entry row."""
    ny, nx = L.shape
    wx, wy = q["wx"], q["wy"]
    pad = np.zeros((ny + 2 * wy, nx + 2 * wx), np.int64)
    pad[wy:wy + ny, wx:wx + nx] = L
    best, key = None, None
    ii = np.arange(2 * wx + 1)
    for kk, cells in enumerate(D):
        c = np.asarray(cells, np.int64)
        x, y = c % nx, c // nx
        for jj in range(2 * wy + 1):
            row = pad[(y + jj)[:, None], x[:, None] + ii[None, :]].sum(axis=0) if len(c) else np.zeros(2 * wx + 1, np.int64)
            for i_ in np.flatnonzero(row == row.max()).tolist():     # (only a row's largest entries can win)
                cand = (-int(row[i_]), (i_ - wx) ** 2 + (jj - wy) ** 2, abs(kk - q["n_a"]), kk, jj, i_)
                if key is None or cand < key:
                    best, key = (kk, jj, i_), cand
    return best, -key[0]


def finish(D, L, q, P, Q, cell, best):
    """Steps 7 and 8 for the best entry (kk, jj, ii): the cm_match_result fields."""
    wx, wy, n_a = q["wx"], q["wy"], q["n_a"]
    kk, jj, ii = best
    k, j, i = kk - n_a, jj - wy, ii - wx
    s0 = leaf(D, L, kk, i, j)
    sub = [0.0, 0.0]
    if q["flags"] & SUBCELL:
        sub[0] = mf.sub_of(leaf(D, L, kk, i - 1, j) if ii > 0 else None, s0, leaf(D, L, kk, i + 1, j) if ii < 2 * wx else None)
        sub[1] = mf.sub_of(leaf(D, L, kk, i, j - 1) if jj > 0 else None, s0, leaf(D, L, kk, i, j + 1) if jj < 2 * wy else None)
    P = np.asarray(P, F32).reshape(3, 4)
    pose = np.zeros((3, 4), F32)
    pose[:2, :3] = Q[kk]
    c = float(F32(cell))
    pose[0, 3] = F32(P[0, 3] + F32((float(i) + sub[0]) * c))
    pose[1, 3] = F32(P[1, 3] + F32((float(j) + sub[1]) * c))
    pose[2] = P[2]
    return dict(best=(kk * (2 * wy + 1) + jj) * (2 * wx + 1) + ii, k=k, i=i, j=j, score=s0, n_cells=len(D[kk]), max_score=255 * len(D[kk]),
                yaw=F32(float(k * q["a_stride"]) * (6.283185307179586 / 4096.0)), sub=tuple(sub), pose=pose)


def inputs(A, dist2, mq, anchor, q, P, tab):
    """Steps 1 to 4 from tests/match_ref.py: (L, Q, D)."""
    P = np.asarray(P, F32).reshape(3, 4)
    L = mf.field(dist2, mf.table(mq["cell"], q["sigma"], q["max_dist"]))
    Q = mf.candidates(P, q, tab)
    D = [mf.cells_of(A, Q[kk], (P[0, 3], P[1, 3]), mq, anchor) for kk in range(len(Q))]
    return L, Q, D


def match(A, dist2, mq, anchor, q, P, tab):
    """Steps 1 to 8: (status, result dictionary or None, info, (L, Q, D))."""
    assert refusal(q, mq["cell"], mq["nx"], mq["ny"]) is None
    L, Q, D = inputs(A, dist2, mq, anchor, q, P, tab)
    status, best, info, _ = search(D, L, q)
    res = finish(D, L, q, P, Q, mq["cell"], best) if status == "ok" else None
    return status, res, info, (L, Q, D)
