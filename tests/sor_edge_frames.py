"""Probe frames for statistical outlier removal (cm_set_statistical_outlier; cm_kernels_sor.hip k_sor_knn):
small clouds at the places where the exact k-nearest-neighbour search can stop too early, where fp32 flushes or overflows,
and at the edges of the statistics.

Every frame is one cloud with the identity pose and translation -0.0 (tests/edge_frames.py: xf_row then keeps every
coordinate's bits, a -0.0 included), so the stage's input is the raw points in order; tests/test_sor_edges.py asserts that
with merged_input. The expectation is tests/sor_ref.py with knn_d2_brute (every pair, no cells) unless a probe names a hand
derivation. Each family's docstring names the branch of k_sor_knn it drives:
  first-launch exit  the k-th d2 against the nearest face of the 3x3x3 block (axis_gap with kRel and |coord| 2^-21)
  listed point       the first launch puts the point on the list with its k-th d2 (or +inf) as the bound
  ring break         the second launch stops once ring s - 1 lies beyond the k-th d2
  row skip           the second launch skips a row whose (y,z) gap exceeds the current k-th d2
  x_range clipping   the second launch scans only the cells of a row within the current bound in x
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from cloud_merger_amd.types import xyzi_cloud
from tests.edge_frames import IDENT_Q, PROBE_T, ulps

F = np.float32
KREL = F(1.0) - F(1.0) / F(1 << 20)                    # kRel of cm_kernels_sor.hip
CELLS = (0.0, 1e-6, 1e3)                               # search cells every family runs with, besides its own


@dataclass
class Probe:
    name: str
    family: str
    xyz: np.ndarray                                    # (n, 3) float32, finite
    k: int
    std_mul: float = 1.0
    cells: Tuple[float, ...] = ()                      # the family's own search cells (0: the library's choice)
    crop: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None
    expect_d: Optional[np.ndarray] = None              # a hand derivation of d_i, where the family has one
    expect_removed: Optional[int] = None
    note: str = ""
    leaf: float = 0.5
    extra: dict = field(default_factory=dict)

    def sensors(self):
        xyz = np.asarray(self.xyz, np.float32)
        return [xyzi_cloud(xyz, np.arange(len(xyz), dtype=np.float32), q_xyzw=IDENT_Q, t_xyz=PROBE_T)]

    def all_cells(self):
        out = []
        for c in tuple(self.cells) + CELLS:
            if c not in out:
                out.append(c)
        return out


def pts(*rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def local_scene(n=3000, seed=0):
    """A few thousand points of a street: noisy ground, a wall, a pole, exact duplicates and a few isolated returns."""
    rng = np.random.default_rng(seed)
    m = n - 60
    xyz = np.empty((m, 3))
    xyz[:, 0] = rng.uniform(-8, 8, m)
    xyz[:, 1] = rng.uniform(-8, 8, m)
    xyz[:, 2] = rng.normal(-1.5, 0.02, m)
    wall = rng.random(m) < 0.3
    xyz[wall, 1] = 5.0 + rng.normal(0, 0.01, wall.sum())
    xyz[wall, 2] = rng.uniform(-1.5, 2.0, wall.sum())
    pole = rng.random(m) < 0.05
    xyz[pole, 0] = 2.0 + rng.normal(0, 0.02, pole.sum())
    xyz[pole, 1] = -3.0 + rng.normal(0, 0.02, pole.sum())
    xyz[pole, 2] = rng.uniform(-1.5, 4.0, pole.sum())
    far = rng.uniform(-1, 1, (20, 3)) * 25.0
    return np.concatenate([xyz, xyz[rng.integers(0, m, 40)], far]).astype(np.float32)


# ---- the first launch's exit test, restated in fp32 (used to place probes only; the expectation is the brute force) ------
def axis_gap(s, cell, coord):
    return max(F(F(F(F(s) * F(cell)) * KREL) - F(F(abs(F(coord))) * F(2.0 ** -21))), F(0.0))


def exit_bound(p, cell, krel=KREL, coord_term=True):
    """fl(fl(g*g) * kRel) for a point whose block has faces on every axis: g is the smallest axis_gap(1, cx, coord).
    krel / coord_term: the same bound with kRel = 1 or without the |coord| 2^-21 term (what a thinner margin would use)."""
    cx = F(1.0) / (F(1.0) / F(cell))
    g = None
    for a in range(3):
        t = F(F(abs(F(p[a]))) * F(2.0 ** -21)) if coord_term else F(0.0)
        ga = max(F(F(F(cx) * krel) - t), F(0.0))
        g = ga if g is None else min(g, ga)
    return F(F(g * g) * krel)


def cell_of(x, inv):
    return int(np.floor(F(F(x) * inv)))


def edge_of_cell(i, inv, top):
    """The largest (top) or smallest fp32 x with floor(fl(x * inv)) == i; None when the cell holds no fp32 value."""
    x = F((i + (1 if top else 0)) / float(inv))
    step = -1 if top else 1
    for _ in range(64):                                # move onto the cell, then to its edge
        c = cell_of(x, inv)
        if (top and c > i) or (not top and c < i):
            x = ulps(x, step)
        else:
            break
    if cell_of(x, inv) != i:
        return None
    for _ in range(1 << 12):
        nx = ulps(x, -step)
        if cell_of(nx, inv) != i:
            return x
        x = nx
    return None


def offset_for(target, lo_ok=False):
    """(dy, dz) with fl(fl(dy*dy) + fl(dz*dz)) == target (fp32), or None. lo_ok: the largest value <= target instead."""
    target = F(target)
    best = None
    y0 = F(np.sqrt(np.float64(target)))
    for sy in range(-40, 8):
        dy = ulps(y0, sy) if sy else y0
        a = F(dy * dy)
        if a > target:
            continue
        if a == target:
            return dy, F(0.0)
        rest = float(target) - float(a)
        z0 = F(np.sqrt(rest))
        for sz in range(-6, 7):
            dz = ulps(z0, sz) if sz else z0
            v = F(a + F(dz * dz))
            if v == target:
                return dy, dz
            if lo_ok and v < target and (best is None or v > best[0]):
                best = (v, dy, dz)
    return (best[1], best[2]) if best else None


# ---- a. far from the origin ----------------------------------------------------------------------------------------------
def family_a():
    """The same local scene translated by +-1e3 ... +-1e6 m along each axis in turn, with search cells of 0.05 m, 0.5 m
    and the library's choice, with and without a crop box around it. At 1e6 m an fp32 step is 6 cm: the |coord| 2^-21
    terms of axis_gap and x_range (first-launch exit, ring break, row skip, x_range clipping) are larger than a 5 cm cell,
    so most points are listed and every branch of the second launch runs with the margins at their widest."""
    base = local_scene(2500, seed=1)
    out = []
    for mag in (1e3, 1e4, 1e5, 1e6):
        for axis in range(3):
            for sign in (1.0, -1.0):
                t = np.zeros(3)
                t[axis] = sign * mag
                xyz = (base.astype(np.float64) + t).astype(np.float32)
                lo = tuple(float(v) for v in F(t - 30.0))
                hi = tuple(float(v) for v in F(t + 30.0))
                name = f"a_{'xyz'[axis]}{'+' if sign > 0 else '-'}{mag:.0e}"
                out.append(Probe(name, "a", xyz, 8, 1.0, cells=(0.05, 0.5), crop=(lo, hi)))
    return out


# ---- b. cell faces and block faces -----------------------------------------------------------------------------------
def _edges(X, cell, span):
    """{i: top of cell i}, {i: bottom of cell i} for the cells within span of X (every fp32 value in between tried)."""
    inv = F(1.0) / F(cell)
    lo, hi = F(max(X - span * cell, X / 2)), F(X + span * cell)
    bits = np.arange(lo.view(np.int32), hi.view(np.int32) + 1, dtype=np.int32)
    x = bits.view(np.float32)
    c = np.floor((x * inv).astype(np.float32)).astype(np.int64)
    ch = np.nonzero(np.diff(c))[0]
    return {int(c[i]): x[i] for i in ch}, {int(c[i + 1]): x[i + 1] for i in ch}


def _face_pairs(X, cell, span=40):
    """(d2, px, qx): p at the top of a cell near X, q at the bottom of the cell two further on — the closest point the
    first launch's 3x3x3 block around p leaves out — ordered by their fp32 d2, smallest first, at least 12 cells apart."""
    tops, bots = _edges(X, cell, span)
    cand = sorted((float(F(F(bots[i + 2] - tops[i]) * F(bots[i + 2] - tops[i]))), i) for i in tops if i + 2 in bots)
    out, used = [], []
    for d2, i in cand:
        if all(abs(i - u) >= 12 for u in used):
            used.append(i)
            out.append((F(d2), tops[i], bots[i + 2]))
    return out


def _frame_corners(center, half):
    """Two isolated points that give every axis of the probes' blocks a face on both sides."""
    c = np.asarray(center, np.float64)
    return [tuple(F(c - half)), tuple(F(c + half))]


def _r_at(p, target, lo_ok=False):
    off = offset_for(target, lo_ok)
    return None if off is None else (p[0], F(p[1] + off[0]), F(p[2] + off[1]))


def family_b():
    """Cell faces and block faces, searched ulp by ulp for explicit search cells at |x| from 1 to 1e6.
    block: p sits at the top of a cell and q at the bottom of the cell two further on — the closest point the 3x3x3 block
    around p leaves out — and p's nearest neighbour r lies inside the block at a d2 of exactly the first launch's exit bound,
    one ulp inside and one ulp outside it (first-launch exit against listed point).
    thin: at cell indices next to a power of two the cell assignment floor(fl(x * inv)) moves the upper face down more than
    the lower one, and q comes nearer than one cell: r sits at the largest d2 the exit bound would allow without its
    |coord| 2^-21 term. q, outside the block, is nearer than r; a first launch that stopped on such a bound reports r.
    ring: p at y = -1e-30 (the |coord| terms are nothing), q at the bottom of the row s - 1 cells up (ring s) and r in p's
    own row at the largest d2 a ring-break bound with kRel = 1 would allow: a ring break without kRel stops before ring s.
    face: pairs whose floor(x * inv_cell) lands on either side of a face, the nearest neighbour across it, k = 3 so every
    point is listed (x_range clipping of the second launch)."""
    out = []
    for X in (1.0, 1e2, 1e4, 1e6):
        for cell in (0.3, 0.7):
            rows = []
            pairs = _face_pairs(max(X, 40 * cell), cell, span=16)
            for (d2q, px, qx), kind in zip(pairs, ("at", "inside", "outside")):
                p = (px, F(0.0), F(0.0))
                T = exit_bound(p, cell)
                if not T > 0:
                    continue
                target = {"at": T, "inside": ulps(T, -1), "outside": ulps(T, 1)}[kind]
                r = _r_at(p, target)
                if r is not None:
                    rows += [p, (qx, F(0.0), F(0.0)), r]
            if rows:
                rows += _frame_corners((float(rows[0][0]), 0.0, 0.0), 60 * cell)
                out.append(Probe(f"b_block_X{X:.0e}_c{cell}", "b", pts(*rows), 1, 1.0, cells=(cell,)))
    for cell in (0.45, 0.9):
        inv = F(1.0) / F(cell)
        for m in (9, 13, 17):
            d2q, px, qx = _face_pairs(2.0 ** m / float(inv), cell, span=6)[0]
            p = (px, F(0.0), F(0.0))
            T_thin = exit_bound(p, cell, coord_term=False)
            if not d2q < T_thin:
                continue
            r = _r_at(p, T_thin, lo_ok=True)
            if r is None or not F(F(r[1] * r[1]) + F(r[2] * r[2])) > d2q:
                continue
            rows = [p, (qx, F(0.0), F(0.0)), r] + _frame_corners((float(px), 0.0, 0.0), 60 * cell)
            out.append(Probe(f"b_thin_2^{m}_c{cell}", "b", pts(*rows), 1, 1.0, cells=(cell,)))
    n_ring = 0
    for cell in (0.3, 0.7, 0.45):
        inv = F(1.0) / F(cell)
        cy = F(1.0) / inv
        found = 0
        for s in range(3, 60):
            qy = edge_of_cell(s - 1, inv, False)
            if qy is None:
                continue
            p = (F(0.0), F(-1e-30), F(0.0))
            d2q = F(F(qy - p[1]) * F(qy - p[1]))
            g1 = F(F(s - 1) * cy)
            T1 = F(g1 * g1)                                   # the ring-break bound with kRel = 1
            if not d2q < T1:
                continue
            off = offset_for(T1, lo_ok=True)
            if off is None or not F(F(off[0] * off[0]) + F(off[1] * off[1])) > d2q:
                continue
            r = (off[0], p[1], off[1])                       # in p's own row: along x, a little up in z
            rows = [p, (F(0.0), qy, F(0.0)), r]
            out.append(Probe(f"b_ring_c{cell}_s{s}", "b", pts(*rows), 1, 1.0, cells=(cell,)))
            found += 1
            if found == 2:
                break
        n_ring += found
    # faces: pairs straddling a face of the search grid, the true nearest neighbour across it, every point listed
    for X in (1.0, 1e3, 1e5):
        for cell in (0.3, 0.05):
            tops, bots = _edges(max(X, 60 * cell), cell, 30)
            rows = []
            for m, i in enumerate(sorted(tops)[::4][:6]):
                if i + 1 not in bots:
                    continue
                top, bot = tops[i], bots[i + 1]
                y0 = F(m * 3 * cell)
                # p at the top of cell i, its nearest neighbour at the bottom of cell i + 1, two more a little farther
                rows += [(top, y0, 0.0), (bot, y0, 0.0), (F(top - F(0.4 * cell)), y0, 0.0), (F(bot + F(0.45 * cell)), y0, 0.0)]
            rows += _frame_corners((float(rows[0][0]), 9 * cell, 0.0), 40 * cell)
            out.append(Probe(f"b_face_X{X:.0e}_c{cell}", "b", pts(*rows), 3, 1.0, cells=(cell,)))
    return out


# ---- c. degenerate grids ---------------------------------------------------------------------------------------------
def family_c():
    """Grids with one cell along two axes (a line along x, y or z: one of dx, dy, dz is 1... two are), a plane, everything in
    one cell, two clusters 1 km apart with only empty rows between them (ring break after many empty rows, row skip), and
    one isolated point whose neighbours are all more than 100 rings away (listed point searched ring by ring)."""
    rng = np.random.default_rng(3)
    out = []
    line = np.zeros((1500, 3), np.float32)
    line[:, 0] = np.sort(rng.uniform(0, 40, 1500)).astype(np.float32)
    for a in range(3):
        xyz = np.roll(line, a, axis=1)
        out.append(Probe(f"c_line_{'xyz'[a]}", "c", xyz, 8, 1.0, cells=(0.5,)))
    plane = rng.uniform(-10, 10, (3000, 3)).astype(np.float32)
    plane[:, 2] = F(-1.25)
    out.append(Probe("c_plane", "c", plane, 12, 1.0, cells=(0.3,)))
    one = (rng.uniform(0, 0.04, (2000, 3)) + 0.3).astype(np.float32)
    out.append(Probe("c_one_cell", "c", one, 16, 1.0, cells=(0.5, 5.0)))
    a = rng.normal(0, 0.5, (1500, 3))
    b = rng.normal(0, 0.5, (1500, 3)) + (0.0, 1000.0, 0.0)
    out.append(Probe("c_two_clusters", "c", np.concatenate([a, b]).astype(np.float32), 20, 1.0, cells=(0.2,)))
    c3 = rng.normal(0, 0.3, (1000, 3))
    iso = np.array([[0.0, 0.0, 60.0]])
    out.append(Probe("c_isolated", "c", np.concatenate([c3, iso]).astype(np.float32), 10, 1.0, cells=(0.1, 0.5)))
    return out


# ---- d. duplicates ---------------------------------------------------------------------------------------------------
def family_d():
    """Stacks of identical points: exactly k, k + 1, 2k and more than 64 copies (first-launch exit at d2 = 0 once a stack
    holds k others; a stack of exactly k copies has only k - 1 at 0 and must look beyond), +0.0 and -0.0 stacks (each
    survivor keeps its own sign bits), and in a crop box a stack larger than a tile of the bucket cell sort on the
    fixed-grid route (the frame may be handed back: PATH_REDONE is recorded, the bytes are the same either way)."""
    out = []
    rng = np.random.default_rng(4)
    bg = rng.uniform(-5, 5, (800, 3)).astype(np.float32)
    for k in (8, 16, 33):
        stacks = []
        for i, copies in enumerate((k, k + 1, 2 * k, 70)):
            stacks.append(np.repeat(pts((i * 2.0 + 0.5, 0.25, 0.125)), copies, axis=0))
        out.append(Probe(f"d_stacks_k{k}", "d", np.concatenate([bg] + stacks), k, 1.0, cells=(0.5,)))
    # (a -0.0 coordinate survives the identity pose only where every other term of its row is -0.0 too: the other
    # coordinates of these points are -0.0 or negative)
    zeros = np.concatenate([np.repeat(pts((0.0, 0.0, 0.0)), 5, 0), np.repeat(pts((-0.0, -0.0, -0.0)), 5, 0),
                            np.repeat(pts((-0.0, -0.5, -0.0)), 3, 0), np.repeat(pts((-0.25, -0.0, -0.0)), 4, 0), bg[:200]])
    out.append(Probe("d_signed_zeros", "d", zeros, 4, 0.0, cells=(0.5,), crop=((-6.0,) * 3, (6.0,) * 3)))
    big = np.concatenate([bg[:500], np.repeat(pts((1.0, 1.0, 1.0)), 4500, 0)])     # (a tile: CM_TILE = 4096 records)
    out.append(Probe("d_big_stack", "d", big, 5, 1.0, cells=(0.5,), crop=((-6.0,) * 3, (6.0,) * 3)))
    return out


# ---- e. subnormal ----------------------------------------------------------------------------------------------------
def family_e():
    """Points 2^-70 apart near the origin: d2 = 2^-140 is subnormal, so a flush to zero anywhere gives d_i = 0 (and every
    square lands in Q's bin 0: cm_sor_split's subnormal significand). Coordinates that are themselves subnormal. A frame
    whose d_i squares land in bin 0 while S stays normal. All in one cell of any search grid: first-launch exit through
    an axis covered whole (g = +inf)."""
    out = []
    t = F(2.0 ** -70)
    rng = np.random.default_rng(5)
    g = rng.integers(0, 8, (300, 3)).astype(np.float64) * float(t)
    out.append(Probe("e_lattice_2m70", "e", g.astype(np.float32), 4, 1.0, cells=(0.5,)))
    sub = (rng.integers(-2000, 2000, (300, 3)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    out.append(Probe("e_subnormal_coords", "e", sub, 3, 1.0, cells=(0.5,)))
    mix = np.concatenate([g[:100], rng.integers(0, 4, (50, 3)) * 2.0 ** -60 + 1e-3]).astype(np.float32)
    out.append(Probe("e_bin0_squares", "e", mix, 2, 0.5, cells=(0.5,)))
    return out


# ---- f. overflow -----------------------------------------------------------------------------------------------------
def family_f():
    """|dx| >= 2^64: d2 = +inf and d_i = +inf, so S = +inf and the variance NaN: nothing is removed. A finite d_i whose fp32
    square overflows (Q = +inf: stddev +inf, threshold +inf). A cloud whose bounds span more than FLT_MAX without a crop box:
    no finite search cell fits, the grid is one cell (inverse 0) and every point's block covers it whole (first-launch
    exit, g = +inf). The same cloud inside a crop box of +-2e38: that box fits no cell either, and the search grid is the
    cloud's own bounds."""
    out = []
    rng = np.random.default_rng(6)
    cl = rng.normal(0, 1, (200, 3))
    far = np.array([[3e19, 0.0, 0.0], [-3e19, 0.0, 0.0]])
    # (voxels of 1e19 m: the voxel grid behind the stage fits these two; the wider clouds report CM_GRID_OVERFLOW)
    out.append(Probe("f_inf_d2", "f", np.concatenate([cl, far]).astype(np.float32), 2, 1.0, cells=(0.5,), leaf=1e19))
    sq = np.array([[0.0, 0.0, 0.0], [2e19, 0.0, 0.0], [4e19, 0.0, 0.0]])
    out.append(Probe("f_square_overflows", "f", np.concatenate([cl, sq]).astype(np.float32), 1, 1.0, cells=(0.5,),
                     leaf=1e19))
    wide = np.concatenate([cl, [[3e38, 0.0, 0.0], [-3e38, 1.0, 0.0], [0.0, 3.4e38, -3.4e38]]]).astype(np.float32)
    out.append(Probe("f_span_over_flt_max", "f", wide, 3, 1.0, cells=(0.5,)))
    out.append(Probe("f_crop_2e38", "f", wide, 3, 1.0, cells=(0.5,), crop=((-2e38,) * 3, (2e38,) * 3)))
    out.append(Probe("f_crop_flt_max", "f", cl.astype(np.float32), 4, 1.0, cells=(0.5,),
                     crop=((-3.4e38, -5.0, -5.0), (3.4e38, 5.0, 5.0))))
    return out


# ---- g. KMAX boundaries ----------------------------------------------------------------------------------------------
def family_g():
    """k = 15, 16, 17, 31, 32, 33, 63, 64 around the three instantiations of k_sor_knn<KMAX> (16 / 32 / 64 floats per lane),
    and frames of n = k + 1 (every point's k-th neighbour is the farthest point of the cloud: listed, ring search to the
    end of the grid) and n = k (the degenerate frame: d_i NaN, threshold +inf, nothing removed)."""
    out = []
    rng = np.random.default_rng(7)
    base = np.concatenate([rng.normal(0, 1.0, (2500, 3)), rng.uniform(-30, 30, (40, 3))]).astype(np.float32)
    for k in (15, 16, 17, 31, 32, 33, 63, 64):
        out.append(Probe(f"g_k{k}", "g", base, k, 1.0, cells=(0.3,)))
    for k in (1, 16, 17, 32, 64):
        few = rng.uniform(-3, 3, (k + 1, 3)).astype(np.float32)
        out.append(Probe(f"g_n_k1_k{k}", "g", few, k, 1.0, cells=(0.5,)))
        out.append(Probe(f"g_n_k_k{k}", "g", few[:k], k, 1.0, cells=(0.5,),
                         expect_d=np.full(k, np.nan, np.float32), expect_removed=0))
    return out


# ---- h. threshold edges ----------------------------------------------------------------------------------------------
def family_h():
    """std_mul = 0 with every d_i equal (points 1 m apart on a line, k = 1: d_i = 1, S = n, Q = n, var = 0, threshold =
    mean = 1 exactly, and the strict > removes nothing); a frame whose threshold equals one d_i exactly (pairs 1, 2 and 3 m
    apart, k = 1, std_mul = 0: mean = 2, the 3 m pairs go, the 2 m pairs stay); a negative and a large std_mul."""
    out = []
    line = np.zeros((200, 3), np.float32)
    line[:, 0] = np.arange(200, dtype=np.float32)
    out.append(Probe("h_all_equal", "h", line, 1, 0.0, cells=(0.5,), expect_d=np.ones(200, np.float32), expect_removed=0))
    rows, want = [], []
    for i, gap in enumerate((1.0, 2.0, 3.0) * 4):
        rows += [(0.0, i * 100.0, 0.0), (gap, i * 100.0, 0.0)]
        want += [gap, gap]
    out.append(Probe("h_threshold_is_a_d", "h", pts(*rows), 1, 0.0, cells=(0.5,), expect_d=np.float32(want), expect_removed=8))
    rng = np.random.default_rng(8)
    cl = np.concatenate([rng.normal(0, 1, (1500, 3)), rng.uniform(-20, 20, (30, 3))]).astype(np.float32)
    for sm in (-0.75, -3.0, 50.0, 1e30):
        out.append(Probe(f"h_std_mul_{sm:g}", "h", cl, 6, sm, cells=(0.5,)))
    return out


def probes(families="abcdefgh"):
    out = []
    for f in families:
        out += globals()["family_" + f]()
    return out


# ---- i. the automatic cell after extreme frames -----------------------------------------------------------------------
def extreme_frames():
    """Frames whose mean distance is +inf, NaN, 2^-70 or 1e6: the next frame's automatic cell must come out usable."""
    rng = np.random.default_rng(9)
    cl = rng.normal(0, 1, (200, 3))
    g = rng.integers(0, 8, (200, 3)) * 2.0 ** -70
    spread = rng.normal(0, 1, (200, 3)) * 1e6
    return {
        "inf": np.concatenate([cl, [[3e19, 0, 0], [-3e19, 0, 0]]]).astype(np.float32),
        "nan": rng.uniform(-1, 1, (4, 3)).astype(np.float32),            # n <= k: the mean is NaN
        "2^-70": g.astype(np.float32),
        "1e6": spread.astype(np.float32),
    }
