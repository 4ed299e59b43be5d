"""Windows of the occupancy map far from the world origin: the placements, the scenes built on them and their CPU guards
(tests/test_map_far_windows.py drives the library over them).

A placement is the absolute cell of window cell (0, 0). Every scene is built backwards: window cells are chosen, fp32
coordinates are taken at their centres, and the restatement's own cell computation (tests/traj_ref.py: cells_of, the header's
floorf(w * inv) strictly inside +-2^30, minus the anchor) says which cell each coordinate really lands in. Far from the
origin that is not the chosen cell: at 2^24 cells fp32 resolves 1.25 cells of 0.1 m, at 2^30 cells it resolves 8 m, and
the product w * inv is rounded to a multiple of 64 there. The guards at the end of each builder are asserted on those answers
alone, on the CPU."""
import math

import numpy as np

from tests import cast_ref as kr
from tests import cost_ref as cr
from tests import map_ref as mpr
from tests import match_ref as mf
from tests import match_search_ref as ms
from tests import mcl_ref as mr
from tests import plan_ref as pr
from tests import test_grid_rays as tr
from tests import test_map_match as tmm
from tests import test_map_match_search as tms
from tests import test_map_mcl as tml
from tests import test_map_mcl_hyp as tmh
from tests import test_occupancy_map as tm
from tests import traj_ref as jr

F32 = np.float32
CELL = 0.1
LIMIT = 1 << 30
COST_Q = cr.params(0.0, 0.3, 3.0)                    # the localisation tests' cost layer: graded out to three cells, no 253
PLAN_Q = pr.params(50, 205, 0)


class Place:
    """A window of nx x ny cells of edge `cell` whose cell (0, 0) is the absolute cell `anchor`."""

    def __init__(self, name, nx, ny, anchor, cell=CELL):
        self.name, self.nx, self.ny, self.anchor, self.cell = name, nx, ny, (int(anchor[0]), int(anchor[1])), cell
        self.mq = mpr.params(cell, nx, ny)
        self.wide = nx > 96

    def __repr__(self):
        return self.name

    def centre(self, ix, iy):
        """The fp32 coordinates nearest the centre of window cell (ix, iy), as Python floats."""
        return float(F32((self.anchor[0] + ix + 0.5) * self.cell)), float(F32((self.anchor[1] + iy + 0.5) * self.cell))

    def cells(self, x, y):
        """(on the window, ix, iy) of fp32 coordinates by the restatement."""
        return jr.cells_of(np.atleast_1d(np.asarray(x, F32)), np.atleast_1d(np.asarray(y, F32)), self.cell, self.anchor, self.nx, self.ny)

    def exists(self, x, y):
        """Whether the absolute cell of fp32 coordinates exists (both axes strictly inside +-2^30)."""
        inv = F32(1.0) / F32(self.cell)
        with np.errstate(over="ignore", invalid="ignore"):
            cx, cy = np.floor(np.atleast_1d(np.asarray(x, F32)) * inv), np.floor(np.atleast_1d(np.asarray(y, F32)) * inv)
        return (np.abs(cx) < F32(LIMIT)) & (np.abs(cy) < F32(LIMIT))

    def landing(self, ix, iy):
        """The window cell the centre coordinates of (ix, iy) really land in, or None."""
        on, jx, jy = self.cells(*self.centre(ix, iy))
        return (int(jx[0]), int(jy[0])) if on[0] else None

    def land(self, ix, iy):
        """((x, y), cell) for a chosen window cell whose coordinates must land on the window."""
        cell = self.landing(ix, iy)
        assert cell is not None, (self.name, ix, iy)
        return self.centre(ix, iy), cell


ORIGIN = Place("origin", 96, 80, tmm.anchor_of(96, 80))
KM = Place("km", 96, 80, (120_000 - 48, -70_000 - 40))
TWO24 = Place("two24", 96, 80, ((1 << 24) - 48, -(1 << 24) - 40))
LIMIT_POS = Place("limit_pos", 2048, 64, (LIMIT - 1024, LIMIT - 1 - 64))
LOADED = [ORIGIN, KM, TWO24, LIMIT_POS]              # what cm_map_load accepts; limit_neg is reachable through cm_map_integrate only


def _named(a, n, cell=CELL):
    """{window index: an fp32 coordinate that lands in it}, over every fp32 value from before the window's first cell to
    beyond its last: what fp32 can name on one axis of a window at the limit."""
    inv, out = F32(1.0) / F32(cell), {}
    v, end = F32((a - 200) * cell), F32((a + n + 200) * cell)
    while v <= end:
        c = np.floor(v * inv)
        if abs(c) < F32(LIMIT) and 0 <= int(c) - a < n:
            out.setdefault(int(c) - a, float(v))
        v = np.nextafter(v, F32(np.inf))
    return out


WIDE_X, WIDE_Y = _named(LIMIT_POS.anchor[0], 2048), _named(LIMIT_POS.anchor[1], 64)
WIDE_COLS = sorted(WIDE_X)                           # fp32 values lie 8 m apart there and w * inv is rounded to a multiple of 64:
(WIDE_ROW,) = WIDE_Y                                 # thirteen columns, all multiples of 64 below 1024, and the one row 2^30 - 64
WIDE_OCC = [2, 5, 9]                                 # the named columns (by rank) that hold an obstacle


def wide_at(rank):
    """((x, y), window cell) of the named column of that rank at limit_pos."""
    return (WIDE_X[WIDE_COLS[rank]], WIDE_Y[WIDE_ROW]), (WIDE_COLS[rank], WIDE_ROW)


# ---- the images -----------------------------------------------------------------------------------------------------------------
def room_image(sym=False):
    """tests/test_map_mcl.py's room (or the symmetric room), free inside, with a doorway of two cells in the right wall and a
    free corridor from it to the window's edge: free cells beside unknown ones (frontiers) and a way off the window."""
    img = tmh.image_with_free_interior(tmh.SYM if sym else tml.ROOM)
    img[40:42, 91:96] = 0
    return img


def wide_image():
    """2048 x 64: a free band of ten rows over the columns that exist, unknown elsewhere; obstacles in the one reachable row."""
    img = np.full((64, 2048), -1, np.int8)
    img[0:10, 0:1100] = 0
    for k in WIDE_OCC:
        img[WIDE_ROW, WIDE_COLS[k]] = 100
    img[8, 100:1000:7] = 100                         # a broken wall: structure for the cost, plan and frontier layers
    return img


def image_of(place, sym=False):
    return wide_image() if place.wide else room_image(sym)


def tables_of(place, sym=False):
    """(image, cost, dist2) by the cost layer's restatement."""
    image = image_of(place, sym)
    cost, dist2, _ = cr.cost_separable(image, place.cell, COST_Q)
    return image, cost, dist2


# ---- plan ----------------------------------------------------------------------------------------------------------------------
def plan_scene(place):
    """Goal and starts as ((x, y), cell): fp32 world points and the window cell the restatement names for them."""
    if place.wide:
        return wide_at(3), [wide_at(7), wide_at(11), wide_at(3)]
    return place.land(20, 60), [place.land(80, 10), place.land(50, 45), place.land(93, 40)]


def plan_restated(place, cost):
    (gxy, goal), starts = plan_scene(place)
    q = dict(PLAN_Q, max_path_cells=place.nx * place.ny)
    pot = pr.potential_dijkstra(cost, q, goal)
    walks = [pr.walk(pot, cost, q, goal, start, q["max_path_cells"]) for _, start in starts]
    assert any(status == pr.FOUND and len(cells) > 10 for cells, status, _ in walks), (place.name, [(len(c), s) for c, s, _ in walks])
    return q, gxy, goal, starts, pot, walks


# ---- rollout -------------------------------------------------------------------------------------------------------------------
def traj_scene(place):
    """Samples that cross the window's edge (through the doorway's corridor) and, at limit_pos, the edge of existence."""
    if place.wide:
        (x, y), _ = wide_at(11)
        return jr.params(4, 5, 6, 1, 1, jr.ALLOW_UNKNOWN), np.array([[8.0, 0.0], [-8.0, 0.0]], F32), jr.window(x, y, 0.0, (0.0, 240.0), (-1.0, 1.0), 0.1)
    (x, y), _ = place.land(89, 40)
    return jr.params(4, 5, 12, 1, 1, jr.ALLOW_UNKNOWN), np.array([[0.1, 0.0], [-0.1, 0.05]], F32), jr.window(x, y, 0.0, (0.0, 3.0), (-2.0, 2.0), 0.1)


def traj_restated(place, cost, pot, tab):
    tq, foot, win = traj_scene(place)
    assert jr.refusal(tq, foot) is None and jr.refusal(tq, foot, win, place.cell, place.anchor, place.nx, place.ny) is None, place.name
    want, winfo = jr.rollout(cost, pot, place.anchor, place.cell, tq, foot, win, tab)
    st = want["status"]
    assert (st == jr.OFF_MAP).any() and (st != jr.OFF_MAP).any(), (place.name, np.bincount(st, minlength=4).tolist())
    if place.wide:                                   # a sample left existence, not only the window
        off = want[st == jr.OFF_MAP]
        assert (~place.exists(off["end_x"], off["end_y"])).any(), place.name
    return tq, foot, win, want, winfo


# ---- matching ------------------------------------------------------------------------------------------------------------------
def match_scene(place):
    """The walls as the vehicle sees them from the window's centre, matched under a prior that is turned by 48 entries (4.2
    degrees) and stands two cells beside the truth; tests/test_map_match.py's scene dictionary, so that its evaluate runs it."""
    if place.wide:                                   # body points every 6.4 m along x: fp32 tells nothing finer apart out there
        scan = [[(1024 + 64 * k, 32) for k in range(-8, 9, 2)], [(1024 + 64 * k, 32) for k in range(-7, 9, 2)]]
        (x, y), _ = wide_at(6)
        q = dict(n_a=1, a_stride=16, wx=3, wy=2, sigma=0.1, max_dist=0.3)
    else:
        walls = tml.ROOM
        scan = [walls[0::2], walls[1::2]]
        x, y = float(F32((place.anchor[0] + 48 + 2) * place.cell)), float(F32((place.anchor[1] + 40 - 1) * place.cell))
        q = dict(n_a=3, a_stride=16, wx=4, wy=3, sigma=0.1, max_dist=0.3)
    return tmm.scene(f"far {place.name}", [[], []], scan_cells=scan, nx=place.nx, ny=place.ny, q=q, prior=(x, y), turn=48)


def match_guard(vol, n_cells):
    assert n_cells > 0 and vol.max() > 0 and vol.min() < vol.max(), (n_cells, int(vol.max()), int(vol.min()))


def match_restated(place, dist2, tab):
    sc = match_scene(place)
    _, A = tmm.scan_of(sc)
    prior = tmm.prior_of(sc, tab)
    assert prior[0, 1] != 0                          # a real rotation
    vol, res = mf.match(A, dist2, sc["mq"], place.anchor, sc["q"], prior, tab)
    match_guard(vol, res["n_cells"])
    status, sres, info, LQD = ms.match(A, dist2, sc["mq"], place.anchor, tms.search_q(sc), prior, tab)
    tms.check_scene(sc, status, sres, info, LQD)
    assert sres["score"] == res["score"] > 0
    return sc


# ---- casting -------------------------------------------------------------------------------------------------------------------
def last_existing(place):
    """The largest fp32 x whose cell exists and the next fp32 value, whose cell does not (limit_pos)."""
    (x, y), _ = wide_at(-1)
    x = F32(x)
    while place.exists(np.nextafter(x, F32(np.inf)), y)[0]:
        x = np.nextafter(x, F32(np.inf))
    return float(x), float(np.nextafter(x, F32(np.inf))), y


def cast_poses(place):
    rng = np.random.default_rng(17)
    if place.wide:
        rows = [wide_at(r)[0] + (int(h),) for r, h in zip(range(len(WIDE_COLS)), rng.integers(0, 1 << 32, len(WIDE_COLS)))]
        last, past, y = last_existing(place)
        rows += [(last, y, 0), (last, y, 1 << 31), (past, y, 0), (past, y, 1 << 31), place.centre(1400, WIDE_ROW) + (0,)]
        rows += [wide_at(r)[0] + (h,) for r in (1, 3, 4, 6) for h in (0, 1 << 31)]      # along the row, towards the obstacles
        return kr.poses_of(rows)
    cells = [(10, 10), (48, 40), (60, 33), (89, 40), (95, 41), (0, 0), (95, 79), (30, 70), (-2, 40), (97, 40), (40, -3), (40, 82)]
    cells += list(zip(rng.integers(5, 91, 40).tolist(), rng.integers(5, 75, 40).tolist()))
    return kr.poses_of([place.centre(ix, iy) + (int(h),) for (ix, iy), h in zip(cells, rng.integers(0, 1 << 32, len(cells)))])


def cast_q(poses):
    return dict(max_poses=len(poses), n_bearings=64, range_cells=200, flags=0)


def cast_guard(place, poses, rays):
    st = rays["status"]
    on, ix, _ = place.cells(poses["x"], poses["y"])
    assert (st == kr.S_HIT).any() and (st == kr.S_NO_ORIGIN).any() and on.any() and (st[on] != kr.S_NO_ORIGIN).all(), place.name
    if place.wide:
        assert len(set(ix[on].tolist())) >= 8 and (~place.exists(poses["x"], poses["y"])).any(), place.name
        last, past, y = last_existing(place)
        assert place.cells(last, y)[0][0] and not place.exists(past, y)[0]


def cast_restated(place, image, tab):
    poses = cast_poses(place)
    rays, info = kr.cast(image, place.cell, place.anchor, cast_q(poses), None, poses, tab)
    cast_guard(place, poses, rays)
    return poses, rays


# ---- localisation --------------------------------------------------------------------------------------------------------------
def mcl_scene(place):
    """(body points of the frame, filter parameters, (x, y, yaw, sd_x, sd_y, sd_yaw) of init_pose)."""
    if place.wide:
        pts = tml.body_points([(64 * k, 0) for k in range(-8, 9)] + [(64 * k + 1, 1) for k in range(-3, 4)])
        (x, y), _ = wide_at(10)
        return pts, tml.q_of(n_particles=256, max_beams=64, range_cells=600, seed=5), (x, y, 0.0, 30.0, 4.0, 0.5)
    dx, dy = (place.anchor[0] - ORIGIN.anchor[0]) * place.cell, (place.anchor[1] - ORIGIN.anchor[1]) * place.cell
    x, y = float(F32(tml.TRUTH0[0] + 0.1 + dx)), float(F32(tml.TRUTH0[1] + dy))
    return tml.body_points(tml.scan_of(tml.TRUTH0)), tml.q_of(n_particles=256, max_beams=256, seed=5), (x, y, tml.TRUTH0[2], 0.3, 0.3, 0.1)


PREDICT = (0.1, 0.0, 0.05, 0.03, 0.03, 0.02)


def mcl_guard(place, parts, table, info):
    """On the particles an update found and its weight table: beams, a score, and both kinds of origin cell where there are both."""
    n_beams = info["n_beams"] if isinstance(info, dict) else info.n_beams
    assert n_beams > 0 and (table["score"] > 0).any(), (place.name, n_beams)
    if place.wide:
        e = place.exists(parts["x"], parts["y"])
        assert e.any() and (~e).any(), (place.name, int(e.sum()))


def frame_cloud(points):
    """The cloud A a frame of the body points makes (tests/test_map_mcl.py: frame)."""
    return tmm.clouds_of(tml.split(points))[1]


def mcl_drive(place, f, update, rounds=2):
    """init_pose, predict and `rounds` updates with a predict after each on a Filter-like f; update() returns (table, info, ...)
    as a restatement's Filter does. The guard after every update, on the particles it found."""
    f.init_pose(*mcl_scene(place)[2])
    f.predict(*PREDICT)
    for _ in range(rounds):
        found = f.parts.copy()
        out = update()
        mcl_guard(place, found, out[0], out[1])
        f.predict(*PREDICT)


def uniform_rounds(place, image):
    """How many free cells' (float)(anchor + i) is not anchor + i on either axis: init_uniform's rounding."""
    iy, ix = np.nonzero(image == 0)
    ax, ay = (place.anchor[0] + ix), (place.anchor[1] + iy)
    return int(((ax.astype(F32).astype(np.int64) != ax) | (ay.astype(F32).astype(np.int64) != ay)).sum())


HYP_Q = dict(bin_q=64, heading_bits=8, max_hyp=64, inject_max=255, alpha_slow=0.05, alpha_fast=0.5)
HYP_MCL = dict(n_particles=1024, max_beams=256, seed=31)


def hyp_frames():
    """The symmetric room's scan, then one that fits the room badly: the average score drops and the recovery injects."""
    return [tml.body_points(tmh.scan_of(tmh.SYM, tmh.SYM_TRUTH0)),
            tml.body_points([(x, 30) for x in range(-30, 31, 2)] + [(33, y) for y in range(-30, 30, 3)])]


def hyp_guard(place, first, second, bins, n_injected):
    """first, second: the hyp infos of the two updates (dictionaries); bins: the (by, bx) of the particles the first update found."""
    assert second["n_inject"] == n_injected > 0 and first["n_inject"] == 0, (place.name, second)
    if place is TWO24:                               # every position on the clamp q = +-2^30: bins +-2^24, the bin bound
        assert bins == {(-(1 << 24), 1 << 24)} and first["n_bins"] <= 256, (place.name, first["n_bins"])
    else:
        assert first["n_bins"] > 900, (place.name, first["n_bins"])


# ---- integration far away ---------------------------------------------------------------------------------------------------------
Q64 = tm.Q64
Q512 = mpr.params(0.5, 512, 512)
X_NEG = -536870848.0                                 # cell -2^30 + 128 at 0.5 m: the window of 512 starts 128 cells below -2^30


def far_sequences():
    """name -> (parameters, frames as per-sensor parts, poses, whether map_ref's guards can hold)."""
    two23 = float(1 << 23)
    return {
        "km": (Q64, tm.frames_of(46, 3), [tm.pose_t(12000.3, -7000.2), tm.pose_t(12000.77, -7000.41), tm.pose_t(12001.93, -6999.74)], True),
        "two24": (Q64, tm.frames_of(49, 3), [tm.pose_t(two23, -two23), tm.pose_t(two23 + 5.0, -two23 - 3.0), tm.pose_t(two23 - 3.5, -two23 - 7.0)], True),
        "limit_neg": (Q512, [tr.scene(52 + k, 3, 1500, (-100.0, 100.0)) for k in range(3)],
                      [tm.pose_t(X_NEG, 0.3), tm.pose_t(X_NEG - 32.0, 20.7), tm.pose_t(X_NEG + 32.0, 41.9)], False),
    }


def point_cells_exist(A, P, cell):
    """Per point of A whether its absolute cell under the pose exists: map_ref's step 1, the existence alone."""
    A, P = np.asarray(A, F32).reshape(-1, 4), np.asarray(P, F32).reshape(3, 4)
    inv = F32(1.0) / F32(cell)
    x, y, z = A[:, 0], A[:, 1], A[:, 2]
    wx = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
    wy = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
    return (np.abs(np.floor(wx * inv)) < F32(LIMIT)) & (np.abs(np.floor(wy * inv)) < F32(LIMIT))


def sequence_guards(name, history, clouds, poses):
    """history: map_ref's (table, image, info) per frame; clouds: the A of every frame."""
    q = history[0][2]
    anchors = [i["anchor"] for _, _, i in history]
    assert len(set(anchors)) == len(anchors), (name, anchors)                      # every frame scrolls
    for k, (_, image, i) in enumerate(history):
        assert i["n_rays"] > 0 and (image == 100).any() and i["sensors_cast"], (name, k)
        assert k == 0 or i["carried"] > 0, (name, k)
    if name == "km":
        assert anchors[0] == (24000 - 32, -14001 - 32)
    if name == "two24":
        assert anchors[0] == ((1 << 24) - 32, -(1 << 24) - 32)
    if name == "limit_neg":
        assert all(a[0] < -LIMIT and a[0] + q["nx"] > -LIMIT for a in anchors), anchors        # the window straddles -2^30
        for A, P in zip(clouds, poses):
            e = point_cells_exist(A, P, 0.5)
            assert e.any() and (~e).any(), (name, int(e.sum()), len(e))


# ---- the exact shift -------------------------------------------------------------------------------------------------------------
B_CELL = 0.125                                       # dyadic: inv is exactly 8
B_NX, B_NY = 96, 80
B_MQ = mpr.params(B_CELL, B_NX, B_NY)
B_SHIFT_CELLS = 65536
B_SHIFT = (B_SHIFT_CELLS * B_CELL, -B_SHIFT_CELLS * B_CELL)             # (+8192 m, -8192 m)
B_TRANS = [(1.5, 0.25, 1.0), (-1.25, -0.5, 1.0)]
B_POSES = [(0.25, -0.125), (1.5, 0.75), (2.75, -1.0)]                    # scrolls of ten and seven cells
B_LATTICE = 1.0 / 128.0


def b_frames():
    """Three frames of two sensors: vehicle-frame points on multiples of 2^-7 m within 7 m, as (sensor-frame parts, A)."""
    out = []
    for k in range(3):
        rng = np.random.default_rng(300 + k)
        parts, A = [], []
        for s, t in enumerate(B_TRANS):
            p = np.concatenate([rng.integers(-896, 897, (500, 2)), rng.integers(0, 65, (500, 1))], axis=1) * B_LATTICE
            ring = np.array([[6.0 * math.cos(a), 4.5 * math.sin(a), 0.25] for a in np.linspace(0, 2 * math.pi, 90, endpoint=False)])
            p = np.concatenate([p, np.round(ring / B_LATTICE) * B_LATTICE])
            q = (p - np.asarray(t)).astype(F32)
            assert (q.astype(np.float64) == p - np.asarray(t)).all()
            parts.append(np.concatenate([q, np.full((len(q), 1), s, F32)], axis=1))
            A.append((q + F32(t)[None, :]).astype(F32))
        out.append((parts, np.concatenate(A)))
    return out


def exact_under_shift(values, shift):
    """float32(v + shift) - shift == v for every value, in double."""
    v = np.asarray(values, np.float64).reshape(-1)
    assert (v == v.astype(F32)).all()
    return bool(((v + shift).astype(F32).astype(np.float64) - shift == v).all())
