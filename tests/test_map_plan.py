"""The plan layer behind the cost layer: cm_map_plan_configure, cm_map_plan_update, cm_map_plan_copy, cm_map_plan_device,
cm_map_plan_path (include/cloudmerge.h, cm_kernels_plan.hip).

The bar on the GPU: every byte of pot, of every path, of all infos (but n_sweeps, which is not a function of the input) and of
the device-pointer variant equal to the restatement (tests/plan_ref.py) fed with the library's own cost table (map_cost()).
There is no tolerance: step costs are positive integers and the shortest-path potential is unique. The images are designed as
in tests/test_map_cost.py: one point of A per wanted obstacle cell; a sensor outside the window gives an image of 100 and -1
only, on which CM_COST_INFLATE_UNKNOWN together with CM_PLAN_ALLOW_UNKNOWN gives a graded, traversable field; a sensor inside
adds free cells. plan_ref.guards are asserted on the restatement's output before the device's bytes are looked at."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cloud_merger_amd import capi
from tests import cost_ref as cr
from tests import plan_ref as pr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_map_cost as tc
from tests import test_occupancy_map as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
NAMES = ("cm_map_plan_configure", "cm_map_plan_update", "cm_map_plan_copy", "cm_map_plan_device", "cm_map_plan_path")
PLAN_TYPES = (capi.PlanParams, capi.PlanInfo, capi.PathInfo)     # (a library without the plan layer fails every test here, at import)
TILE = tr.device_define("CM_PLAN_TILE")            # the edge of one k_plan_sweep tile in cells
Q = pr.params()                                    # navfn's 50 and 0.8
BOTH = (0, pr.ALLOW_UNKNOWN)


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_plan_structs_and_constants_match_header(tmp_path):
    structs = {"cm_plan_params": (capi.PlanParams, ["neutral", "cost_factor_q8", "flags", "max_path_cells"]),
               "cm_plan_info": (capi.PlanInfo, ["goal", "n_sweeps"]),
               "cm_path_info": (capi.PathInfo, ["start", "goal", "n_cells", "status", "pot_start"])}
    names = ["CM_PLAN_UNREACHABLE", "CM_PLAN_ALLOW_UNKNOWN", "CM_PATH_FOUND", "CM_PATH_UNREACHABLE", "CM_PATH_TRUNCATED"]
    items, want = [], []
    for s, (T, fields) in structs.items():
        items += [f"sizeof({s})"] + [f"offsetof({s},{f})" for f in fields]
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%llu ",(unsigned long long)({it}));' for it in items + names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(want)] == want == [16, 0, 4, 8, 12, 16, 0, 8, 32, 0, 8, 16, 20, 24]
    assert got[len(want):] == [capi.PLAN_UNREACHABLE, capi.PLAN_ALLOW_UNKNOWN, capi.PATH_FOUND, capi.PATH_UNREACHABLE, capi.PATH_TRUNCATED]
    assert got[len(want):] == [pr.UNREACHABLE, pr.ALLOW_UNKNOWN, pr.FOUND, pr.PATH_UNREACHABLE, pr.TRUNCATED] == [0xFFFFFFFF, 1, 0, 1, 2]
    assert TILE == 32 and tr.device_define("CM_PLAN_BLOCK") == TILE * TILE
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.PlanParams(50, 205, 0, 16)
    info, minfo, pinfo = capi.PlanInfo(), capi.MapInfo(), capi.PathInfo()
    before = bytes(info), bytes(minfo), bytes(pinfo)
    buf = np.full(16, 7, np.uint32)
    a = C.c_void_p(5)
    assert L.cm_map_plan_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_plan_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_plan_update(None, 0.0, 0.0, C.byref(info), C.byref(minfo)) == capi.BAD_ARG
    assert L.cm_map_plan_copy(None, buf.ctypes.data, 16, C.byref(info), C.byref(minfo)) == capi.BAD_ARG
    assert L.cm_map_plan_device(None, C.byref(a), C.byref(info), C.byref(minfo)) == capi.BAD_ARG
    assert L.cm_map_plan_path(None, 0.0, 0.0, buf.ctypes.data, 16, C.byref(pinfo)) == capi.BAD_ARG
    assert (buf == 7).all() and (bytes(info), bytes(minfo), bytes(pinfo)) == before and a.value == 5


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def random_cost(seed, ny, nx):
    """Uniform in 0..252, 20 % lethal (254), 5 % unknown (255)."""
    rng = np.random.default_rng(seed)
    cost = rng.integers(0, 253, (ny, nx)).astype(np.uint8)
    r = rng.random((ny, nx))
    cost[r < 0.20] = 254
    cost[r >= 0.95] = 255
    return cost


def goal_of(cost, want_lethal=False):
    """The cell nearest (nx / 3, ny / 2), scanning along x then y, that is (or is not) lethal."""
    ny, nx = cost.shape
    cells = sorted(((x - nx // 3) ** 2 + (y - ny // 2) ** 2, x, y) for y in range(ny) for x in range(nx))
    return next((x, y) for _, x, y in cells if (cost[y, x] == 254) == want_lethal)


RANDOM_SHAPES = ((1, 1), (1, 70), (70, 1), (33, 65), (67, 129), (257, 255))                       # (ny, nx)


@pytest.fixture(scope="module")
def random_cases():
    """(cost, goal, q, pot) per shape and flag setting, by the relaxation; the 33 x 65 image has its goal in a lethal cell."""
    out = []
    for k, (ny, nx) in enumerate(RANDOM_SHAPES):
        cost = random_cost(100 + k, ny, nx)
        if (ny, nx) == (1, 1):
            cost[:] = 7
        goal = goal_of(cost, want_lethal=(ny, nx) == (33, 65))
        for f in BOTH:
            q = pr.params(flags=f, max_path_cells=nx * ny)
            out.append((cost, goal, q, pr.potential_relaxed(cost, q, goal)))
    return out


def test_the_two_restatements_agree(random_cases):
    lethal_goals = 0
    for cost, goal, q, pot in random_cases:
        ny, nx = cost.shape
        if min(nx, ny) >= 33:                          # the vacuity guard first, on the restatement alone
            pr.guards(pot, cost, q, goal, ("mostly_reachable", "some_unreachable", "graded"))
        lethal_goals += int(cost[goal[1], goal[0]] == 254)
        other = pr.potential_dijkstra(cost, q, goal)
        assert pot.dtype == other.dtype == np.uint32 and pot.shape == other.shape == (ny, nx) and pot.tobytes() == other.tobytes()
    assert lethal_goals == 2


def test_an_empty_image_has_the_closed_form():
    for ny, nx, goal in ((1, 1, (0, 0)), (40, 70, (23, 20)), (65, 33, (0, 64)), (9, 9, (8, 0))):
        for neutral in (1, 50, 255):
            q = pr.params(neutral=neutral, max_path_cells=nx * ny)
            want = pr.closed_form(nx, ny, goal, neutral)
            cost = np.zeros((ny, nx), np.uint8)
            assert pr.potential_relaxed(cost, q, goal).tobytes() == want.tobytes() == pr.potential_dijkstra(cost, q, goal).tobytes()


def test_known_weights():
    cost = np.array([[0, 100, 252, 253, 254, 255]], np.uint8)
    assert pr.weights(cost, Q).tolist() == [[50, 130, 251, 0, 0, 0]]                      # 50 + (20500 >> 8), 50 + (51660 >> 8)
    assert pr.weights(cost, dict(Q, flags=1)).tolist() == [[50, 130, 251, 0, 0, 251]]
    assert pr.weights(cost, pr.params(1, 0)).tolist() == [[1, 1, 1, 0, 0, 0]] and pr.weights(cost, pr.params(255, 256)).tolist()[0][:3] == [255, 355, 507]
    assert pr.w_max(Q) == 251 and pr.w_max(pr.params(255, 256)) == 507


# y |  x ->   neutral 1, factor 0: every passable cell weighs 1, a straight step 5, a diagonal one 7. The goal is (0, 3). The
#             lethal cells (1, 1) and (2, 2) touch at a corner: the step between (1, 2) and (2, 1) would pass between them and
#             does not exist (with it, pot(2, 1) were 7 + 7 = 14), and no diagonal step passes either of them: (2, 1) is reached
#             around the far side. Ties: (2, 1) over (3, 1) [direction 0] and (2, 0) [6]; (4, 1) over (4, 2) [2] and (3, 2) [3];
#             (3, 0) over (3, 1) [2] and (2, 0) [4]; (4, 0) over (4, 1) [2] and (3, 1) [3].
HAND_COST = [[0, 0, 0, 0, 0],
             [0, 254, 0, 0, 0],
             [0, 0, 254, 0, 0],
             [0, 0, 0, 0, 0]]
U = pr.UNREACHABLE
HAND_POT = [[15, 20, 25, 30, 32],
            [10, U, 30, 25, 27],
            [5, 7, U, 20, 22],
            [0, 5, 10, 15, 20]]
HAND_GOAL = (0, 3)
HAND_PATHS = {(2, 1): [7, 8, 13, 18, 17, 16, 15], (4, 1): [9, 14, 18, 17, 16, 15], (0, 3): [15], (1, 2): [11, 15]}
HAND_TIES = {(2, 1): [0, 6], (4, 1): [2, 3], (3, 0): [2, 4], (4, 0): [2, 3]}


def test_known_answers_on_a_5_by_4_image():
    cost = np.array(HAND_COST, np.uint8)
    q = pr.params(1, 0, max_path_cells=20)
    for f in (pr.potential_dijkstra, pr.potential_relaxed):
        assert f(cost, q, HAND_GOAL).tolist() == HAND_POT
    pot = np.array(HAND_POT, np.uint32)
    for start, want in HAND_PATHS.items():
        cells, status, ps = pr.walk(pot, cost, q, HAND_GOAL, start, 20)
        assert cells.tolist() == want and status == pr.FOUND and ps == HAND_POT[start[1]][start[0]]
        assert pr.check_path(cells, status, pot, cost, q, HAND_GOAL) == ps
    for (x, y), want in HAND_TIES.items():
        assert pr.ties(pot, cost, q, HAND_GOAL, x, y) == want
    assert pr.walk(pot, cost, q, HAND_GOAL, (1, 1), 20)[1:] == (pr.PATH_UNREACHABLE, U)


def starts_of(pot, goal, n=4, seed=5):
    """The goal itself, the reachable cell farthest from it, a few random reachable cells and an unreachable one if there is one."""
    ny, nx = pot.shape
    reach = np.argwhere(pot != U)
    far = reach[np.argmax(pot[pot != U])]
    rng = np.random.default_rng(seed)
    out = [tuple(goal), (int(far[1]), int(far[0]))] + [(int(x), int(y)) for y, x in reach[rng.integers(0, len(reach), n)]]
    lost = np.argwhere(pot == U)
    return out + ([(int(lost[0][1]), int(lost[0][0]))] if len(lost) else [])


def test_path_invariants_on_every_case(random_cases):
    hand = (np.array(HAND_COST, np.uint8), HAND_GOAL, pr.params(1, 0, max_path_cells=20), np.array(HAND_POT, np.uint32))
    found = lost = 0
    for cost, goal, q, pot in random_cases + [hand]:
        ny, nx = cost.shape
        for start in starts_of(pot, goal):
            cells, status, ps = pr.walk(pot, cost, q, goal, start, nx * ny)
            assert ps == pot[start[1], start[0]]
            if ps == U:
                assert status == pr.PATH_UNREACHABLE and len(cells) == 0
                lost += 1
                continue
            assert status == pr.FOUND and cells[0] == start[0] + start[1] * nx and pr.check_path(cells, status, pot, cost, q, goal) == ps
            assert (len(cells) == 1) == (start == tuple(goal))
            found += 1
            # truncation exactly at, one below and one above the path's length
            n = len(cells)
            for cap in (n, n - 1, n + 1):
                if cap >= 1:
                    c2, s2, _ = pr.walk(pot, cost, q, goal, start, cap)
                    assert c2.tolist() == cells[:cap].tolist() and s2 == (pr.TRUNCATED if cap < n else pr.FOUND)
                    pr.check_path(c2, s2, pot, cost, q, goal)
    assert found > 40 and lost > 5


REFUSED_PARAMS = [dict(neutral=0), dict(neutral=256), dict(neutral=1 << 31), dict(cost_factor_q8=257), dict(cost_factor_q8=1 << 31),
                  dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(max_path_cells=0), dict(max_path_cells=16 * 8 + 1)]
RANGE_WINDOW = (1101, 1100)                          # 7 * 507 * (nx * ny - 1) is above 0xFFFFFFFE here, 7 * 506 * (nx * ny - 1) is not
# The cell count exactly at the limit, within the cost layer's axis limit: neutral 255 and factor 249 give w_max 500, and
# 7 * 500 * (1227134 - 1) <= 0xFFFFFFFE < 7 * 500 * 1227134. 1634 x 751 = 1227134 cells is the largest window for these weights
# (a rule with nx * ny in place of nx * ny - 1 would refuse it), 2015 x 609 = 1227135 cells is one cell too many.
RANGE_PARAMS = (255, 249)
RANGE_LARGEST, RANGE_ONE_MORE = (1634, 751), (2015, 609)


def test_every_refusal_of_the_restatement():
    ok = pr.params(max_path_cells=16 * 8)
    assert pr.refusal(ok) is None and pr.refusal(dict(ok, flags=1)) is None
    bad = lambda **kw: pr.refusal(dict(ok, **kw))
    assert bad(neutral=0) == bad(neutral=256) == "neutral" and bad(neutral=1) is None and bad(neutral=255) is None
    assert bad(cost_factor_q8=257) == "factor" and bad(cost_factor_q8=0) is None and bad(cost_factor_q8=256) is None
    assert bad(flags=2) == bad(flags=3) == bad(flags=1 << 31) == "flags"
    assert bad(max_path_cells=0) == bad(max_path_cells=129) == "max_path_cells" and bad(max_path_cells=1) is None
    assert all(pr.refusal(dict(ok, **kw)) is not None for kw in REFUSED_PARAMS)
    assert pr.refusal(ok, have_cost=False) == "cost" and pr.refusal(ok, in_flight=True) == "flight"
    # step 5 at its exact boundary: the largest window for the largest weight, and one cell more
    top = pr.params(255, 256, max_path_cells=1)
    assert 7 * 507 * (1210191 - 1) <= 0xFFFFFFFE < 7 * 507 * (1210192 - 1)
    assert pr.refusal(top, 1210191, 1) is None and pr.refusal(top, 1210192, 1) == "range"
    assert pr.refusal(top, *RANGE_WINDOW) == "range" and pr.refusal(pr.params(255, 255, max_path_cells=1), *RANGE_WINDOW) is None
    edge = pr.params(*RANGE_PARAMS, max_path_cells=1)
    assert pr.w_max(edge) == 500 and RANGE_LARGEST[0] * RANGE_LARGEST[1] == 1227134 == RANGE_ONE_MORE[0] * RANGE_ONE_MORE[1] - 1
    assert 7 * 500 * (1227134 - 1) <= 0xFFFFFFFE < 7 * 500 * 1227134 and max(RANGE_LARGEST + RANGE_ONE_MORE) <= cr.MAX_AXIS
    assert pr.refusal(edge, *RANGE_LARGEST) is None and pr.refusal(edge, *RANGE_ONE_MORE) == "range"
    assert pr.refusal(dict(ok, max_path_cells=1), 1000, 1000) is None and pr.refusal(dict(ok, max_path_cells=1), 2048, 2048) == "range"


def test_window_cells():
    assert pr.window_cell(0.05, -0.05, 0.1, (-8, -4), 16, 8) == (8, 3)
    assert pr.window_cell(0.75, 0.0, 0.1, (-8, -4), 16, 8) == (15, 4) and pr.window_cell(0.85, 0.0, 0.1, (-8, -4), 16, 8) is None
    for v in (np.nan, np.inf, -np.inf, 3e38):
        assert pr.window_cell(v, 0.0, 0.1, (-8, -4), 16, 8) is None and pr.window_cell(0.0, v, 0.1, (-8, -4), 16, 8) is None
    for ix, iy in ((0, 0), (15, 7), (3, 5)):
        assert pr.window_cell(*pr.cell_centre(ix, iy, 0.1, (-8, -4)), 0.1, (-8, -4), 16, 8) == (ix, iy)


# ---- designed images ------------------------------------------------------------------------------------------------------
OUTSIDE = tc.OUTSIDE
INSIDE = (0.0, 0.0, 0.0)
WALLS = cr.params(0.0, 0.0, 3.0)                     # R = 0: the obstacle cells are 254 and nothing else is inflated
GRADED = dict(cr.params(0.15, 0.85, 3.0), flags=cr.INFLATE_UNKNOWN)


def plan_tuple(info):
    return (tuple(info.goal), info._pad)


def path_tuple(info):
    return (tuple(info.start), tuple(info.goal), info.n_cells, info.status, info.pot_start, info._pad)


def make_cost(cm, nx, ny, cells, trans, cq, cell=0.1, exact=True):
    """One frame with the wanted obstacle cells into a fresh map, the cost layer over it: (cost, map info)."""
    tm.configure(cm, tc.map_q(cell, nx, ny))
    tg.run_frame(cm, tc.frame_of(cells, cell, nx, ny, trans), tc.PARAMS)
    minfo = cm.map_integrate(None)
    cm.map_cost_configure(cq["inscribed_radius"], cq["inflation_radius"], cq["cost_scaling"], bool(cq["flags"] & 1))
    cm.map_cost_update()
    cost = cm.map_cost()[0]
    if exact:
        want = np.zeros(cost.shape, bool)
        if len(cells):
            want[np.asarray(cells)[:, 1], np.asarray(cells)[:, 0]] = True
        assert ((cost == 254) == want).all()
    return cost, minfo


def plan(cm, cost, minfo, q, goal, need=(), starts=None, label="", cell=0.1, caps=False, want=None):
    """Configure, update, read everything back and compare with the restatement of the library's own cost table (or with
    `want`, where the caller has a closed form): pot, both infos, the device table, then paths from `starts` and, with caps,
    with max_path_cells at, one below and one above the length of the second one's path, and 1."""
    ny, nx = cost.shape
    anchor = tuple(minfo.anchor)
    q = dict(q, max_path_cells=q["max_path_cells"] or nx * ny)
    want = pr.potential_relaxed(cost, q, goal) if want is None else want
    pr.guards(want, cost, q, goal, need)
    gx, gy = pr.cell_centre(*goal, cell, anchor)
    assert pr.window_cell(gx, gy, cell, anchor, nx, ny) == tuple(goal)
    cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], bool(q["flags"] & 1), q["max_path_cells"])
    info = cm.map_plan_update(gx, gy)
    pot, i1 = cm.map_plan()
    ptr, i2, m2 = cm.map_plan_device()
    reach = want != U
    print(f"{label}: {nx} x {ny} goal {goal} sweeps {info.n_sweeps} reachable {int(reach.sum())} of {int((pr.weights(cost, q) > 0).sum())} passable, "
          f"largest pot {int(want[reach].max())}")
    assert plan_tuple(info) == plan_tuple(i1) == plan_tuple(i2) == (tuple(goal), 0) and info.n_sweeps == i1.n_sweeps == i2.n_sweeps >= 1
    assert tm.info_tuple(m2) == tm.info_tuple(minfo) and ptr
    assert pot.dtype == np.uint32 and pot.shape == want.shape
    if pot.tobytes() != want.tobytes():
        bad = np.argwhere(pot != want)
        iy, ix = bad[0]
        raise AssertionError(f"{label}: pot differs in {len(bad)} of {want.size} cells, first ({ix}, {iy}): got {pot[iy, ix]} want {want[iy, ix]}")
    dev = np.zeros_like(pot)
    assert tg.hip_rt().hipMemcpy(C.c_void_p(dev.ctypes.data), C.c_void_p(ptr), C.c_size_t(pot.nbytes), 2) == 0
    assert dev.tobytes() == want.tobytes(), label
    for start in starts if starts is not None else starts_of(want, goal):
        paths(cm, cost, minfo, q, goal, want, start, label, cell)
    if caps:
        start = (starts if starts is not None else starts_of(want, goal))[1]
        n = len(pr.walk(want, cost, q, goal, start, nx * ny)[0])
        for cap in (n, n - 1, n + 1, 1):
            cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], bool(q["flags"] & 1), cap)
            cm.map_plan_update(gx, gy)
            paths(cm, cost, minfo, dict(q, max_path_cells=cap), goal, want, start, f"{label} cap {cap}", cell)
        cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], bool(q["flags"] & 1), q["max_path_cells"])
        cm.map_plan_update(gx, gy)
    return want, info


def paths(cm, cost, minfo, q, goal, want, start, label, cell=0.1):
    nx = cost.shape[1]
    cells, status, ps = pr.walk(want, cost, q, goal, start, q["max_path_cells"])
    if len(cells):
        pr.check_path(cells, status, want, cost, q, goal)
    got, info = cm.map_path(*pr.cell_centre(*start, cell, tuple(minfo.anchor)))
    assert path_tuple(info) == (tuple(start), tuple(goal), len(cells), status, ps, 0), (label, start, path_tuple(info))
    assert got.dtype == np.uint32 and got.tobytes() == cells.tobytes(), (label, start)
    return cells, status


def serpentine(nx, ny, pitch=10):
    """Walls across x every `pitch` rows with a gap of two cells that alternates between the two ends."""
    cells = []
    for k, y in enumerate(range(pitch // 2, ny, pitch)):
        cells += [(x, y) for x in (range(0, nx - 2) if k % 2 else range(2, nx))]
    return cells


def room(x0, y0, x1, y1):
    return sorted({(x, y) for x in range(x0, x1 + 1) for y in (y0, y1)} | {(x, y) for y in range(y0, y1 + 1) for x in (x0, x1)})


SHAPES = ((1, 1), (70, 1), (1, 70), (65, 33), (33, 65), (257, 255))                                # (nx, ny)


def goals_of(nx, ny):
    """A tile's first and last cell, a cell of the last (corner) tile, the middle."""
    t = TILE
    out = {(0, 0), (min(t, nx) - 1, min(t, ny) - 1), (nx - 1, ny - 1), (nx // 2, ny // 2)}
    if nx > t:
        out |= {(t, 0), (t - 1, min(t, ny) - 1)}
    if ny > t:
        out |= {(0, t), (min(t, nx) - 1, t - 1)}
    return sorted(out)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_obstacle_at_all_against_the_closed_form(shape):
    """A sensor outside and no point in the window: the cost table is all 255, which CM_PLAN_ALLOW_UNKNOWN makes 252; without
    the flag nothing but the goal has a potential. Goals on a tile's first and last cell and in the corner tile."""
    nx, ny = shape
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, [], OUTSIDE, WALLS)
        assert (cost == 255).all()
        for goal in goals_of(nx, ny):
            plan(cm, cost, minfo, pr.params(7, 0, pr.ALLOW_UNKNOWN), goal, label=f"empty {goal}", want=pr.closed_form(nx, ny, goal, 7),
                 starts=[goal, (0, 0), (nx - 1, ny - 1), (nx - 1, 0)])
        goal = goals_of(nx, ny)[-1]
        alone = np.full((ny, nx), U, np.uint32)
        alone[goal[1], goal[0]] = 0
        plan(cm, cost, minfo, pr.params(50, 205, 0), goal, need=("nothing_passable",), label="empty, unknown not allowed", want=alone)
        plan(cm, cost, minfo, pr.params(50, 205, 1), goals_of(nx, ny)[0], label="empty 50 / 205", want=pr.closed_form(nx, ny, goals_of(nx, ny)[0], 251))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_obstacles_on_a_graded_field(shape):
    """17 % obstacles under a sensor outside the window, inflated into the unknown: a graded field with both flag settings. On
    the two shapes that are one cell wide every obstacle is a wall across the whole window, so at 17 % the goal reaches a
    handful of cells: they run at 17 % as well, and also at 3 %, where the reachable stretch is a few dozen cells."""
    nx, ny = shape
    with capi.CloudMerger(max_points_total=nx * ny + 4096, max_sensors=1) as cm:
        for share in (0.17,) if min(nx, ny) > 1 else (0.17, 0.03):
            rng = np.random.default_rng(nx * 1000 + ny)
            cells = [(x, y) for y in range(ny) for x in range(nx) if rng.random() < share and (x, y) != (nx // 3, ny // 2)]
            cost, minfo = make_cost(cm, nx, ny, cells, OUTSIDE, dict(GRADED, inscribed_radius=0.0))
            big = min(nx, ny) >= 33
            plan(cm, cost, minfo, pr.params(flags=1), (nx // 3, ny // 2), need=("graded", "mostly_reachable", "several_tiles") if big else ("graded",),
                 label=f"random {share}, unknown allowed", caps=True)
            plan(cm, cost, minfo, pr.params(flags=0), (nx // 3, ny // 2), label=f"random {share}, unknown not allowed")
            plan(cm, cost, minfo, pr.params(flags=1), cells[len(cells) // 2], need=("goal_impassable",), label=f"random {share}, goal in a lethal cell")


@pytest.mark.gpu
def test_free_cells_of_a_sensor_inside_the_window():
    """The sensor inside the window clears cells: known free cells beside unknown ones, so the flag decides what is reachable."""
    nx, ny = 65, 33
    cells = sorted(set(tc.scattered(3, nx, ny, 40)) - {(nx // 2, ny // 2)})
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, cells, INSIDE, cr.params(0.05, 0.45, 3.0))
        assert (cost == 255).any() and (cost < 253).any()
        a, _ = plan(cm, cost, minfo, pr.params(flags=0), (nx // 2, ny // 2), need=("graded",), label="inside, unknown not allowed")
        b, _ = plan(cm, cost, minfo, pr.params(flags=1), (nx // 2, ny // 2), need=("graded", "mostly_reachable"), label="inside, unknown allowed")
        assert (a != U).sum() < (b != U).sum()


@pytest.mark.gpu
def test_a_serpentine_re_enters_tiles():
    """70 x 130, walls whose gaps alternate between the two ends: the shortest path crosses every tile edge many times, so no
    single sweep can finish a tile."""
    nx, ny = 70, 130
    cells = serpentine(nx, ny)
    with capi.CloudMerger(max_points_total=nx * ny, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, cells, OUTSIDE, WALLS)
        want, info = plan(cm, cost, minfo, pr.params(flags=1), (nx // 2, 0), need=("mostly_reachable", "detour", "several_tiles"),
                          starts=[(nx // 2, ny - 1), (0, ny - 1), (nx // 2, 0), (3, 77)], label="serpentine", caps=True)
        assert info.n_sweeps >= 2


@pytest.mark.gpu
def test_a_wall_makes_first_values_wrong_until_another_side_improves_them():
    """Two walls with their gaps at opposite ends and a field that is cheapest a little way off them: a tile behind a wall first
    gets values through whatever reached it first, and later sweeps lower them from another side."""
    nx, ny = 96, 64
    wall = [(40, y) for y in range(4, ny)] + [(56, y) for y in range(0, ny - 4)]
    with capi.CloudMerger(max_points_total=nx * ny, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, wall, OUTSIDE, dict(cr.params(0.0, 1.25, 0.5), flags=cr.INFLATE_UNKNOWN), exact=False)
        want, info = plan(cm, cost, minfo, pr.params(1, 256, 1), (8, ny // 2), need=("graded", "mostly_reachable", "several_tiles"),
                          label="two walls", starts=[(nx - 1, ny // 2), (48, ny // 2), (41, ny - 1)])
        assert info.n_sweeps >= 2


@pytest.mark.gpu
def test_a_closed_room_every_cell_lethal_and_a_goal_in_a_lethal_cell():
    nx, ny = 65, 33
    with capi.CloudMerger(max_points_total=nx * ny, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, room(28, 10, 40, 22), OUTSIDE, WALLS)
        plan(cm, cost, minfo, pr.params(flags=1), (2, 2), need=("some_unreachable", "several_tiles"), starts=[(34, 16), (2, 2), (64, 32)],
             label="room from outside")
        want, _ = plan(cm, cost, minfo, pr.params(flags=1), (34, 16), need=("some_unreachable",), starts=[(2, 2), (29, 11), (39, 21)],
                       label="room from inside")
        assert (want != U).sum() == 11 * 11
        plan(cm, cost, minfo, pr.params(flags=1), (28, 16), need=("goal_impassable", "mostly_reachable"), starts=[(2, 2), (34, 16), (28, 15)],
             label="goal in the wall")                 # (both sides of the wall reach it; the wall cell above it does not)
        cost, minfo = make_cost(cm, nx, ny, [(x, y) for y in range(ny) for x in range(nx)], OUTSIDE, WALLS)
        for f in BOTH:
            plan(cm, cost, minfo, pr.params(flags=f), (TILE, TILE), need=("nothing_passable", "goal_impassable"), starts=[(TILE, TILE), (0, 0)],
                 label="every cell lethal")


@pytest.mark.gpu
def test_parameter_extremes_and_the_corner_trap():
    """cost_factor_q8 0 and 256, neutral 1 and 255; the 5 x 4 image by hand with inscribed radius 0."""
    nx, ny = 65, 33
    cells = sorted(set(tc.scattered(7, nx, ny, 60)) - {(5, 5)})
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        cost, minfo = make_cost(cm, nx, ny, cells, OUTSIDE, GRADED, exact=False)
        for neutral, factor in ((1, 0), (1, 256), (255, 0), (255, 256), (50, 205)):
            for f in BOTH:
                plan(cm, cost, minfo, pr.params(neutral, factor, f), (5, 5), need=("graded", "mostly_reachable") if f and factor else (),
                     label=f"{neutral} / {factor} flags {f}")
        lethal = [(x, y) for y in range(4) for x in range(5) if HAND_COST[y][x] == 254]
        cost, minfo = make_cost(cm, 5, 4, lethal, OUTSIDE, WALLS)
        q = pr.params(1, 0, 1)
        assert pr.weights(cost, q).tolist() == pr.weights(np.array(HAND_COST, np.uint8), q).tolist()
        want, _ = plan(cm, cost, minfo, q, HAND_GOAL, starts=list(HAND_PATHS) + [(1, 1), (4, 0), (3, 0)], label="corner trap", caps=True)
        assert want.tolist() == HAND_POT
        for start, cells in HAND_PATHS.items():        # (plan() compared them with the walk; here with the hand's)
            assert cm.map_path(*pr.cell_centre(*start, 0.1, tuple(minfo.anchor)))[0].tolist() == cells


@pytest.mark.gpu
def test_a_three_frame_sequence_with_a_scroll_beside_a_context_without_the_layer():
    nx, ny, cell, poses = tc.SEQ
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm, capi.CloudMerger(max_points_total=4096, max_sensors=1) as never:
        for c in (cm, never):
            tm.configure(c, tc.map_q(cell, nx, ny))
            c.map_cost_configure(GRADED["inscribed_radius"], GRADED["inflation_radius"], GRADED["cost_scaling"], True)
        cm.map_plan_configure(50, 205, True)
        for k, xy in enumerate(poses):
            cells, _ = tc.seq_cells(k)
            outs = []
            for c in (cm, never):
                res = tg.run_frame(c, tc.frame_of(cells, cell, nx, ny, OUTSIDE, xy), tc.PARAMS)
                outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), c.merged(4096).tobytes()))
            assert outs[0] == outs[1]                  # the frame behind a plan: that of a context that never had the layer
            infos = [c.map_integrate(tm.pose_t(xy[0], xy[1])) for c in (cm, never)]
            assert tm.info_tuple(infos[0]) == tm.info_tuple(infos[1])
            for c in (cm, never):
                c.map_cost_update()
            anchor = tuple(infos[0].anchor)
            cost = cm.map_cost()[0]
            goal, q = (nx - 5, ny // 2), pr.params(flags=1, max_path_cells=nx * ny)
            want = pr.potential_relaxed(cost, q, goal)
            pr.guards(want, cost, q, goal, ("graded", "mostly_reachable"))
            cm.map_plan_update(*pr.cell_centre(*goal, cell, anchor))
            assert cm.map_plan()[0].tobytes() == want.tobytes()
            paths(cm, cost, infos[0], q, goal, want, (nx // 2, ny // 2), f"frame {k}", cell)       # from the vehicle cell
            assert cm.map()[0].tobytes() == never.map()[0].tobytes() and cm.map_occupancy()[0].tobytes() == never.map_occupancy()[0].tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(cm.map_cost()[:2], never.map_cost()[:2]))
            assert tm.info_tuple(cm.map()[1]) == tm.info_tuple(never.map()[1])


@pytest.mark.gpu
def test_staleness_and_lifetime():
    nx, ny, cell = 64, 48, 0.1
    cells = tc.CORNERS_64_48
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, tc.map_q(cell, nx, ny))
        tm.refused(cm, cm.map_plan_configure, text=b"cm_map_cost_configure")                   # no cost layer
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        cm.map_plan_configure(50, 205, True)
        L = cm._lib
        buf = np.full(nx * ny, 7, np.uint32)
        for call in (cm.map_plan, cm.map_plan_device, lambda: cm.map_path(0.0, 0.0)):
            tm.refused(cm, call, text=b"stale")
            tm.refused(cm, call, text=b"cm_map_plan_configure")                                # ... which names the reason
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_cost_update")               # the cost layer itself is stale
        cm.map_cost_update()
        tm.refused(cm, cm.map_plan, text=b"cm_map_cost_update")
        info = cm.map_plan_update(3.25, 2.45)          # before any integration (the anchor is (0, 0)): all unknown, allowed
        pot, _ = cm.map_plan()
        assert tuple(info.goal) == (32, 24) and pot.tobytes() == pr.closed_form(nx, ny, (32, 24), 251).tobytes()
        tg.run_frame(cm, tc.frame_of(cells, cell, nx, ny, OUTSIDE), tc.PARAMS)
        assert cm.map_plan()[0].tobytes() == pot.tobytes()                                     # a merge leaves the layer alone
        cm.map_integrate(None)
        for call in (cm.map_plan, cm.map_plan_device, lambda: cm.map_path(0.0, 0.0)):
            tm.refused(cm, call, text=b"cm_map_integrate")
        assert L.cm_map_plan_copy(cm._ctx, buf.ctypes.data, nx * ny, None, None) == capi.BAD_ARG and (buf == 7).all()
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"stale")                            # ... and so is the cost layer
        cm.map_cost_update()
        tm.refused(cm, cm.map_plan, text=b"cm_map_cost_update")
        cm.map_plan_update(0.05, 0.05)
        pot2, _ = cm.map_plan()
        assert pot2.tobytes() != pot.tobytes() and pot2.tobytes() == pr.potential_relaxed(cm.map_cost()[0], pr.params(flags=1), (32, 24)).tobytes()
        cm.map_plan_configure(50, 205, True)           # configure again: stale again
        tm.refused(cm, cm.map_plan, text=b"cm_map_plan_configure")
        cm.map_plan_update(0.05, 0.05)
        # each configure call above it frees the layer
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_plan_configure")
        cm.map_cost_update()
        cm.map_plan_configure(50, 205, True)
        cm.map_cost_configure(None)
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_cost_configure")
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        cm.map_plan_configure(50, 205, True)
        tm.configure(cm, tc.map_q(cell, nx, ny))
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_cost_configure")
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        cm.map_plan_configure(50, 205, True)
        cm.map_configure(None)
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_configure")
        cm.map_plan_configure(None)                    # freeing what is not there is fine


@pytest.mark.gpu
def test_refusals_and_capacity():
    nx, ny, cell = 16, 8, 0.5
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        L = cm._lib
        tm.refused(cm, cm.map_plan_configure, text=b"cm_map_configure")                        # no map
        for call in (cm.map_plan, cm.map_plan_device, lambda: cm.map_path(0.0, 0.0), lambda: cm.map_plan_update(0.0, 0.0)):
            tm.refused(cm, call, text=b"cm_map_configure")
        tm.configure(cm, tc.map_q(cell, nx, ny))
        assert pr.refusal(pr.params(max_path_cells=1), nx, ny, have_cost=False) == "cost"
        tm.refused(cm, cm.map_plan_configure, text=b"cm_map_cost_configure")                   # a map, no cost layer
        cm.map_cost_configure(0.0, 1.0, 1.0, True)
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_plan_configure")            # a cost layer, no plan layer
        ok = pr.params(max_path_cells=nx * ny)
        for kw in REFUSED_PARAMS:                      # every refusal of the restatement's validator is the library's
            q = dict(ok, **kw)
            assert pr.refusal(q, nx, ny) is not None
            p = capi.PlanParams(q["neutral"], q["cost_factor_q8"], q["flags"], q["max_path_cells"])
            assert L.cm_map_plan_configure(cm._ctx, C.byref(p)) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
        tm.refused(cm, cm.map_plan_update, 0.0, 0.0, text=b"cm_map_plan_configure")            # a refused call configured nothing
        for q in (ok, dict(ok, neutral=1, cost_factor_q8=0), dict(ok, neutral=255, cost_factor_q8=256, flags=1), dict(ok, max_path_cells=1)):
            assert pr.refusal(q, nx, ny) is None
            cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], bool(q["flags"]), q["max_path_cells"])
        # step 5 at its boundary: the largest weight on a window of 1101 x 1100, and one less
        tm.configure(cm, tc.map_q(cell, *RANGE_WINDOW))
        cm.map_cost_configure(0.0, 1.0, 1.0, True)
        tm.refused(cm, cm.map_plan_configure, 255, 256, False, 1, text=b"0xFFFFFFFE")
        cm.map_plan_configure(255, 255, False, 1)
        # ... and the cell count exactly at the limit for w_max 500, then one cell more
        tm.configure(cm, tc.map_q(cell, *RANGE_LARGEST))
        cm.map_cost_configure(0.0, 1.0, 1.0, True)
        cm.map_plan_configure(*RANGE_PARAMS, False, 1)
        tm.configure(cm, tc.map_q(cell, *RANGE_ONE_MORE))
        cm.map_cost_configure(0.0, 1.0, 1.0, True)
        tm.refused(cm, cm.map_plan_configure, *RANGE_PARAMS, False, 1, text=b"0xFFFFFFFE")
        tm.configure(cm, tc.map_q(cell, nx, ny))
        cm.map_cost_configure(0.0, 1.0, 1.0, True)
        cm.map_plan_configure(50, 205, True)
        tg.run_frame(cm, tc.frame_of([(3, 2)], cell, nx, ny, OUTSIDE), tc.PARAMS)
        minfo = cm.map_integrate(None)
        cm.map_cost_update()
        anchor = tuple(minfo.anchor)
        # goals and starts that are not finite, have no cell or lie outside the window
        outside = [(np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0), (3e38, 0.0), ((anchor[0] + nx + 0.5) * cell, 0.0), (0.0, (anchor[1] - 0.5) * cell)]
        for x, y in outside:
            assert pr.window_cell(x, y, cell, anchor, nx, ny) is None
            tm.refused(cm, cm.map_plan_update, x, y, text=b"goal")
        info = cm.map_plan_update(*pr.cell_centre(12, 6, cell, anchor))
        pot, _ = cm.map_plan()
        for x, y in outside:
            tm.refused(cm, cm.map_path, x, y, text=b"start")
        # destinations that are too small: CM_CAPACITY, nothing copied, the infos still written
        n = nx * ny
        buf = np.full(n, 7, np.uint32)
        for cap in (n - 1, 0):
            got, m = capi.PlanInfo(), capi.MapInfo()
            assert L.cm_map_plan_copy(cm._ctx, buf.ctypes.data, cap, C.byref(got), C.byref(m)) == capi.CAPACITY and (buf == 7).all()
            assert plan_tuple(got) == plan_tuple(info) == ((12, 6), 0) and tm.info_tuple(m) == tm.info_tuple(minfo)
        assert L.cm_map_plan_copy(cm._ctx, buf.ctypes.data, n + 5, None, None) == capi.OK and buf.tobytes() == pot.tobytes()
        assert L.cm_map_plan_copy(cm._ctx, None, n, None, None) == capi.BAD_ARG                # no destination
        sx, sy = pr.cell_centre(1, 1, cell, anchor)
        cells, pinfo = cm.map_path(sx, sy)
        assert pinfo.n_cells == len(cells) > 3 and pinfo.status == pr.FOUND
        buf = np.full(n, 7, np.uint32)
        for cap in (len(cells) - 1, 0):
            got = capi.PathInfo()
            assert L.cm_map_plan_path(cm._ctx, sx, sy, buf.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (buf == 7).all()
            assert path_tuple(got) == path_tuple(pinfo)
        assert L.cm_map_plan_path(cm._ctx, sx, sy, buf.ctypes.data, len(cells), None) == capi.OK and buf[:len(cells)].tobytes() == cells.tobytes()
        assert (buf[len(cells):] == 7).all()
        assert L.cm_map_plan_path(cm._ctx, sx, sy, None, n, None) == capi.BAD_ARG              # no destination
        ptr = C.c_void_p()
        assert L.cm_map_plan_device(cm._ctx, C.byref(ptr), None, None) == capi.OK and ptr.value
        assert L.cm_map_plan_device(cm._ctx, None, None, None) == capi.OK
        # a frame in flight
        cm.submit_all(tc.frame_of([(3, 2)], cell, nx, ny, OUTSIDE))
        cm.merge_voxelize_async(capi.make_params(tc.PARAMS))
        assert pr.refusal(ok, nx, ny, in_flight=True) == "flight"
        for call in (cm.map_plan_configure, cm.map_plan, cm.map_plan_device, lambda: cm.map_path(sx, sy), lambda: cm.map_plan_update(sx, sy)):
            tm.refused(cm, call, text=b"flight")
        assert cm.wait().status == capi.OK
        assert cm.map_plan()[0].tobytes() == pot.tobytes()                                     # none of it touched the table


@pytest.mark.gpu
def test_stage_names_under_profile():
    nx, ny, cell = 40, 24, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        cost, minfo = make_cost(cm, nx, ny, [(3, 2)], OUTSIDE, GRADED)
        cm.map_plan_configure(50, 205, True)
        assert not any("plan" in n for n, _ in cm.stage_times())
        cm.map_plan_update(0.05, 0.05)
        assert [n for n, _ in cm.stage_times()] == ["k_plan_init", "k_plan_sweep"]
        cm.map_path(1.0, 0.5)
        assert [n for n, _ in cm.stage_times()] == ["k_plan_path"] and all(ms >= 0.0 for _, ms in cm.stage_times())
        tg.run_frame(cm, tc.frame_of([(3, 2)], cell, nx, ny, OUTSIDE), tc.PARAMS)   # a frame's own list never holds the call's stages
        assert not any("plan" in n for n, _ in cm.stage_times())


# ---- no update or path call allocates: the counts of the test build, as tests/test_ctx_memory.py takes them --------------------
def case_no_plan_call_allocates():
    nx, ny, cell = 96, 64, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, tc.map_q(cell, nx, ny))
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        before = capi.device_allocations()
        cm.map_plan_configure(50, 205, True)           # every buffer of the layer is taken here:
        after = capi.device_allocations()
        assert [a - b for a, b in zip(after, before)] == [4, 4]        # pot, the flags and counters, the path, the page-locked words
        totals = []
        for k in range(4):
            if k:
                tg.run_frame(cm, tc.frame_of(tc.scattered(23 + k, nx, ny, 9), cell, nx, ny, OUTSIDE), tc.PARAMS)
                cm.map_integrate(tm.pose_t(0.0, 0.0))
            cm.map_cost_update()
            b = capi.device_allocations()
            cm.map_plan_update(0.05 + k, 0.05)         # (k = 0: the first one, before any integration)
            cm.map_plan()
            cm.map_plan_device()
            cm.map_path(2.0, 1.0)
            a = capi.device_allocations()
            print(f"update {k}: before {b} after {a}")
            totals.append((b, a))
        assert all(b == a for b, a in totals), totals
        live = capi.device_allocations()[0]
        cm.map_plan_configure(None)
        assert capi.device_allocations()[0] == live - 4
        cm.map_plan_configure(50, 205, True)
        cm.map_cost_configure(None)                    # the cost layer takes the plan layer with it
        assert capi.device_allocations()[0] == live - 4 - 4


@pytest.mark.gpu
def test_no_plan_update_or_path_call_allocates():
    assert os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")), "the test build is missing"
    env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK")}
    env.update(CM_LIB_VARIANT="testhooks", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_map_plan", "no_plan_call_allocates"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    {"no_plan_call_allocates": case_no_plan_call_allocates}[sys.argv[1]]()
