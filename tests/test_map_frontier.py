"""The frontier layer behind the plan layer: cm_map_frontier_configure, cm_map_frontier_update, cm_map_frontier_copy,
cm_map_frontier_labels_copy, cm_map_frontier_device (include/cloudmerge.h, cm_kernels_front.hip).

The bar on the GPU: every byte of the labels, of the table, of all infos and of the device-pointer variant equal to the
restatement (tests/front_ref.py) fed with the library's own image (map_occupancy()), cost table (map_cost()) and potential
(map_plan()). There is no tolerance: every quantity is an integer and every reduction commutative. The images come from real
frames through cm_map_integrate: a sensor inside the window paints free cells along its rays into the unknown, so every ray
cell with unknown beside it is a frontier cell; up to 16 sensors per frame give 16 origins, and a sensor far outside the
window adds obstacle cells without rays. The designed scenes are run through the restatements of the map, the cost layer
and the plan layer on the CPU first (test_the_designed_scenes_hold_their_guards), and a GPU case asserts its named guards
(front_ref.guards) again on the image the library actually returned, before anything is compared."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import xyzi_cloud
from tests import cost_ref as cr
from tests import front_ref as fr
from tests import map_ref as mr
from tests import plan_ref as pr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_map_cost as tc
from tests import test_occupancy_map as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
F32 = np.float32
NAMES = ("cm_map_frontier_configure", "cm_map_frontier_update", "cm_map_frontier_copy", "cm_map_frontier_labels_copy",
         "cm_map_frontier_device")
FRONTIER_TYPES = (capi.FrontierParams, capi.Frontier, capi.FrontierInfo)   # (a library without the layer fails every test here, at import)
TILE = tr.device_define("CM_FRONT_TILE")           # the edge of one k_front_local tile in cells
NONE, U = fr.NONE, fr.UNREACHABLE
STAGES = ["k_front_local", "k_front_merge", "k_front_flatten", "k_front_count", "k_front_scan", "k_front_number", "k_front_table",
          "k_front_best"]


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_frontier_structs_and_constants_match_header(tmp_path):
    structs = {"cm_frontier_params": (capi.FrontierParams, ["min_cells", "max_frontiers", "max_cost", "pot_scale", "gain_scale"]),
               "cm_frontier": (capi.Frontier, ["first_cell", "n_cells", "sum_x", "sum_y", "min_pot", "min_pot_cell", "x0", "y0", "x1", "y1"]),
               "cm_frontier_info": (capi.FrontierInfo, ["n_frontier_cells", "n_components", "n_frontiers", "n_written", "best", "best_score"])}
    names = ["CM_FRONTIER_NONE", "CM_FRONTIER_MAX_TABLE", "CM_PLAN_UNREACHABLE"]
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
    assert got[:len(want)] == want == [20, 0, 4, 8, 12, 16, 40, 0, 4, 8, 16, 24, 28, 32, 34, 36, 38, 32, 0, 4, 8, 12, 16, 24]
    assert got[len(want):] == [capi.FRONTIER_NONE, capi.FRONTIER_MAX_TABLE, capi.PLAN_UNREACHABLE] == [fr.NONE, fr.MAX_TABLE, fr.UNREACHABLE]
    assert fr.MAX_TABLE == 1 << 16 == tr.device_define("CM_FRONT_MAX_TABLE_DEV") and fr.NONE == 0xFFFFFFFF
    assert TILE == 32 and tr.device_define("CM_FRONT_BLOCK") == TILE * TILE
    assert capi.FRONTIER_DTYPE == fr.FRONTIER_DTYPE and fr.FRONTIER_DTYPE.itemsize == 40
    for (name, (T, fields)) in list(structs.items())[1:2]:
        assert [fr.FRONTIER_DTYPE.fields[f][1] for f in fields] == [getattr(T, f).offset for f in fields]
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.FrontierParams(1, 16, 252, 1, 0)
    info, minfo = capi.FrontierInfo(), capi.MapInfo()
    before = bytes(info), bytes(minfo)
    buf = np.full(160, 7, np.uint32)
    a, b = C.c_void_p(5), C.c_void_p(6)
    assert L.cm_map_frontier_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_frontier_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_frontier_update(None, C.byref(info), C.byref(minfo)) == capi.BAD_ARG
    assert L.cm_map_frontier_copy(None, buf.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_frontier_labels_copy(None, buf.ctypes.data, 160, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_frontier_device(None, C.byref(a), C.byref(b), C.byref(info)) == capi.BAD_ARG
    assert (buf == 7).all() and (bytes(info), bytes(minfo)) == before and (a.value, b.value) == (5, 6)


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def same(a, b):
    return (a[0].dtype == b[0].dtype == np.uint32 and a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes() and
            a[1].dtype == b[1].dtype == fr.FRONTIER_DTYPE and a[1].tobytes() == b[1].tobytes() and a[2] == b[2])


def random_image(seed, ny, nx):
    """Image values from {-1, 0, 100} at 30 / 45 / 25 %, a uniform cost byte with a fifth above 200, a uniform pot that is
    unreachable in a tenth of the cells and in the whole right third of the image."""
    rng = np.random.default_rng(seed)
    image = rng.choice(np.array([-1, 0, 100], np.int8), (ny, nx), p=[0.30, 0.45, 0.25])
    cost = rng.integers(0, 200, (ny, nx)).astype(np.uint8)
    cost[rng.random((ny, nx)) < 0.2] = 230
    pot = rng.integers(0, 5000, (ny, nx)).astype(np.uint32)
    pot[rng.random((ny, nx)) < 0.1] = U
    pot[:, nx - nx // 3:] = U
    return image, cost, pot


RANDOM_SHAPES = ((1, 1), (1, 70), (70, 1), (33, 65), (67, 129))                                   # (ny, nx)
RANDOM_Q = [fr.params(), fr.params(min_cells=3, max_cost=200, pot_scale=3, gain_scale=40), fr.params(min_cells=2, max_frontiers=2, max_cost=100)]


def test_the_two_restatements_agree_on_random_images():
    for k, (ny, nx) in enumerate(RANDOM_SHAPES):
        image, cost, pot = random_image(300 + k, ny, nx)
        for q in RANDOM_Q:
            a, b = fr.frontiers_flood(image, cost, pot, q), fr.frontiers_propagate(image, cost, pot, q)
            if min(nx, ny) >= 33 and q["max_frontiers"] > 2:       # the vacuity guards first, on the restatement alone
                fr.guards(image, cost, pot, q, b, ("three_frontiers", "unreachable", "all_three_values") + (("small_component",) if q["min_cells"] > 1 else ()))
                assert b[2][4] != NONE and (b[1]["min_pot"] != U).any()
            assert same(a, b), (ny, nx, q)
            labels, table, info = b
            assert info[3] == len(table) == min(info[2], q["max_frontiers"]) and info[0] >= (labels != NONE).sum()
            if info[2]:
                assert int(labels[labels != NONE].max()) == info[2] - 1        # numbers at or above max_frontiers stay in the labels
    # the 1 x 1 images, each value
    for v, n in ((-1, 0), (0, 0), (100, 0)):
        r = fr.frontiers_flood(np.full((1, 1), v, np.int8), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint32), fr.params())
        assert r[2] == (n, 0, 0, 0, NONE, 0, 0) and r[0].tolist() == [[NONE]] and len(r[1]) == 0


# y |  x ->   min_cells 2, max_cost 100, pot_scale 2, gain_scale 5. F free, U unknown, O occupied.
#   row 0:  F U O O F U     (0,0) has U to its right, (1,1) has U above: joined by the diagonal alone, exactly min_cells cells.
#   row 1:  O F O O O O     (4,0) has U to its right and no frontier cell around it: a component of one cell, one short.
#   row 2:  O O O O O O
#   row 3:  F F F O F F     (0,3), (1,3), (2,3) have U below; (2,3) costs 200 > max_cost and is none, (1,3) costs exactly 100.
#   row 4:  U U U O U F     (4,3) has U below, (5,4) has U to its left: a diagonal pair again. (5,3) is free at the window's
#                           edge: F to its left, O above, F below, nothing to its right: no frontier cell.
# pot: (0,0) unreachable, (1,1) 50; (0,3) and (1,3) both 30: the lower cell 18 wins; (4,3) 40, (5,4) 30; (2,3) 5 and (4,0) 1 do
# not count. Scores: 2 * 50 - 5 * 2 = 90, 2 * 30 - 10 = 50, 2 * 30 - 10 = 50: the tie goes to frontier 1.
F_, U_, O_ = 0, -1, 100
HAND_IMAGE = [[F_, U_, O_, O_, F_, U_],
              [O_, F_, O_, O_, O_, O_],
              [O_, O_, O_, O_, O_, O_],
              [F_, F_, F_, O_, F_, F_],
              [U_, U_, U_, O_, U_, F_]]
HAND_COST = [[0, 255, 254, 254, 0, 255],
             [254, 0, 254, 254, 254, 254],
             [254, 254, 254, 254, 254, 254],
             [0, 100, 200, 254, 0, 0],
             [255, 255, 255, 254, 255, 0]]
HAND_POT = [[U, U, U, U, 1, U],
            [U, 50, U, U, U, U],
            [U, U, U, U, U, U],
            [30, 30, 5, U, 40, 45],
            [U, U, U, U, U, 30]]
HAND_Q = fr.params(min_cells=2, max_cost=100, pot_scale=2, gain_scale=5)
N_ = NONE
HAND_LABELS = [[0, N_, N_, N_, N_, N_],
               [N_, 0, N_, N_, N_, N_],
               [N_, N_, N_, N_, N_, N_],
               [1, 1, N_, N_, 2, N_],
               [N_, N_, N_, N_, N_, 2]]
HAND_TABLE = [(0, 2, 1, 1, 50, 7, 0, 0, 1, 1), (18, 2, 1, 6, 30, 18, 0, 3, 1, 3), (22, 2, 9, 7, 30, 29, 4, 3, 5, 4)]
HAND_INFO = (7, 4, 3, 3, 1, 0, 50)


def hand():
    return np.array(HAND_IMAGE, np.int8), np.array(HAND_COST, np.uint8), np.array(HAND_POT, np.uint32)


def test_known_answers_on_a_6_by_5_image():
    image, cost, pot = hand()
    for f in (fr.frontiers_flood, fr.frontiers_propagate):
        labels, table, info = f(image, cost, pot, HAND_Q)
        assert labels.tolist() == HAND_LABELS and table.tolist() == HAND_TABLE and info == HAND_INFO
        # one cell more per frontier is asked for: nothing is left; one less: the single cell is a frontier too, number 1
        assert f(image, cost, pot, dict(HAND_Q, min_cells=3))[2] == (7, 4, 0, 0, NONE, 0, 0)
        l1, t1, i1 = f(image, cost, pot, dict(HAND_Q, min_cells=1))
        assert i1 == (7, 4, 4, 4, 1, 0, 2 * 1 - 5 * 1) and t1.tolist()[1] == (4, 1, 4, 0, 1, 4, 4, 0, 4, 0) and l1[0, 4] == 1 and l1[3, 0] == 2
        # max_cost 200 lets (2, 3) in: frontier 1 has three cells and pot 5
        l2, t2, i2 = f(image, cost, pot, dict(HAND_Q, max_cost=200))
        assert i2 == (8, 4, 3, 3, 1, 0, 2 * 5 - 5 * 3) and t2.tolist()[1] == (18, 3, 3, 9, 5, 20, 0, 3, 2, 3)
        # a table of two entries: frontier 2 stays in the labels, and the choice is among the two
        l3, t3, i3 = f(image, cost, pot, dict(HAND_Q, max_frontiers=2))
        assert l3.tolist() == HAND_LABELS and t3.tolist() == HAND_TABLE[:2] and i3 == (7, 4, 3, 2, 1, 0, 50)
        # no reachable cell anywhere: no choice
        assert f(image, cost, np.full_like(pot, U), HAND_Q)[2] == (7, 4, 3, 3, NONE, 0, 0)
        assert f(image, cost, np.full_like(pot, U), HAND_Q)[1]["min_pot_cell"].tolist() == [NONE] * 3
    fr.guards(image, cost, pot, HAND_Q, (np.array(HAND_LABELS, np.uint32), np.array(HAND_TABLE, fr.FRONTIER_DTYPE), HAND_INFO),
              ("three_frontiers", "small_component", "all_three_values"))


SCORE_DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include "cm_front_score.hpp"
int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4)
        std::printf("%" PRId64 "\n", cm_front_score(static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[i + 1], nullptr, 10)),
                                                    static_cast<uint32_t>(std::strtoul(argv[i + 2], nullptr, 10)), static_cast<uint32_t>(std::strtoul(argv[i + 3], nullptr, 10))));
    return 0;
}
"""


def test_score_arithmetic_on_the_cpu_is_the_restatement(tmp_path):
    """cm_front_score.hpp, which k_front_best includes, in a program of its own under the address and undefined-behaviour
    sanitizers: a signed overflow anywhere in it ends the program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    (tmp_path / "driver.cpp").write_text(SCORE_DRIVER)
    exe = tmp_path / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "cloud_merger_amd", "csrc"), str(tmp_path / "driver.cpp"), "-o", str(exe)], check=True)
    top = 0xFFFFFFFF
    edge = [0, 1, 2, 1 << 22, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, top - 1, top]
    rng = np.random.default_rng(9)
    cases = [(a, b, c, d) for a in edge for b in (0, 1, top) for c in edge for d in (1, 1 << 22, top)]
    cases += [tuple(int(v) for v in rng.integers(0, 1 << 32, 4)) for _ in range(200)]
    r = subprocess.run([str(exe)] + [str(v) for case in cases for v in case], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in r.stdout.split()]
    want = [fr.score(fr.params(pot_scale=a, gain_scale=b), c, d) for a, b, c, d in cases]
    assert got == want and fr.INT64_MAX in got and min(got) == -(1 << 63) and any(0 < v < fr.INT64_MAX for v in got)


def test_the_score_does_not_wrap():
    top = 0xFFFFFFFF
    assert fr.score(fr.params(pot_scale=top, gain_scale=0), top - 1, 1) == fr.INT64_MAX < top * (top - 1)
    assert fr.score(fr.params(pot_scale=top, gain_scale=top), 1 << 31, 5) == top * (1 << 31) - 5 * top < fr.INT64_MAX
    assert fr.score(fr.params(pot_scale=0, gain_scale=top), 77, 1 << 22) == -top * (1 << 22) > -(1 << 63)
    assert fr.score(fr.params(pot_scale=0, gain_scale=0), 77, 9) == 0


REFUSED_PARAMS = [dict(min_cells=0), dict(max_frontiers=0), dict(max_frontiers=fr.MAX_TABLE + 1), dict(max_frontiers=1 << 31),
                  dict(max_cost=253), dict(max_cost=255), dict(max_cost=1 << 31)]


def test_every_refusal_of_the_restatement():
    ok = fr.params()
    assert fr.refusal(ok) is None
    bad = lambda **kw: fr.refusal(dict(ok, **kw))
    assert bad(min_cells=0) == "min_cells" and bad(min_cells=1) is None and bad(min_cells=0xFFFFFFFF) is None
    assert bad(max_frontiers=0) == bad(max_frontiers=fr.MAX_TABLE + 1) == "max_frontiers" and bad(max_frontiers=1) is None and bad(max_frontiers=fr.MAX_TABLE) is None
    assert bad(max_cost=253) == bad(max_cost=1 << 31) == "max_cost" and bad(max_cost=0) is None and bad(max_cost=252) is None
    assert bad(pot_scale=0xFFFFFFFF, gain_scale=0xFFFFFFFF) is None and bad(pot_scale=0, gain_scale=0) is None
    assert all(fr.refusal(dict(ok, **kw)) is not None for kw in REFUSED_PARAMS)
    assert fr.refusal(ok, have_plan=False) == "plan" and fr.refusal(ok, in_flight=True) == "flight"


# ---- designed scenes ------------------------------------------------------------------------------------------------------
# A scene: the window, then its frames; a frame is a list of (origin cell or None, hit cells): one sensor each, standing at the
# centre of its origin cell (None: far outside the window, no rays) with one point at the centre of every hit cell. The
# vehicle stays at the world's origin, so the anchor is (-(nx // 2), -(ny // 2)).
CELL = 0.1
OUTSIDE = tc.OUTSIDE
COST_Q = cr.params(0.05, 0.45, 3.0)
UNKNOWN_HITS = dict(l_occ=86)                        # l_hit 85 < l_occ: a hit cell stays unknown, only the ray is painted


def star(nx=96, ny=96, o=(48, 48), r=40, n=12):
    hits = sorted({(o[0] + int(round(r * np.cos(2 * np.pi * k / n))), o[1] + int(round(r * np.sin(2 * np.pi * k / n)))) for k in range(n)})
    return nx, ny, [[(o, hits)]]


def corner():
    """A row ray, a column ray and the exact diagonal from (20, 20): the diagonal passes (31, 31) and (32, 32), a tile corner."""
    return 70, 70, [[((20, 20), [(60, 20), (20, 60), (44, 44)])]]


def zigzag():
    """Segments (5,5) -> (40,5) -> (40,15) -> (5,15) -> (5,25) -> (40,25): rows 5 and 15 of tile (0, 0) meet only at x = 40."""
    pts = [(5, 5), (40, 5), (40, 15), (5, 15), (5, 25), (40, 25)]
    return 64, 64, [[(a, [b]) for a, b in zip(pts[:-1], pts[1:])]]


def fans(nx=96, ny=64):
    """Three sensors far from one another, each with a few short rays: three frontiers in the order of their first cells;
    the vehicle cell (48, 32) is the second one's origin."""
    return nx, ny, [[((10, 40), [(4, 46), (10, 47), (16, 46)]), ((48, 32), [(40, 26), (48, 24), (56, 26), (58, 32)]),
                     ((80, 8), [(74, 3), (86, 3), (88, 8)])]]


def beside_an_obstacle():
    """A row ray from (10, 20) to (60, 20) and an occupied cell at (35, 23) from a sensor outside: the cost byte rises in the
    middle of the ray and at its end."""
    return 72, 40, [[((10, 20), [(60, 20)]), (None, [(35, 23)])]]


def generic(nx, ny, seed=5):
    """A fan of rays around each quarter point of the window (its hit cells stay unknown under UNKNOWN_HITS, also where they
    lie on another ray), and a few cells hit by two sensors outside, which makes them occupied."""
    rng = np.random.default_rng(seed + 1000 * nx + ny)
    r = max(2, max(nx, ny) // 6 if min(nx, ny) == 1 else min(nx, ny) // 5)
    origins = sorted({(nx // 4, ny // 4), (3 * nx // 4, ny // 4), (nx // 4, 3 * ny // 4), (3 * nx // 4, 3 * ny // 4)}) if nx * ny > 1 else []
    frame = []
    for o in origins:
        hits = {(min(max(o[0] + dx, 0), nx - 1), min(max(o[1] + dy, 0), ny - 1)) for dx, dy in rng.integers(-r, r + 1, (6, 2)).tolist()} - {o}
        if hits:
            frame.append((o, sorted(hits)))
    obstacles = sorted(set(tc.scattered(seed, nx, ny, 5)) - set(origins))
    return nx, ny, [frame + [(None, obstacles), (None, obstacles)]]


SHAPES = ((1, 1), (70, 1), (1, 70), (65, 33), (33, 65), (257, 255))                               # (nx, ny)


def centre_of(ix, iy, nx, ny):
    return ((ix - nx // 2 + 0.5) * CELL, (iy - ny // 2 + 0.5) * CELL)


def clouds_of(frame, nx, ny):
    out = []
    for origin, hits in frame:
        t = centre_of(*origin, nx, ny) + (0.0,) if origin is not None else OUTSIDE
        w = np.array([centre_of(x, y, nx, ny) + (0.0,) for x, y in hits], np.float64)
        p = (w - np.asarray(t, np.float64)).astype(F32)
        out.append(xyzi_cloud(p, np.zeros(len(p), F32), t_xyz=tuple(t)))
    return out


def simulate(scene, mq_kw, plan_q, goal):
    """The scene through the restatements of the map, the cost layer and the plan layer: (image, cost, pot)."""
    nx, ny, frames = scene
    m = mr.MapVectorised(mr.params(CELL, nx, ny, **mq_kw))
    for frame in frames:
        clouds = clouds_of(frame, nx, ny)
        A = np.concatenate([np.concatenate([np.stack([c.data[k] for k in ("x", "y", "z")], axis=1) + F32(c.t_xyz), np.zeros((c.n, 1), F32)], axis=1)
                            for c in clouds]).astype(F32)
        tags = np.concatenate([np.full(c.n, s) for s, c in enumerate(clouds)])
        _, image, _ = m.integrate(A, np.zeros((0, 4), F32), tags, np.zeros(0, np.int64), [c.t_xyz for c in clouds], np.eye(3, 4, dtype=F32))
    cost = tc.restate(image, CELL, COST_Q)[0]
    return image, cost, pr.potential_relaxed(cost, dict(plan_q, max_path_cells=nx * ny), goal)


# name: (scene, map parameters, plan flags, frontier parameters, guards)
CASES = {
    "star": (star(), UNKNOWN_HITS, 1, fr.params(), ("several_tiles",)),
    "corner": (corner(), UNKNOWN_HITS, 1, fr.params(), ("corner_only", "several_tiles")),
    "zigzag": (zigzag(), UNKNOWN_HITS, 1, fr.params(), ("re_enters",)),
    "fans": (fans(), {}, 1, fr.params(pot_scale=3, gain_scale=2), ("three_frontiers", "all_three_values")),
    "behind_a_wall": (fans(), {}, 0, fr.params(), ("three_frontiers", "unreachable")),
    "beside_an_obstacle": (beside_an_obstacle(), {}, 1, fr.params(), ("all_three_values",)),
}


def goal_of(scene):
    return scene[0] // 2, scene[1] // 2


def test_the_designed_scenes_hold_their_guards():
    for name, (scene, mq, flags, q, need) in CASES.items():
        image, cost, pot = simulate(scene, mq, pr.params(flags=flags), goal_of(scene))
        a, b = fr.frontiers_flood(image, cost, pot, q), fr.frontiers_propagate(image, cost, pot, q)
        assert same(a, b), name
        fr.guards(image, cost, pot, q, b, need)
        print(name, b[2], b[1]["n_cells"].tolist())
        if name == "star":
            assert b[2][2] == 1
        if name == "fans":
            assert (b[1]["n_cells"] == b[1]["n_cells"].min()).sum() == 1
    for nx, ny in SHAPES:                              # the rays from the centre of every shape of the GPU part
        image, cost, pot = simulate(generic(nx, ny), UNKNOWN_HITS, pr.params(flags=1), (nx // 2, ny // 2))
        b = fr.frontiers_propagate(image, cost, pot, fr.params())
        if min(nx, ny) >= 33:
            fr.guards(image, cost, pot, fr.params(), b, ("all_three_values", "three_frontiers"))
        assert (b[2][0] > 0) == (nx * ny > 1)
        print(nx, ny, b[2])
    # the fans are numbered by their first cells: the sensor at the lowest y first
    image, cost, pot = simulate(fans(), {}, pr.params(flags=1), (48, 32))
    labels, table, info = fr.frontiers_propagate(image, cost, pot, fr.params())
    assert info[2] == 3 and [int(labels[y, x]) for x, y in ((80, 8), (48, 32), (10, 40))] == [0, 1, 2]
    assert table["first_cell"].tolist() == sorted(table["first_cell"].tolist())
    # the obstacle splits the ray's frontier where the cost byte rises
    image, cost, pot = simulate(beside_an_obstacle(), {}, pr.params(flags=1), (36, 20))
    mid = int(cost[20, 35])
    assert 0 < mid <= 252 and cost[20, 45] == 0 and cost[20, 20] == 0
    assert [fr.frontiers_propagate(image, cost, pot, fr.params(max_cost=c))[2][2] for c in (252, mid, mid - 1, 0)] == [1, 1, 2, 2]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def info_tuple(i):
    return (i.n_frontier_cells, i.n_components, i.n_frontiers, i.n_written, i.best, i._pad, i.best_score)


def build(cm, scene, mq_kw={}, plan_flags=1, goal=None):
    """The scene's frames into a fresh map, the cost layer and the plan layer over it with the goal at the vehicle (or `goal`):
    the library's own (image, cost, pot)."""
    nx, ny, frames = scene
    tm.configure(cm, mr.params(CELL, nx, ny, **mq_kw))
    for frame in frames:
        tg.run_frame(cm, clouds_of(frame, nx, ny), tc.PARAMS)
        cm.map_integrate(None)
    cm.map_cost_configure(COST_Q["inscribed_radius"], COST_Q["inflation_radius"], COST_Q["cost_scaling"], False)
    cm.map_cost_update()
    cm.map_plan_configure(50, 205, bool(plan_flags))
    cm.map_plan_update(*centre_of(*(goal or goal_of(scene)), nx, ny))
    return cm.map_occupancy()[0], cm.map_cost()[0], cm.map_plan()[0]


def check(cm, tables, q, need=(), label=""):
    """Configure, update, read everything back and compare with the restatement of the library's own tables: the guards
    first, then the infos of every call, the labels, the table and both device tables."""
    image, cost, pot = tables
    ny, nx = image.shape
    want = fr.frontiers_propagate(image, cost, pot, q)
    assert same(want, fr.frontiers_flood(image, cost, pot, q)), label
    fr.guards(image, cost, pot, q, want, need)
    cm.map_frontier_configure(q["min_cells"], q["max_frontiers"], q["max_cost"], q["pot_scale"], q["gain_scale"])
    info = cm.map_frontier_update()
    table, i1 = cm.map_frontiers()
    labels, i2 = cm.map_frontier_labels()
    pl, pt, i3 = cm.map_frontier_device()
    print(f"{label}: {nx} x {ny} {q} -> {info_tuple(info)} want {want[2]}")
    assert info_tuple(info) == info_tuple(i1) == info_tuple(i2) == info_tuple(i3) == want[2], label
    assert labels.dtype == np.uint32 and labels.shape == (ny, nx)
    if labels.tobytes() != want[0].tobytes():
        bad = np.argwhere(labels != want[0])
        iy, ix = bad[0]
        raise AssertionError(f"{label}: labels differ in {len(bad)} of {labels.size} cells, first ({ix}, {iy}): got {labels[iy, ix]} want {want[0][iy, ix]}")
    assert table.dtype == fr.FRONTIER_DTYPE and len(table) == len(want[1])
    if table.tobytes() != want[1].tobytes():
        k = next(j for j in range(len(table)) if table[j] != want[1][j])
        raise AssertionError(f"{label}: the table differs, first in entry {k}: got {table[k]} want {want[1][k]}")
    dl, dt = np.zeros_like(labels), np.zeros_like(table)
    assert pl and pt
    assert tg.hip_rt().hipMemcpy(C.c_void_p(dl.ctypes.data), C.c_void_p(pl), C.c_size_t(dl.nbytes), 2) == 0
    if dt.nbytes:
        assert tg.hip_rt().hipMemcpy(C.c_void_p(dt.ctypes.data), C.c_void_p(pt), C.c_size_t(dt.nbytes), 2) == 0
    assert dl.tobytes() == want[0].tobytes() and dt.tobytes() == want[1].tobytes(), label
    return want


def merger():
    return capi.CloudMerger(max_points_total=4096, max_sensors=capi.MAX_SENSORS)


@pytest.mark.gpu
def test_an_all_unknown_image_has_no_frontier():
    nx, ny = 70, 40
    with merger() as cm:
        tm.configure(cm, mr.params(CELL, nx, ny))
        cm.map_cost_configure(COST_Q["inscribed_radius"], COST_Q["inflation_radius"], COST_Q["cost_scaling"], False)
        cm.map_cost_update()
        cm.map_plan_configure(50, 205, True)
        cm.map_plan_update(0.05, 0.05)
        tables = cm.map_occupancy()[0], cm.map_cost()[0], cm.map_plan()[0]
        assert (tables[0] == -1).all()
        want = check(cm, tables, fr.params(), need=("none",), label="all unknown")
        assert want[2] == (0, 0, 0, 0, NONE, 0, 0) and (want[0] == NONE).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rays_from_the_centre_on_every_shape(shape):
    nx, ny = shape
    with merger() as cm:
        tables = build(cm, generic(nx, ny), UNKNOWN_HITS)
        big = min(nx, ny) >= 33
        check(cm, tables, fr.params(), need=("all_three_values", "three_frontiers") if big else (), label="rays")
        check(cm, tables, fr.params(min_cells=3, max_frontiers=2, max_cost=100, pot_scale=7, gain_scale=3), label="rays, narrow")
        assert ((tables[0] == 0).any() and (tables[0] == 100).any()) == (nx * ny > 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["star", "corner", "zigzag", "fans", "behind_a_wall", "beside_an_obstacle"])
def test_designed_scenes(name):
    scene, mq, flags, q, need = CASES[name]
    with merger() as cm:
        tables = build(cm, scene, mq, flags)
        want = check(cm, tables, q, need, label=name)
        if name == "star":
            assert want[2][2] == 1
        if name == "fans":                             # the numbering follows first_cell: the sensor at the lowest y first
            assert want[2][2] == 3 and [int(want[0][y, x]) for x, y in ((80, 8), (48, 32), (10, 40))] == [0, 1, 2]


@pytest.mark.gpu
def test_min_cells_and_max_frontiers_at_their_edges():
    with merger() as cm:
        tables = build(cm, fans())
        base = check(cm, tables, fr.params(), need=("three_frontiers",), label="fans")
        n = int(base[1]["n_cells"].min())              # the smallest frontier: at, one below and one above its size
        assert (base[1]["n_cells"] == n).sum() == 1
        got = [check(cm, tables, fr.params(min_cells=m), label=f"min_cells {m}")[2][2] for m in (n, n - 1, n + 1)]
        assert got == [3, 3, 2]
        for cap in (3, 2, 4, 1):
            want = check(cm, tables, fr.params(max_frontiers=cap), label=f"max_frontiers {cap}")
            assert want[2][2] == 3 and want[2][3] == min(3, cap) and int(want[0][want[0] != NONE].max()) == 2       # the labels keep the higher numbers
        assert check(cm, tables, fr.params(min_cells=0xFFFFFFFF), label="min_cells at its largest")[2][2] == 0


@pytest.mark.gpu
def test_max_cost_splits_a_frontier():
    with merger() as cm:
        tables = build(cm, beside_an_obstacle(), goal=(36, 20))
        mid = int(tables[1][20, 35])
        assert 0 < mid <= 252
        got = [check(cm, tables, fr.params(max_cost=c), label=f"max_cost {c}")[2][2] for c in (252, mid, mid - 1, 0)]
        assert got == [1, 1, 2, 2]


@pytest.mark.gpu
def test_scale_extremes_do_not_wrap():
    top = 0xFFFFFFFF
    with merger() as cm:
        tables = build(cm, fans(), goal=(90, 60))      # a goal far from every fan: each min_pot is some thousands
        for ps, gs in ((0, 0), (top, 0), (0, top), (top, top), (1, top), (top, 1)):
            want = check(cm, tables, fr.params(pot_scale=ps, gain_scale=gs), need=("three_frontiers",), label=f"scales {ps} {gs}")
            assert want[2][4] != NONE and -(1 << 63) < want[2][6] <= fr.INT64_MAX and int(want[1]["min_pot"].min()) > 1000
        # a potential that makes pot_scale * min_pot pass INT64_MAX needs a window the tests do not use: the clamp itself is
        # the restatement's (test_the_score_does_not_wrap) and the kernel's arithmetic is the host program's (front_tests)


@pytest.mark.gpu
def test_a_three_frame_sequence_with_a_scroll_beside_a_context_without_the_layer():
    nx, ny, cell, poses = tc.SEQ
    inside = (0.0, 0.0, 0.0)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm, capi.CloudMerger(max_points_total=4096, max_sensors=1) as never:
        for c in (cm, never):
            tm.configure(c, tc.map_q(cell, nx, ny))
            c.map_cost_configure(COST_Q["inscribed_radius"], COST_Q["inflation_radius"], COST_Q["cost_scaling"], False)
            c.map_plan_configure(50, 205, True)
        cm.map_frontier_configure(2, 64, 200, 2, 1)
        q = fr.params(2, 64, 200, 2, 1)
        for k, xy in enumerate(poses):
            cells, _ = tc.seq_cells(k)
            outs = []
            for c in (cm, never):
                res = tg.run_frame(c, tc.frame_of(cells, cell, nx, ny, inside, xy), tc.PARAMS)
                outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), c.merged(4096).tobytes()))
            assert outs[0] == outs[1]                  # the frame behind the layer: that of a context that never had it
            infos = [c.map_integrate(tm.pose_t(xy[0], xy[1])) for c in (cm, never)]
            assert tm.info_tuple(infos[0]) == tm.info_tuple(infos[1])
            for c in (cm, never):
                c.map_cost_update()
                c.map_plan_update(float(xy[0]), float(xy[1]))       # exploration: the goal is the vehicle's position
            image, cost, pot = cm.map_occupancy()[0], cm.map_cost()[0], cm.map_plan()[0]
            want = fr.frontiers_propagate(image, cost, pot, q)
            fr.guards(image, cost, pot, q, want, ("all_three_values",))
            assert want[2][2] >= 1 and want[2][4] != NONE
            info = cm.map_frontier_update()
            assert info_tuple(info) == want[2] and cm.map_frontier_labels()[0].tobytes() == want[0].tobytes()
            assert cm.map_frontiers()[0].tobytes() == want[1].tobytes()
            assert cm.map()[0].tobytes() == never.map()[0].tobytes() and image.tobytes() == never.map_occupancy()[0].tobytes()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(cm.map_cost()[:2], never.map_cost()[:2]))
            assert pot.tobytes() == never.map_plan()[0].tobytes() and tm.info_tuple(cm.map()[1]) == tm.info_tuple(never.map()[1])


def layers(cm, nx, ny, cell=CELL, upto=3):
    tm.configure(cm, tc.map_q(cell, nx, ny))
    if upto >= 2:
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
    if upto >= 3:
        cm.map_plan_configure(50, 205, True)


@pytest.mark.gpu
def test_staleness_and_lifetime():
    nx, ny, cell = 64, 48, 0.1
    reads = lambda cm: (cm.map_frontiers, cm.map_frontier_labels, cm.map_frontier_device)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        layers(cm, nx, ny, upto=2)
        tm.refused(cm, cm.map_frontier_configure, text=b"cm_map_plan_configure")               # no plan layer
        cm.map_plan_configure(50, 205, True)
        cm.map_frontier_configure()
        L = cm._lib
        buf = np.full(nx * ny, 7, np.uint32)
        for call in reads(cm):
            tm.refused(cm, call, text=b"stale")
            tm.refused(cm, call, text=b"cm_map_frontier_configure")                            # ... which names the reason
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_plan_configure")                  # the plan layer itself is stale
        cm.map_cost_update()
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_cost_update")
        cm.map_plan_update(0.05, 0.05)
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_plan_update")
        info = cm.map_frontier_update()                # before any integration: all unknown
        assert info_tuple(info) == (0, 0, 0, 0, NONE, 0, 0) and (cm.map_frontier_labels()[0] == NONE).all()
        tg.run_frame(cm, tc.frame_of(tc.CORNERS_64_48, cell, nx, ny, (0.0, 0.0, 0.0)), tc.PARAMS)
        assert (cm.map_frontier_labels()[0] == NONE).all()                                     # a merge leaves the layer alone
        cm.map_integrate(None)
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_integrate")
        assert L.cm_map_frontier_labels_copy(cm._ctx, buf.ctypes.data, nx * ny, None) == capi.BAD_ARG and (buf == 7).all()
        tm.refused(cm, cm.map_frontier_update, text=b"stale")                                  # ... and so is the plan layer
        cm.map_cost_update()
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_cost_update")
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_cost_update")
        cm.map_plan_update(0.05, 0.05)
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_plan_update")
        info = cm.map_frontier_update()
        tables = cm.map_occupancy()[0], cm.map_cost()[0], cm.map_plan()[0]
        want = fr.frontiers_propagate(*tables, fr.params())
        assert info_tuple(info) == want[2] and info.n_frontiers >= 1 and cm.map_frontier_labels()[0].tobytes() == want[0].tobytes()
        cm.map_frontier_configure()                    # configure again: stale again
        tm.refused(cm, cm.map_frontiers, text=b"cm_map_frontier_configure")
        cm.map_frontier_update()
        # each configure call above it frees the layer
        cm.map_plan_configure(50, 205, True)
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_frontier_configure")
        cm.map_frontier_configure()
        cm.map_plan_configure(None)
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_plan_configure")
        cm.map_plan_configure(50, 205, True)
        cm.map_frontier_configure()
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_plan_configure")
        cm.map_plan_configure(50, 205, True)
        cm.map_frontier_configure()
        tm.configure(cm, tc.map_q(cell, nx, ny))
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_cost_configure")
        layers(cm, nx, ny)
        cm.map_frontier_configure()
        cm.map_configure(None)
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_configure")
        cm.map_frontier_configure(None)                # freeing what is not there is fine


@pytest.mark.gpu
def test_refusals_and_capacity():
    nx, ny = fans()[:2]
    with merger() as cm:
        L = cm._lib
        calls = (cm.map_frontiers, cm.map_frontier_labels, cm.map_frontier_device, cm.map_frontier_update)
        tm.refused(cm, cm.map_frontier_configure, text=b"cm_map_configure")                    # no map
        for call in calls:
            tm.refused(cm, call, text=b"cm_map_configure")
        layers(cm, nx, ny, upto=1)
        tm.refused(cm, cm.map_frontier_configure, text=b"cm_map_cost_configure")               # a map, no cost layer
        layers(cm, nx, ny, upto=2)
        assert fr.refusal(fr.params(), have_plan=False) == "plan"
        tm.refused(cm, cm.map_frontier_configure, text=b"cm_map_plan_configure")               # a cost layer, no plan layer
        cm.map_plan_configure(50, 205, True)
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_frontier_configure")              # a plan layer, no frontier layer
        ok = fr.params()
        for kw in REFUSED_PARAMS:                      # every refusal of the restatement's validator is the library's
            q = dict(ok, **kw)
            assert fr.refusal(q) is not None
            p = capi.FrontierParams(q["min_cells"], q["max_frontiers"], q["max_cost"], q["pot_scale"], q["gain_scale"])
            assert L.cm_map_frontier_configure(cm._ctx, C.byref(p)) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
        tm.refused(cm, cm.map_frontier_update, text=b"cm_map_frontier_configure")              # a refused call configured nothing
        for q in (ok, dict(ok, min_cells=0xFFFFFFFF), dict(ok, max_frontiers=1, max_cost=0), dict(ok, pot_scale=0xFFFFFFFF, gain_scale=0xFFFFFFFF)):
            assert fr.refusal(q) is None
            cm.map_frontier_configure(q["min_cells"], q["max_frontiers"], q["max_cost"], q["pot_scale"], q["gain_scale"])
        tables = build(cm, fans())
        want = check(cm, tables, fr.params(pot_scale=3, gain_scale=2), need=("three_frontiers",), label="fans")
        info = cm.map_frontier_update()
        # destinations that are too small: CM_CAPACITY, nothing copied, the info still written
        n = nx * ny
        buf = np.full(n, 7, np.uint32)
        for cap in (n - 1, 0):
            got = capi.FrontierInfo()
            assert L.cm_map_frontier_labels_copy(cm._ctx, buf.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (buf == 7).all()
            assert info_tuple(got) == info_tuple(info) == want[2]
        assert L.cm_map_frontier_labels_copy(cm._ctx, buf.ctypes.data, n + 5, None) == capi.OK and buf.tobytes() == want[0].tobytes()
        assert L.cm_map_frontier_labels_copy(cm._ctx, None, n, None) == capi.BAD_ARG           # no destination
        tab = np.zeros(8, fr.FRONTIER_DTYPE)
        tab["n_cells"] = 7
        for cap in (2, 0):
            got = capi.FrontierInfo()
            assert L.cm_map_frontier_copy(cm._ctx, tab.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (tab["n_cells"] == 7).all()
            assert info_tuple(got) == want[2]
        assert L.cm_map_frontier_copy(cm._ctx, tab.ctypes.data, 8, None) == capi.OK and tab[:3].tobytes() == want[1].tobytes()
        assert (tab["n_cells"][3:] == 7).all()
        assert L.cm_map_frontier_copy(cm._ctx, None, 8, None) == capi.BAD_ARG                  # no destination
        pl, pt = C.c_void_p(), C.c_void_p()
        assert L.cm_map_frontier_device(cm._ctx, C.byref(pl), C.byref(pt), None) == capi.OK and pl.value and pt.value
        assert L.cm_map_frontier_device(cm._ctx, None, None, None) == capi.OK
        # a frame in flight
        cm.submit_all(clouds_of(fans()[2][0], nx, ny))
        cm.merge_voxelize_async(capi.make_params(tc.PARAMS))
        assert fr.refusal(ok, in_flight=True) == "flight"
        for call in (cm.map_frontier_configure,) + calls:
            tm.refused(cm, call, text=b"flight")
        assert cm.wait().status == capi.OK
        assert cm.map_frontier_labels()[0].tobytes() == want[0].tobytes()                      # none of it touched the labels


@pytest.mark.gpu
def test_stage_names_under_profile():
    nx, ny = fans()[:2]
    with capi.CloudMerger(max_points_total=4096, max_sensors=capi.MAX_SENSORS, flags=capi.FLAG_PROFILE) as cm:
        build(cm, fans())
        cm.map_frontier_configure()
        assert not any("front" in n for n, _ in cm.stage_times())
        cm.map_frontier_update()
        assert [n for n, _ in cm.stage_times()] == STAGES and all(ms >= 0.0 for _, ms in cm.stage_times())
        tg.run_frame(cm, clouds_of(fans()[2][0], nx, ny), tc.PARAMS)       # a frame's own list never holds the call's stages
        assert not any("front" in n for n, _ in cm.stage_times())


# ---- no update allocates: the counts of the test build, as tests/test_ctx_memory.py takes them -------------------------------
def case_no_frontier_call_allocates():
    nx, ny, cell = 96, 64, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        layers(cm, nx, ny)
        before = capi.device_allocations()
        cm.map_frontier_configure(2, 64)               # every buffer of the layer is taken here:
        after = capi.device_allocations()
        assert [a - b for a, b in zip(after, before)] == [5, 5]        # the labels, the words, the table, its box, the page-locked words
        totals = []
        for k in range(4):
            if k:
                tg.run_frame(cm, tc.frame_of(tc.scattered(23 + k, nx, ny, 9), cell, nx, ny, (0.0, 0.0, 0.0)), tc.PARAMS)
                cm.map_integrate(tm.pose_t(0.0, 0.0))
            cm.map_cost_update()
            cm.map_plan_update(0.05, 0.05)
            b = capi.device_allocations()
            info = cm.map_frontier_update()            # (k = 0: the first one, before any integration)
            cm.map_frontiers()
            cm.map_frontier_labels()
            cm.map_frontier_device()
            a = capi.device_allocations()
            print(f"update {k}: before {b} after {a} frontiers {info.n_frontiers}")
            totals.append((b, a))
        assert all(b == a for b, a in totals), totals
        assert info.n_frontiers >= 1
        live = capi.device_allocations()[0]
        cm.map_frontier_configure(None)
        assert capi.device_allocations()[0] == live - 5
        cm.map_frontier_configure(2, 64)
        cm.map_plan_configure(None)                    # the plan layer takes the frontier layer with it
        assert capi.device_allocations()[0] == live - 5 - 4


@pytest.mark.gpu
def test_no_frontier_update_allocates():
    assert os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")), "the test build is missing"
    env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK")}
    env.update(CM_LIB_VARIANT="testhooks", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_map_frontier", "no_frontier_call_allocates"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    {"no_frontier_call_allocates": case_no_frontier_call_allocates}[sys.argv[1]]()
