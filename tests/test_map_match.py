"""Correlative scan matching of a frame against the occupancy map: cm_map_match_configure, cm_map_match_evaluate,
cm_map_match_copy, cm_map_match_device, cm_map_match_table_copy, cm_match_table (include/cloudmerge.h, cm_kernels_match.hip,
DESIGN.md §26).

The bar on the GPU: every byte of the score volume, of the device-pointer variant and of the result equal to the restatement
(tests/match_ref.py) fed with the library's own merged(), map_cost() distance field and traj_directions(). There is no
tolerance. The scenes are designed as in tests/test_map_plan.py: one point of A per wanted window cell, at the cell's centre,
both sensors outside the window (no rays: the image holds hits and unknown cells only). Every scene is first computed on the
CPU alone, from cost_ref's distance field of the wanted image and the points the frame is built from: there its hand-worked
answers are asserted, so the geometry is chosen before a device byte is looked at; on the GPU the same answers are asserted
again on the restatement of the library's tables, then the bytes are compared."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import cost_ref as cr
from tests import map_ref as mr
from tests import match_ref as mf
from tests import motion_edge_frames as ef
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_map_cost as tc
from tests import test_occupancy_map as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
NAMES = ("cm_map_match_configure", "cm_map_match_evaluate", "cm_map_match_copy", "cm_map_match_device", "cm_map_match_table_copy", "cm_match_table")
MATCH_TYPES = (capi.MatchParams, capi.MatchResult)   # (a library without the layer fails every test here, at import)
TILE = tr.device_define("CM_MATCH_TILE")
F32 = np.float32
CELL = 0.1
NX, NY = 96, 80                                      # not a multiple of 32 in y, three bitmap words per row
TRANS = [(200.0, 0.0, 0.0), (200.0, 7.0, 0.0)]       # both sensors far outside every window below: no rays
SHARP = dict(sigma=0.1, max_dist=0.05)               # R = 1 and lut[1] = 0: the field is 255 on hit cells and 0 elsewhere


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_match_structs_and_constants_match_header(tmp_path):
    structs = {"cm_match_params": (capi.MatchParams, ["sigma", "max_dist", "n_a", "a_stride", "wx", "wy", "flags"]),
               "cm_match_result": (capi.MatchResult, ["best", "k", "i", "j", "score", "n_cells", "max_score", "yaw", "sub", "pose"])}
    names = ["CM_MATCH_MAX_RADIUS_CELLS", "CM_MATCH_MAX_SHIFT", "CM_MATCH_MAX_ANGLES", "CM_MATCH_MAX_CANDIDATES", "CM_MATCH_SUBCELL"]
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
    assert got[:len(want)] == want == [28, 0, 4, 8, 12, 16, 20, 24, 96, 0, 4, 8, 12, 16, 20, 24, 28, 32, 48]
    assert got[len(want):] == [capi.MATCH_MAX_RADIUS_CELLS, capi.MATCH_MAX_SHIFT, capi.MATCH_MAX_ANGLES, capi.MATCH_MAX_CANDIDATES, capi.MATCH_SUBCELL]
    assert got[len(want):] == [mf.MAX_RADIUS_CELLS, mf.MAX_SHIFT, mf.MAX_ANGLES, mf.MAX_CANDIDATES, mf.SUBCELL] == [64, 64, 127, 1 << 22, 1]
    assert TILE >= 8 and (TILE + 2 * 64) ** 2 + 2 * TILE * TILE <= 160 * 1024       # the staged field and the cell list fit the LDS
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.MatchParams(0.1, 0.3, 1, 1, 1, 1, 0)
    pose = np.eye(3, 4, dtype=F32)
    res = capi.MatchResult()
    before = bytes(res)
    buf = np.full(27, 7, np.uint32)
    lut = np.full(17, 7, np.uint8)
    n = C.c_uint64(99)
    a = C.c_void_p(5)
    assert L.cm_map_match_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_match_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_match_evaluate(None, pose.ctypes.data, C.byref(res)) == capi.BAD_ARG
    assert L.cm_map_match_copy(None, buf.ctypes.data, 27, C.byref(res)) == capi.BAD_ARG
    assert L.cm_map_match_device(None, C.byref(a), C.byref(res)) == capi.BAD_ARG
    assert L.cm_map_match_table_copy(None, lut.ctypes.data, 17, C.byref(n)) == capi.BAD_ARG
    assert (buf == 7).all() and (lut == 7).all() and bytes(res) == before and a.value == 5 and n.value == 99


TABLES = [(0.1, 0.1, 0.3), (0.1, 0.25, 1.0), (0.5, 0.3, 32.0), (0.05, 0.02, 0.3), (0.1, 0.1, 0.05), (0.1, 3.0, 6.4), (0.25, 1e-3, 1.0),
          (0.1, 1e-30, 0.3), (0.1, 1e30, 0.3)]


@pytest.mark.parametrize("cell,sigma,max_dist", TABLES)
def test_the_field_table_against_the_restatement(cell, sigma, max_dist):
    got, want = capi.match_table(cell, sigma, max_dist), mf.table(cell, sigma, max_dist)
    R = mf.radius(cell, max_dist)
    assert got.dtype == np.uint8 and len(got) == R * R + 1 and got.tobytes() == want.tobytes() and got[0] == 255
    m = np.sqrt(np.arange(len(got), dtype=np.float64)) * float(F32(cell))
    assert (got[m > float(F32(max_dist))] == 0).all()                  # the cut at max_dist
    assert (np.diff(got.astype(int)) <= 0).all()                       # a likelihood falls with the distance


def test_the_field_table_by_hand_and_its_refusals():
    t = capi.match_table(0.1, 0.1, 0.3)
    # 0.3f / 0.1f is a little above 3 in double: R = 4, 17 entries; exp(-d2 / 2) * 255 floored; d2 = 9 is still within max_dist
    assert t.tolist() == [255, 154, 93, 56, 34, 20, 12, 7, 4, 2] + [0] * 7
    assert [int(math.floor(255.0 * math.exp(-d2 / 2.0))) for d2 in range(1, 10)] == t[1:10].tolist()
    assert capi.match_table(*((0.1,) + tuple(SHARP.values()))).tolist() == [255, 0]
    L = capi.load()
    buf = np.full(20, 7, np.uint8)
    n = C.c_uint64(99)
    assert L.cm_match_table(0.1, 0.1, 0.3, buf.ctypes.data, 16, C.byref(n)) == capi.CAPACITY and n.value == 17 and (buf == 7).all()
    assert L.cm_match_table(0.1, 0.1, 0.3, buf.ctypes.data, 0, None) == capi.CAPACITY and (buf == 7).all()
    n = C.c_uint64(99)
    for bad in [(0.0, 0.1, 0.3), (-0.1, 0.1, 0.3), (np.nan, 0.1, 0.3), (np.inf, 0.1, 0.3), (0.1, 0.0, 0.3), (0.1, -1.0, 0.3), (0.1, np.nan, 0.3),
                (0.1, np.inf, 0.3), (0.1, 0.1, 0.0), (0.1, 0.1, -0.3), (0.1, 0.1, np.nan), (0.1, 0.1, np.inf), (0.1, 0.1, 6.5), (1e-30, 0.1, 0.3)]:
        assert L.cm_match_table(*bad, buf.ctypes.data, 20, C.byref(n)) == capi.BAD_ARG and n.value == 99 and (buf == 7).all(), bad
    assert L.cm_match_table(0.1, 0.1, 0.3, None, 20, C.byref(n)) == capi.BAD_ARG and n.value == 99
    assert L.cm_match_table(0.1, 0.1, 0.3, buf.ctypes.data, 17, None) == capi.OK and buf[:17].tobytes() == t.tobytes() and (buf[17:] == 7).all()
    assert len(capi.match_table(0.1, 0.1, 6.4)) == 64 * 64 + 1        # the largest table


def test_refusals_of_the_restatement():
    ok = mf.params()
    assert mf.refusal(ok, CELL) is None
    for kw in REFUSED_PARAMS:
        assert mf.refusal(dict(ok, **kw), CELL) is not None, kw
    for kw in ACCEPTED_PARAMS:
        assert mf.refusal(dict(ok, **kw), CELL) is None, kw


REFUSED_PARAMS = [dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=np.nan), dict(sigma=np.inf), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=np.nan),
                  dict(max_dist=np.inf), dict(max_dist=6.5), dict(n_a=128), dict(a_stride=0), dict(n_a=127, a_stride=9), dict(n_a=2, a_stride=513),
                  dict(wx=65), dict(wy=65), dict(n_a=126, a_stride=8, wx=64, wy=64), dict(flags=2), dict(flags=3), dict(flags=1 << 31)]
ACCEPTED_PARAMS = [dict(max_dist=6.4), dict(n_a=0), dict(n_a=127, a_stride=8), dict(n_a=2, a_stride=512), dict(n_a=1, a_stride=1024), dict(wx=64, wy=0),
                   dict(wx=0, wy=64), dict(n_a=125, a_stride=8, wx=64, wy=64), dict(flags=1)]


# ---- the scenes ----------------------------------------------------------------------------------------------------------
def anchor_of(nx, ny):
    return (-(nx // 2), -(ny // 2))                # the vehicle of the map's frame stands at the world's origin


def parts_of(cells_by_sensor, nx, ny, extra=()):
    """Per sensor the (n, 3) vehicle-frame points: the centre of every wanted window cell (the vehicle at the world's origin, the
    pose the identity), then the extra points of that sensor. A sensor without a point gets one far outside the window."""
    ax, ay = anchor_of(nx, ny)
    out = []
    for s, cells in enumerate(cells_by_sensor):
        c = np.asarray(cells, np.float64).reshape(-1, 2)
        p = np.stack([(ax + c[:, 0] + 0.5) * CELL, (ay + c[:, 1] + 0.5) * CELL, np.zeros(len(c))], axis=1)
        e = np.asarray(extra[s] if s < len(extra) else [], np.float64).reshape(-1, 3)
        p = np.concatenate([p, e])
        if len(p) == 0:
            p = np.array([[(ax + nx + 40.5) * CELL, 0.0, 0.0]])
        out.append(p)
    return out


def clouds_of(parts):
    """The sensors' clouds, and the cloud A the frame makes of them under the pure translations: fp32 p + t per component."""
    sensors, A = [], []
    for s, p in enumerate(parts):
        q = (p - np.asarray(TRANS[s], np.float64)).astype(F32)
        sensors.append(xyzi_cloud(q, np.full(len(q), s, F32), t_xyz=TRANS[s]))
        A.append(np.concatenate([(q + F32(TRANS[s])[None, :]).astype(F32), np.full((len(q), 1), s, F32)], axis=1))
    return sensors, np.concatenate(A)


def image_of(cells_by_sensor, nx, ny):
    img = np.full((ny, nx), -1, np.int8)
    for cells in cells_by_sensor:
        for x, y in cells:
            img[y, x] = 100
    return img


def rotated(P, entries, tab):
    """P's rows 0 and 1 rotated by a number of heading-table entries about z through the vehicle (the prior of a recovery)."""
    c, s = F32(tab[entries & 4095, 0]), F32(tab[entries & 4095, 1])
    return np.stack([F32(c) * P[0, :3] - F32(s) * P[1, :3], F32(s) * P[0, :3] + F32(c) * P[1, :3]]).astype(F32)


def scene(name, map_cells, scan_cells=None, nx=NX, ny=NY, q=None, prior=None, turn=0, mq=None, map_extra=(), scan_extra=(), expect=None, check=None):
    """map_cells / scan_cells: per sensor the window cells of the frame that is integrated under the identity and of the frame
    that is matched (None: the same frame, matched after its integration). prior: (tx, ty) of the prior; turn: heading-table
    entries it is rotated by. expect: fields of the result. check: a function of (volume, result, scene) with further asserts."""
    return dict(name=name, map_cells=map_cells, scan_cells=scan_cells, nx=nx, ny=ny, q=dict(mf.params(), **(q or {})), prior=prior or (0.0, 0.0),
                turn=turn, mq=mr.params(CELL, nx, ny, **(mq or {})), map_extra=map_extra, scan_extra=scan_extra, expect=expect or {}, check=check)


def prior_of(sc, tab):
    P = tm.pose_t(*sc["prior"])
    if sc["turn"]:
        P[:2, :3] = rotated(P, sc["turn"], tab)
    return P


def spread(seed, nx, ny, n, margin):
    rng = np.random.default_rng(seed)
    return sorted(set(zip(rng.integers(margin, nx - margin, n).tolist(), rng.integers(margin, ny - margin, n).tolist())))


BASE = [spread(3, NX, NY, 20, 6), spread(4, NX, NY, 16, 6) + [(20, 20)]]
BASE[0] = BASE[0] + [(20, 20)]                       # both sensors hit (20, 20): counted once
N_BASE = len(set(BASE[0]) | set(BASE[1]))
CENTRE = (2 * 5 + 2) * 7 + 3                         # the prior's entry at n_a = 2, wy = 2, wx = 3


def scan_of(sc):
    """(clouds, A) of the frame that is matched."""
    own = sc["scan_cells"] is not None
    return clouds_of(parts_of(sc["scan_cells"] if own else sc["map_cells"], sc["nx"], sc["ny"], sc["scan_extra"] if own else sc["map_extra"]))


def hits_back(vol, res, sc):
    """The returned pose reproduces the map's hit cells."""
    _, A = scan_of(sc)
    got = mf.cells_of(A, res["pose"][:2, :3], (res["pose"][0, 3], res["pose"][1, 3]), sc["mq"], anchor_of(sc["nx"], sc["ny"]))
    want = sorted({x + y * sc["nx"] for cells in sc["map_cells"] for x, y in cells})
    assert got.tolist() == want


def one_k_only(vol, res, sc):
    """A point leaves the window under some candidates only; the rest of the frame stays."""
    n = [len(d) for d in res["D"]]
    assert max(n) == n[sc["q"]["n_a"]] == len(set(sc["map_cells"][0]) | set(sc["map_cells"][1])) and min(n) < max(n), n


def shifts_leave(vol, res, sc):
    """With hit cells in the first and last row and column every shift but (0, 0) loses cells to the outside."""
    n_a, wx, wy = sc["q"]["n_a"], sc["q"]["wx"], sc["q"]["wy"]
    assert vol[n_a, wy, wx] == res["max_score"] and (np.delete(vol[n_a].reshape(-1), wy * (2 * wx + 1) + wx) < res["max_score"]).all()


EDGE_CELLS = [[(0, 0), (95, 0), (0, 79), (95, 79), (0, 40), (48, 0)], [(95, 41), (47, 79), (31, 31), (32, 32), (63, 40), (64, 40)]]
WORDS_70 = [[(31, 0), (32, 0), (69, 0), (0, 1), (25, 1), (26, 1)], [(31, 31), (32, 31), (31, 32), (32, 32), (63, 44), (64, 44), (69, 44), (0, 44)]]
# 70-cell rows: cell index 31 | 32 is a word edge in row 0, 95 | 96 = (25, 1) | (26, 1) in row 1; x = 31 | 32 and 63 | 64 are tile edges


def scenes():
    out = []
    # identity: the frame against the map it made
    out.append(scene("identity", BASE, expect=dict(k=0, i=0, j=0, best=CENTRE, n_cells=N_BASE, score=255 * N_BASE, max_score=255 * N_BASE)))
    # recovery: the prior two cells to the left, one up, turned right by a_stride entries (32 of them: 2.8 degrees move a point
    # a metre away by half a cell, so that the angle shows in the cells)
    out.append(scene("recovery", BASE, prior=(-2 * CELL, 1 * CELL), turn=-32, q=dict(a_stride=32), check=hits_back,
                     expect=dict(k=1, i=2, j=-1, n_cells=N_BASE, score=255 * N_BASE, max_score=255 * N_BASE)))
    out.append(scene("recovery, sub-cell on", BASE, prior=(-2 * CELL, 1 * CELL), turn=-32, q=dict(a_stride=32, flags=1), check=hits_back,
                     expect=dict(k=1, i=2, j=-1, score=255 * N_BASE, sub=(0.0, 0.0))))
    # edges: hit cells in the first and last row and column
    out.append(scene("edges", EDGE_CELLS, check=shifts_leave, expect=dict(k=0, i=0, j=0, n_cells=12, score=255 * 12)))
    # (95, 79) is 4.75 m and 3.95 m from the vehicle: a turn to the left lifts it over the window's upper edge at 4.0 m
    out.append(scene("a point that leaves under one k", [[(95, 79), (50, 50)], [(40, 30)]], q=dict(a_stride=16), check=one_k_only, expect=dict(k=0, i=0, j=0, n_cells=3)))
    # a point above the height band is in A and is not counted; two sensors in one cell count once
    out.append(scene("out of band", [[(30, 30), (60, 50)], [(30, 30)]], mq=dict(z_band=(-0.5, 1.0)), map_extra=([(1.05, 1.05, 1.5)], [(-2.05, 1.05, -0.75)]),
                     expect=dict(k=0, i=0, j=0, n_cells=2, score=510, max_score=510)))
    # tiles and bitmap words
    out.append(scene("tile and word edges, 70 x 45", WORDS_70, nx=70, ny=45, expect=dict(k=0, i=0, j=0, n_cells=14, score=255 * 14)))
    out.append(scene("a window smaller than the halo", [[(0, 0), (7, 7)], [(3, 4)]], nx=8, ny=8, q=dict(wx=64, wy=64, n_a=1), expect=dict(k=0, i=0, j=0, n_cells=3, score=765)))
    # ties. An empty map: the prior, score 0
    out.append(scene("empty map", [[], []], scan_cells=BASE, expect=dict(k=0, i=0, j=0, best=CENTRE, score=0, n_cells=N_BASE)))
    out.append(scene("empty map, sub-cell on: flat", [[], []], scan_cells=BASE, q=dict(flags=1), expect=dict(k=0, i=0, j=0, score=0, sub=(0.0, 0.0))))
    # two shifts tie at 255: i = -3 has the lower index, i = +1 the smaller i * i + j * j
    out.append(scene("two shifts tie", [[(39, 40)], [(43, 40)]], scan_cells=[[(42, 40)], []], q=SHARP, expect=dict(k=0, i=1, j=0, score=255, n_cells=1)))
    # two angles tie: the point 4.0748 m ahead moves one row per candidate (a_stride 16: 0.1 m per step); k = -2 and k = +1 hit
    out.append(scene("two angles tie", [[(88, 38)], [(88, 41)]], scan_cells=[[], []], scan_extra=([(4.0748, 0.05, 0.0)], []), q=dict(SHARP, a_stride=16),
                     expect=dict(k=1, i=0, j=0, score=255, n_cells=1)))
    # sub-cell: two scan cells; to their right one has a hit cell (255), the other a neighbour at d2 = 1 (154); to the left both 154
    out.append(scene("sub-cell by hand", [[(40, 40), (50, 40)], [(41, 40)]], scan_cells=[[(40, 40)], [(50, 40)]], q=dict(flags=1),
                     expect=dict(k=0, i=0, j=0, score=510, n_cells=2, sub=(0.5 * (308.0 - 409.0) / (308.0 - 1020.0 + 409.0), 0.0))))
    out.append(scene("the same without the flag", [[(40, 40), (50, 40)], [(41, 40)]], scan_cells=[[(40, 40)], [(50, 40)]], expect=dict(score=510, sub=(0.0, 0.0))))
    # the best entry on the search window's edge: no neighbour beyond it, sub = 0 although the scores fall towards the inside
    out.append(scene("sub-cell at the window's edge", [[(43, 40)], []], scan_cells=[[(40, 40)], []], q=dict(flags=1), expect=dict(k=0, i=3, j=0, score=255, sub=(0.0, 0.0))))
    # caps: every angle candidate once
    out.append(scene("255 angles on 16 x 16", [[(2, 3), (12, 9)], [(8, 8)]], nx=16, ny=16, q=dict(n_a=127, a_stride=8), expect=dict(k=0, i=0, j=0, score=765)))
    # a denser frame over several tiles, a wider search
    out.append(scene("dense", [spread(11, NX, NY, 400, 12), spread(12, NX, NY, 300, 12)], q=dict(n_a=3, a_stride=24, wx=9, wy=8, sigma=0.15, max_dist=0.5),
                     prior=(3 * CELL, -4 * CELL), turn=48, expect=dict(k=-2, i=-3, j=4)))
    return out


SCENES = scenes()


def result_dict(r):
    return dict(best=r.best, k=r.k, i=r.i, j=r.j, score=r.score, n_cells=r.n_cells, max_score=r.max_score, yaw=F32(r.yaw), sub=(r.sub[0], r.sub[1]),
                pose=np.array(list(r.pose), F32).reshape(3, 4))


def check_expectations(sc, vol, res):
    q = sc["q"]
    assert vol.shape == (2 * q["n_a"] + 1, 2 * q["wy"] + 1, 2 * q["wx"] + 1) and vol.dtype == np.uint32
    for f, v in sc["expect"].items():
        assert res[f] == v, (sc["name"], f, res[f], v)
    assert res["score"] == vol.max() and res["max_score"] == 255 * res["n_cells"] and res["score"] <= res["max_score"]
    assert abs(float(res["yaw"]) - res["k"] * q["a_stride"] * 2 * math.pi / 4096) < 1e-6 and (res["pose"][2] == prior_of(sc, TAB())[2]).all()
    if sc["check"]:
        sc["check"](vol, res, sc)


_tab = []


def TAB():
    if not _tab:
        _tab.append(capi.traj_directions())
    return _tab[0]


@pytest.mark.parametrize("sc", SCENES, ids=lambda s: s["name"])
def test_every_scene_on_the_restatement_alone(sc):
    """No GPU: the image the map's frame makes (hits and unknown cells), cost_ref's distance field of it, the points of the frame."""
    dist2 = cr.dist2_separable(image_of(sc["map_cells"], sc["nx"], sc["ny"]))
    assert (dist2 == cr.dist2_brute(image_of(sc["map_cells"], sc["nx"], sc["ny"]))).all()
    _, A = scan_of(sc)
    vol, res = mf.match(A, dist2, sc["mq"], anchor_of(sc["nx"], sc["ny"]), sc["q"], prior_of(sc, TAB()), TAB())
    check_expectations(sc, vol, res)


def test_the_best_entry_of_hand_made_volumes():
    q = mf.params(n_a=1, wx=1, wy=1)
    vol = np.zeros((3, 3, 3), np.uint32)
    assert mf.best_of(vol, q) == 13                                    # all equal: the centre
    vol[0, 0, 0] = vol[2, 2, 2] = 5
    assert mf.best_of(vol, q) == 0                                     # the same d2 and |k|: the lower index
    vol[1, 0, 0] = 5
    assert mf.best_of(vol, q) == 9                                     # the smaller |k|
    vol[0, 1, 2] = 5
    assert mf.best_of(vol, q) == 5                                     # the smaller d2 before the smaller |k|
    vol[2, 2, 2] = 6
    assert mf.best_of(vol, q) == 26                                    # the score before everything
    assert mf.sub_of(308, 510, 409) == 101.0 / 606.0 and mf.sub_of(None, 5, 3) == 0.0 and mf.sub_of(5, 5, 5) == 0.0 and mf.sub_of(0, 1, 9) == 0.0
    assert mf.sub_of(0, 10, 10) == 0.5 and mf.sub_of(10, 10, 0) == -0.5 and mf.sub_of(9, 10, 10) == 0.5


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def same_result(got, want):
    return all(got[f] == want[f] for f in ("best", "k", "i", "j", "score", "n_cells", "max_score", "sub")) and \
        F32(got["yaw"]).tobytes() == F32(want["yaw"]).tobytes() and got["pose"].tobytes() == want["pose"].tobytes()


def configure_match(cm, q):
    cm.map_match_configure(q["sigma"], q["max_dist"], q["n_a"], q["a_stride"], q["wx"], q["wy"], bool(q["flags"] & 1))


def build_map(cm, sc):
    tm.configure(cm, sc["mq"])
    sensors, _ = clouds_of(parts_of(sc["map_cells"], sc["nx"], sc["ny"], sc["map_extra"]))
    tg.run_frame(cm, sensors, tc.PARAMS)
    minfo = cm.map_integrate(None)
    assert tuple(minfo.anchor) == anchor_of(sc["nx"], sc["ny"])
    cm.map_cost_configure(0.0, 0.3, 3.0, False)
    cm.map_cost_update()
    assert ((cm.map_occupancy()[0] == 100) == (image_of(sc["map_cells"], sc["nx"], sc["ny"]) == 100)).all()


def evaluate(cm, sc, n_cap=4096):
    """Configure the layer, match, read everything back and compare with the restatement of the library's own tables."""
    if sc["scan_cells"] is not None:
        tg.run_frame(cm, scan_of(sc)[0], tc.PARAMS)
    A = tg.host_clouds(cm, n_cap, False)[0]
    _, dist2, minfo = cm.map_cost()
    prior = prior_of(sc, TAB())
    want_vol, want = mf.match(A, dist2, sc["mq"], tuple(minfo.anchor), sc["q"], prior, TAB())
    check_expectations(sc, want_vol, want)
    configure_match(cm, sc["q"])
    assert cm.map_match_table().tobytes() == mf.table(CELL, sc["q"]["sigma"], sc["q"]["max_dist"]).tobytes()
    res = cm.map_match(prior)
    vol, r1 = cm.map_match_scores()
    ptr, r2 = cm.map_match_device()
    got = result_dict(res)
    print(f"{sc['name']}: best {got['best']} (k, i, j) = ({got['k']}, {got['i']}, {got['j']}) score {got['score']} of {got['max_score']} sub {got['sub']}")
    assert bytes(res) == bytes(r1) == bytes(r2)
    assert vol.shape == want_vol.shape and vol.dtype == want_vol.dtype
    if vol.tobytes() != want_vol.tobytes():
        bad = np.argwhere(vol != want_vol)
        raise AssertionError(f"{sc['name']}: {len(bad)} of {vol.size} entries differ, first {bad[0]}: got {vol[tuple(bad[0])]} want {want_vol[tuple(bad[0])]}")
    dev = np.zeros_like(vol)
    assert ptr and tg.hip_rt().hipMemcpy(C.c_void_p(dev.ctypes.data), C.c_void_p(ptr), C.c_size_t(vol.nbytes), 2) == 0
    assert dev.tobytes() == want_vol.tobytes(), sc["name"]
    assert same_result(got, want), (sc["name"], got, {k: v for k, v in want.items() if k not in ("D", "L")})
    return vol, res


def groups():
    """Scenes that share a map run behind one another on one context."""
    out = {}
    for sc in SCENES:
        key = (sc["nx"], sc["ny"], repr(sc["map_cells"]), repr(sc["map_extra"]), repr(sorted(sc["mq"].items())))
        out.setdefault(key, []).append(sc)
    return list(out.values())


@pytest.mark.gpu
@pytest.mark.parametrize("group", groups(), ids=lambda g: g[0]["name"])
def test_every_scene_against_the_restatement(group):
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm:
        build_map(cm, group[0])
        for sc in group:
            evaluate(cm, sc)


@pytest.mark.gpu
def test_with_ground_removal():
    """tests/test_grid_map.py's ground scene: the plane's points are in G, not in A, and must not be counted; the boxes are."""
    parts = tg.ground_scene(31)
    n_cap = sum(len(p) for p in parts)
    q = mf.params(sigma=0.5, max_dist=1.5, n_a=2, a_stride=4, wx=3, wy=2, flags=1)
    mq = mr.params(0.5, 320, 24)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params([tg.FRONT, tg.FRONT]))
        tm.configure(cm, mq)
        tg.run_frame(cm, tg.clouds_of(parts), MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=1, **tg.ROI))
        A, G = tg.host_clouds(cm, n_cap, True)
        assert len(G) > n_cap // 2 and len(A) > 500
        minfo = cm.map_integrate(None)
        cm.map_cost_configure(0.0, 1.0, 3.0, False)
        cm.map_cost_update()
        configure_match(cm, q)
        prior = tm.pose_t(1.0, -0.5)                                   # two cells right, one down
        want_vol, want = mf.match(A, cm.map_cost()[1], mq, tuple(minfo.anchor), q, prior, TAB())
        with_g, _ = mf.match(np.concatenate([A, G]), cm.map_cost()[1], mq, tuple(minfo.anchor), q, prior, TAB())
        assert (with_g != want_vol).any()                              # counting G would show
        res = cm.map_match(prior)
        vol, _ = cm.map_match_scores()
        assert vol.tobytes() == want_vol.tobytes() and same_result(result_dict(res), want)
        assert (res.k, res.i, res.j) == (0, -2, 1) and res.score == res.max_score


# A moving vehicle: 7.2 m/s and a slow turn. Sensor 0's points carry a time over 0.1 s behind a stamp 50 ms after the
# reference instant, sensor 1's are all at its stamp 80 ms before it: every point moves by 3 to 11 cells of 0.1 m.
DESKEW = dict(v=(6.0, -4.0, 0.0), w=(0.0, 0.0, 0.05), t_ref=1_700_000_000_000_000_000, d_stamp=(50_000_000, -80_000_000), kinds=("velo22", "xyzi16"))


def deskew_raws(parts):
    """Per sensor the vehicle-frame points `parts` as a raw cloud under its translation (tests/motion_edge_frames.py's Cloud):
    velo22 with float32 seconds at byte 18 for sensor 0, XYZI16 without a time field for sensor 1; and the two stamps."""
    rng = np.random.default_rng(5)
    raws = []
    for s, p in enumerate(parts):
        q = (np.asarray(p, np.float64) - np.asarray(TRANS[s], np.float64)).astype(F32)
        tau = np.sort(rng.uniform(0.0, 0.1, len(q))).astype(F32) if s == 0 else None
        raws.append(ef.Cloud(DESKEW["kinds"][s], q, tau, np.full(len(q), s, F32), t=TRANS[s], seed=s))
    return raws, [DESKEW["t_ref"] + d for d in DESKEW["d_stamp"]]


def run_deskewed(cm, raws, stamps, n_cap=4096):
    """The frame of the raw clouds with compensation on. Returns the library's A and, per sensor, the numpy-compensated cloud
    (tests/motion_ref.py) as XYZI16 with the identity transform: what a context without motion is fed."""
    v, w, t_ref = DESKEW["v"], DESKEW["w"], DESKEW["t_ref"]
    for s, r in enumerate(raws):
        cm.set_transform(s, r.q, r.t)
        cm.set_time_field(s, *r.time)
        cm.submit(s, r.cloud)
    cm.set_ego_motion(capi.make_motion(v, w, t_ref, stamps))
    res = cm.merge_voxelize(tc.PARAMS)
    assert res.status == capi.OK and res.path_flags & capi.PATH_MOTION
    want = [r.compensated(cm.get_matrix(s), stamps[s], t_ref, v, w) for s, r in enumerate(raws)]
    A = tg.host_clouds(cm, n_cap, False)[0]
    assert A.tobytes() == np.concatenate(want).tobytes()
    return A, [xyzi_cloud(c[:, :3], c[:, 3]) for c in want]


def moved_by_cells(A, A0):
    """The compensated cloud against the uncompensated one: (smallest, largest) displacement of a point in cells."""
    assert A.shape == A0.shape and np.array_equal(A[:, 3], A0[:, 3])
    d = np.hypot(A[:, 0] - A0[:, 0], A[:, 1] - A0[:, 1]) / CELL
    return float(d.min()), float(d.max())


@pytest.mark.gpu
def test_with_deskew():
    """k_match_mark reads the frame's clouds in place: under motion those are the compensated records of the pre-pass. The
    identity scene's map, then its frame from a moving vehicle: the volume and the result are the restatement's on the
    library's merged(), and the bytes a context without motion gives on the numpy-compensated clouds."""
    sc = scene("deskew", BASE, q=dict(n_a=2, a_stride=16, wx=6, wy=5, flags=1))
    raws, stamps = deskew_raws(parts_of(sc["map_cells"], sc["nx"], sc["ny"]))
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm, capi.CloudMerger(max_points_total=4096, max_sensors=2) as plain:
        build_map(cm, sc)
        build_map(plain, sc)
        A, comp = run_deskewed(cm, raws, stamps)
        lo, hi = moved_by_cells(A, scan_of(sc)[1])
        assert lo > 3.0 and hi < 12.0, (lo, hi)                        # the points did move, by several cells
        vol, res = evaluate(cm, sc)
        assert 0 < res.n_cells <= len(A)
        tg.run_frame(plain, comp, tc.PARAMS)
        assert tg.host_clouds(plain, 4096, False)[0].tobytes() == A.tobytes()
        p_vol, p_res = evaluate(plain, sc)
        assert vol.tobytes() == p_vol.tobytes() and bytes(res) == bytes(p_res)
        unmoved = mf.match(scan_of(sc)[1], cm.map_cost()[1], sc["mq"], anchor_of(sc["nx"], sc["ny"]), sc["q"], prior_of(sc, TAB()), TAB())[0]
        assert unmoved.tobytes() != vol.tobytes()                      # matching the raw clouds would show


def small_stack(cm, nx=64, ny=48, cell=0.1, match=True):
    tm.configure(cm, tc.map_q(cell, nx, ny))
    cm.map_cost_configure(0.35, 1.05, 3.0, True)
    if match:
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)


@pytest.mark.gpu
def test_staleness_and_lifetime():
    nx, ny, cell = 64, 48, 0.1
    I = np.eye(3, 4, dtype=F32)
    frame = lambda cm: tg.run_frame(cm, tc.frame_of(tc.CORNERS_64_48, cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.refused(cm, cm.map_match_configure, 0.1, 0.3, text=b"cm_map_configure")
        tm.configure(cm, tc.map_q(cell, nx, ny))
        tm.refused(cm, cm.map_match_configure, 0.1, 0.3, text=b"cm_map_cost_configure")         # no cost layer
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        for call in (cm.map_match_scores, cm.map_match_device, cm.map_match_table, lambda: cm.map_match(I)):
            tm.refused(cm, call, text=b"cm_map_match_configure")                                 # no matching layer
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
        assert cm.map_match_table().tobytes() == mf.table(cell, 0.1, 0.3).tobytes()              # (the table is not stale: it is the configure call's)
        L = cm._lib
        buf = np.full(75, 7, np.uint32)
        for call in (cm.map_match_scores, cm.map_match_device):                                  # copy before evaluate
            tm.refused(cm, call, text=b"stale")
            tm.refused(cm, call, text=b"cm_map_match_configure")                                 # ... which names the reason
        tm.refused(cm, cm.map_match, I, text=b"no result")                                       # no frame yet
        frame(cm)
        tm.refused(cm, cm.map_match, I, text=b"cm_map_integrate")                                # n_frames == 0
        cm.map_cost_update()
        tm.refused(cm, cm.map_match, I, text=b"cm_map_integrate")                                # still no frame in the map
        cm.map_integrate(None)
        tm.refused(cm, cm.map_match, I, text=b"cm_map_cost_update")                              # dist2 is stale
        cm.map_cost_update()
        for call in (cm.map_match_scores, cm.map_match_device):
            tm.refused(cm, call, text=b"cm_map_cost_update")
        res = cm.map_match(I)                                                                    # an integrated frame may be matched
        vol, _ = cm.map_match_scores()
        assert (res.k, res.i, res.j, res.score) == (0, 0, 0, 255 * 5) and vol[1, 2, 2] == 255 * 5
        frame(cm)                                                                                # a merge
        for call in (cm.map_match_scores, cm.map_match_device):
            tm.refused(cm, call, text=b"merge")
        assert L.cm_map_match_copy(cm._ctx, buf.ctypes.data, 75, None) == capi.BAD_ARG and (buf == 7).all()
        assert cm.map_match(I).score == 255 * 5 and cm.map_match_scores()[0].tobytes() == vol.tobytes()    # a frame that is not integrated
        cm.map_integrate(None)
        for call in (cm.map_match_scores, cm.map_match_device):
            tm.refused(cm, call, text=b"cm_map_integrate")
        tm.refused(cm, cm.map_match, I, text=b"stale")
        cm.map_cost_update()
        tm.refused(cm, cm.map_match_scores, text=b"cm_map_cost_update")
        cm.map_match(I)
        cm.map_match_scores()
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)                                             # configure again: stale again
        tm.refused(cm, cm.map_match_scores, text=b"cm_map_match_configure")
        cm.map_match(I)
        cm.map_match_configure(None)                                                             # NULL frees
        tm.refused(cm, cm.map_match, I, text=b"cm_map_match_configure")
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
        cm.map_cost_configure(0.35, 1.05, 3.0, True)                                             # the cost layer takes it along
        tm.refused(cm, cm.map_match, I, text=b"cm_map_match_configure")
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
        cm.map_cost_configure(None)
        tm.refused(cm, cm.map_match, I, text=b"cm_map_cost_configure")
        small_stack(cm)
        tm.configure(cm, tc.map_q(cell, nx, ny))                                                 # and so does the map
        tm.refused(cm, cm.map_match, I, text=b"cm_map_cost_configure")
        small_stack(cm)
        cm.map_configure(None)
        tm.refused(cm, cm.map_match, I, text=b"cm_map_configure")
        cm.map_match_configure(None)                                                             # freeing what is not there is fine


@pytest.mark.gpu
def test_refusals_and_capacity():
    nx, ny, cell = 64, 48, 0.1
    I = np.eye(3, 4, dtype=F32)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        L = cm._lib
        small_stack(cm, match=False)
        ok = mf.params(n_a=1, a_stride=8, wx=2, wy=2)
        for kw in REFUSED_PARAMS:                      # every refusal of the restatement's validator is the library's
            q = dict(ok, **kw)
            p = capi.MatchParams(q["sigma"], q["max_dist"], q["n_a"], q["a_stride"], q["wx"], q["wy"], q["flags"])
            assert L.cm_map_match_configure(cm._ctx, C.byref(p)) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
        tm.refused(cm, cm.map_match, I, text=b"cm_map_match_configure")                          # a refused call configured nothing
        for kw in ACCEPTED_PARAMS:
            configure_match(cm, dict(ok, **kw))
        configure_match(cm, ok)
        tg.run_frame(cm, tc.frame_of([(3, 2), (40, 30)], cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
        cm.map_integrate(None)
        cm.map_cost_update()
        res = cm.map_match(I)
        vol, _ = cm.map_match_scores()
        assert res.score == 510 and L.cm_map_match_evaluate(cm._ctx, None, None) == capi.BAD_ARG
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, 3, 7, 10, 11):
                P = I.copy()
                P.reshape(-1)[at] = bad
                tm.refused(cm, cm.map_match, P, text=b"finite")
        far = I.copy()
        far[0, 3] = 3e38
        tm.refused(cm, cm.map_match, far, text=b"vehicle")
        assert cm.map_match_scores()[0].tobytes() == vol.tobytes()                               # a refused evaluate leaves the volume
        moved = cm.map_match(tm.pose_t(0.1, 0.0))
        assert (moved.i, moved.j) == (-1, 0) and cm.map_match_scores()[0].tobytes() != vol.tobytes()
        res = cm.map_match(I)
        assert cm.map_match_scores()[0].tobytes() == vol.tobytes()                               # a function of the inputs alone
        # destinations that are too small: CM_CAPACITY, nothing copied, the result still written
        buf = np.full(80, 7, np.uint32)
        for cap in (74, 0):
            got = capi.MatchResult()
            assert L.cm_map_match_copy(cm._ctx, buf.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (buf == 7).all() and bytes(got) == bytes(res)
        assert L.cm_map_match_copy(cm._ctx, buf.ctypes.data, 80, None) == capi.OK and buf[:75].tobytes() == vol.tobytes() and (buf[75:] == 7).all()
        assert L.cm_map_match_copy(cm._ctx, None, 75, None) == capi.BAD_ARG                      # no destination
        lut = np.full(20, 7, np.uint8)
        n = C.c_uint64(0)
        assert L.cm_map_match_table_copy(cm._ctx, lut.ctypes.data, 16, C.byref(n)) == capi.CAPACITY and n.value == 17 and (lut == 7).all()
        assert L.cm_map_match_table_copy(cm._ctx, None, 17, None) == capi.BAD_ARG
        ptr = C.c_void_p()
        assert L.cm_map_match_device(cm._ctx, C.byref(ptr), None) == capi.OK and ptr.value
        assert L.cm_map_match_device(cm._ctx, None, None) == capi.OK
        # a frame in flight
        cm.submit_all(tc.frame_of([(3, 2), (40, 30)], cell, nx, ny, tc.OUTSIDE))
        cm.merge_voxelize_async(capi.make_params(tc.PARAMS))
        for c in (lambda: cm.map_match_configure(0.1, 0.3), cm.map_match_scores, cm.map_match_device, cm.map_match_table, lambda: cm.map_match(I)):
            tm.refused(cm, c, text=b"flight")
        assert cm.wait().status == capi.OK
        tm.refused(cm, cm.map_match_scores, text=b"merge")


@pytest.mark.gpu
def test_an_evaluate_changes_no_other_layer():
    nx, ny, cell = 64, 48, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        small_stack(cm, nx, ny)
        cm.map_plan_configure(50, 205, True)
        cm.map_traj_configure(3, 3, 4, [(0.1, 0.0)], 1, 1, True)
        tg.run_frame(cm, tc.frame_of(tc.CORNERS_64_48, cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
        cm.map_integrate(None)
        cm.map_cost_update()
        cm.map_plan_update(2.05, 1.05)
        cm.map_traj_evaluate(0.05, 0.05, 0.0, (0.0, 1.0), (-1.0, 1.0), 0.1)

        def state():
            table, info = cm.map()
            cost, dist2, _ = cm.map_cost()
            return (table.tobytes(), cm.map_occupancy()[0].tobytes(), tm.info_tuple(info), cost.tobytes(), dist2.tobytes(), cm.map_cost_table().tobytes(),
                    cm.map_plan()[0].tobytes(), cm.map_traj()[0].tobytes(), bytes(cm.map_traj()[1]), cm.merged(4096).tobytes())

        before = state()
        assert not any("match" in n for n, _ in cm.stage_times())
        res = cm.map_match(tm.pose_t(0.2, -0.1))
        assert [n for n, _ in cm.stage_times()] == ["match_clear", "k_match_field", "k_match_mark", "k_match_score", "k_match_best"]
        assert all(ms >= 0.0 for _, ms in cm.stage_times()) and (res.i, res.j, res.score) == (-2, 1, 255 * 5)
        assert state() == before                       # nothing went stale either: every read above still answers
        tg.run_frame(cm, tc.frame_of([(3, 2)], cell, nx, ny, tc.OUTSIDE), tc.PARAMS)      # a frame's own list never holds the call's stages
        assert not any("match" in n for n, _ in cm.stage_times())
