"""The rolling log-odds occupancy map accumulated over frames: cm_map_configure, cm_map_integrate, cm_map_copy, cm_map_device,
cm_map_occupancy_copy (include/cloudmerge.h, cm_kernels_map.hip).

The bar on the GPU: after every frame of a sequence every byte of the state table, of the image, of the info and of the
device-pointer variant equal to the restatement (tests/map_ref.py: MapVectorised) fed with the same context's merged() and
ground() host copies, the per-point sensor (the tag tests/test_grid_map.py's scenes carry in the intensity), the sensors'
translations and the poses. There is no tolerance: everything is integer arithmetic over sets of distinct rays apart from the
fp32 cell computation, which the restatement repeats operation by operation. No comparison is vacuous: map_ref.guards (and
scroll_guards where the window moves) is asserted on the restatement's own output before the device's bytes are looked at,
wherever the sequence can satisfy it, and test_the_sequences_satisfy_the_guards checks on the CPU that the named seeds do."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from tests import map_ref as mr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
F32 = np.float32
INF = float("inf")
NAMES = ("cm_map_configure", "cm_map_integrate", "cm_map_copy", "cm_map_device", "cm_map_occupancy_copy")
TRANS = tr.TRANS
COARSE = tg.COARSE
NO_G = np.zeros((0, 4), F32)
MAP_TYPES = (capi.MapParams, capi.MapCell, capi.MapInfo)          # (a library without the map fails every test here, at import)


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_map_structs_match_header(tmp_path):
    fields_p = ["cell", "nx", "ny", "z_min", "z_max", "l_hit", "l_miss", "l_min", "l_max", "l_free", "l_occ", "max_range_cells"]
    fields_i = ["anchor", "nx", "ny", "n_frames", "sensors_cast", "_pad"]
    items = (["sizeof(cm_map_params)"] + [f"offsetof(cm_map_params,{f})" for f in fields_p] +
             ["sizeof(cm_map_cell)", "offsetof(cm_map_cell,logodds)", "offsetof(cm_map_cell,n_obs)", "sizeof(cm_map_info)"] +
             [f"offsetof(cm_map_info,{f})" for f in fields_i])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, B, I = MAP_TYPES
    want = ([C.sizeof(P)] + [getattr(P, f).offset for f in fields_p] + [C.sizeof(B), B.logodds.offset, B.n_obs.offset, C.sizeof(I)] +
            [getattr(I, f).offset for f in fields_i])
    assert got == want
    assert got[:13] == [48] + list(range(0, 48, 4))                          # twelve 4-byte fields, no padding
    assert got[13:] == [8, 0, 4, 32, 0, 8, 12, 16, 24, 28]
    d = capi.MAP_DTYPE
    assert d == mr.MAP_DTYPE and d.itemsize == 8 and [d.fields[f][1] for f in ("logodds", "n_obs")] == [0, 4]
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)
    m = re.search(r"#define\s+CM_MAP_MAX_LOGODDS\s+\(1 << (\d+)\)", text)
    assert m and 1 << int(m.group(1)) == capi.MAP_MAX_LOGODDS == mr.MAX_LOGODDS


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.map_params(0.5, 4, 4)
    pose = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    info = capi.MapInfo()
    before = bytes(info)
    out = np.zeros(16, capi.MAP_DTYPE)
    img = np.full(16, 7, np.int8)
    ptr = C.c_void_p(5)
    assert L.cm_map_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_integrate(None, pose, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_copy(None, out.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_device(None, C.byref(ptr), C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_occupancy_copy(None, img.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert not out.view(np.uint8).any() and (img == 7).all() and bytes(info) == before and ptr.value == 5


# ---- poses, clouds, sequences ---------------------------------------------------------------------------------------------
def pose_t(tx, ty, tz=0.0):
    P = np.eye(3, 4, dtype=F32)
    P[:, 3] = (tx, ty, tz)
    return P


def pose_rot(yaw_deg, pitch_deg, t):
    cy, sy = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    cp, sp = math.cos(math.radians(pitch_deg)), math.sin(math.radians(pitch_deg))
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    return np.concatenate([Rz @ Ry, np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F32)


def frames_of(seed, n, n_sensors=3, n_per=1500):
    return [tr.scene(seed + k, n_sensors, n_per) for k in range(n)]


def restate_sequence(q, clouds, trans, poses, loop=False):
    """clouds: per frame (A, G). The history of (table, image, info)."""
    ref = (mr.MapLoop if loop else mr.MapVectorised)(q)
    return [ref.integrate(A, G, tg.sensor_of(A), tg.sensor_of(G), trans, P) for (A, G), P in zip(clouds, poses)]


# Named sequences on scene(seed + k) under TRANS[:3]: the parameters and the poses. Each holds the guards (checked on the CPU
# below from the clouds pure translations give); the ones whose window moves hold the scroll guards too.
Q64 = mr.params(0.5, 64, 64)                      # 32 m: the scenes reach beyond every edge, so a scroll drops observed cells
SEQUENCES = {
    "identity": (40, Q64, [pose_t(0, 0)] * 3, False),
    "whole_cells": (43, Q64, [pose_t(0, 0), pose_t(1.0, 0.5), pose_t(2.5, -1.5)], True),
    "fractional": (46, Q64, [pose_t(0.3, 0.2), pose_t(0.77, -0.41), pose_t(1.93, 0.26)], True),
    "negative": (49, Q64, [pose_t(-3.2, -7.9), pose_t(-4.1, -8.3), pose_t(-5.7, -9.6)], True),
    "yaw_pitch_z": (52, Q64, [pose_rot(30.0, 5.0, (2.0, 1.0, 0.7)), pose_rot(30.0, 5.0, (2.9, 1.6, 0.7)),
                              pose_rot(31.0, 5.5, (3.8, 2.1, 0.8))], True),
    "odd": (55, mr.params(0.5, 63, 57), [pose_t(0.2, 0.1), pose_t(0.9, -0.6), pose_t(1.4, -1.3)], True),
    "saturating": (58, mr.params(0.5, 64, 64, l_hit=85, l_miss=40, l_min=-60, l_max=100, l_free=-40, l_occ=85), [pose_t(0, 0)] * 3, False),
}
JUMP = (61, Q64, [pose_t(0, 0), pose_t(1.0, 0.0), pose_t(100.0, 100.0), pose_t(101.0, 100.0)])


def moved_clouds(seed, n, trans=TRANS, n_sensors=3, n_per=1500):
    return [(tr.moved(parts, trans), NO_G) for parts in frames_of(seed, n, n_sensors, n_per)]


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def test_the_two_restatements_agree():
    rays = 0
    poses = [pose_t(0.3, 0.2), pose_rot(30.0, 5.0, (0.9, -0.6, 0.7)), pose_t(-1.2, -0.7), pose_t(40.0, 0.0)]
    for k, q in enumerate([mr.params(0.5, 24, 24), mr.params(0.75, 13, 9, max_range_cells=3), mr.params(1.0, 1, 1),
                           mr.params(1.0, 12, 1), mr.params(0.5, 24, 24, z_band=(1.8, 2.5), l_min=-60, l_max=100),
                           mr.params(0.25, 30, 40, l_hit=1, l_miss=1, l_min=-2, l_max=2, l_free=-1, l_occ=1)]):
        clouds = []
        for f, parts in enumerate(frames_of(70 + 4 * k, 4, 3, 120)):
            A = tr.moved([p * F32([0.3, 0.3, 1.0, 1.0]) for p in parts])
            pick = np.random.default_rng(k * 10 + f).random(len(A)) < 0.3
            clouds.append((A[~pick], A[pick] + F32([0.0, 0.0, -0.2, 0.0])))
        a = restate_sequence(q, clouds, TRANS[:3], poses)
        b = restate_sequence(q, clouds, TRANS[:3], poses, loop=True)
        for (ta, ia, fa), (tb, ib, fb) in zip(a, b):
            assert ta.tobytes() == tb.tobytes() and ia.tobytes() == ib.tobytes()
            assert all(fa[key] == fb[key] for key in fb)
            rays += fa["n_rays"]
        assert a[3][2]["carried"] == 0 and a[3][2]["anchor"] != a[2][2]["anchor"]     # the last pose is far away
    assert rays > 2000


def test_known_answers_on_a_5_by_4_map():
    """Unit cells, l_hit 85, l_miss 40, clamps -100 and 200, thresholds -40 and 85. Frame 1: the vehicle at (2.5, 2.5), cell (2, 2),
    anchor (0, 0). Sensor 0 at window cell (0, 1), sensor 1 at (0, 3); both hit (4, 1); sensor 1 has a ground return in (2, 3).
    Sensor 1 walks (0,3), (1,2), (2,2), (3,1) to the hit and (0,3), (1,3) to the ground end. Frame 2: the same clouds, the vehicle
    one cell further along x, so the window scrolls by one cell and the evidence per window cell is the same."""
    q = mr.params(1.0, 5, 4, l_hit=85, l_miss=40, l_min=-100, l_max=200, l_free=-40, l_occ=85)
    A = F32([[2.0, -1.0, 0.0, 0.0], [2.0, -1.0, 0.5, 1.0]])
    G = F32([[0.0, 1.0, 0.0, 1.0]])
    trans = [(-2.0, -1.0, 0.0), (-2.0, 1.0, 0.0)]
    poses = [pose_t(2.5, 2.5), pose_t(3.5, 2.5)]
    for loop in (False, True):
        (t1, i1, f1), (t2, i2, f2) = restate_sequence(q, [(A, G)] * 2, trans, poses, loop)
        assert f1["anchor"] == (0, 0) and f2["anchor"] == (1, 0) and f1["sensors_cast"] == f2["sensors_cast"] == 3
        assert (f1["n_frames"], f2["n_frames"]) == (1, 2)
        d = [[0, 0, 0, 0, 0], [-40, -40, -40, -80, 170], [0, -40, -40, 0, 0], [-80, -40, -40, 0, 0]]
        assert t1["logodds"].tolist() == d and t1["n_obs"].tolist() == [[int(v != 0) for v in row] for row in d]
        assert i1.tolist() == [[-1] * 5, [0, 0, 0, 0, 100], [-1, 0, 0, -1, -1], [0, 0, 0, -1, -1]]
        # the old columns 1..4 are the new columns 0..3; -40 - 80 = -120 clamps to -100 twice; 170 - 80 = 90 stays occupied
        assert t2["logodds"].tolist() == [[0, 0, 0, 0, 0], [-80, -80, -100, 90, 170], [-40, -80, -40, 0, 0], [-100, -80, -40, 0, 0]]
        assert t2["n_obs"].tolist() == [[0, 0, 0, 0, 0], [2, 2, 2, 2, 1], [1, 2, 1, 0, 0], [2, 2, 1, 0, 0]]
        assert i2.tolist() == [[-1] * 5, [0, 0, 0, 100, 100], [0, 0, 0, -1, -1], [0, 0, 0, -1, -1]]
        if not loop:
            assert f1["ground_only"] == 1 and f1["hit_over_pass"] == 0 and f2["clamped"] == 2
            assert f2["carried"] == 8 and f2["dropped"] == 2 and f1["n_rays"] == 3 and f1["longest"] == 4


def test_every_parameter_refusal_of_the_restatement():
    ok = mr.params(0.5, 8, 8)
    assert mr.refusal(ok) is None
    bad = lambda **kw: mr.refusal(dict(ok, **kw))
    for cell in (0.0, -0.5, np.nan, INF, -INF):
        assert bad(cell=cell) == "cell"
    assert bad(cell=1e-39) == "inv"
    for nx, ny in ((0, 8), (8, 0), (2049, 2048), (2 ** 32 - 1, 2 ** 32 - 1), (2 ** 31, 2)):
        assert bad(nx=nx, ny=ny) == "size"
    assert mr.refusal(mr.params(0.5, 2048, 2048)) is None
    for band in ((np.nan, 1.0), (0.0, np.nan), (1.0, 0.5), (INF, -INF)):
        assert bad(z_band=band) == "band"
    assert bad(z_band=(-INF, INF)) is None and bad(z_band=(1.0, 1.0)) is None
    assert bad(l_hit=0) == bad(l_miss=0) == bad(l_hit=-5) == "step"
    big = mr.MAX_LOGODDS + 1
    for kw in (dict(l_hit=big), dict(l_miss=big), dict(l_max=big), dict(l_min=-big), dict(l_occ=big, l_max=big), dict(l_free=-big, l_min=-big)):
        assert bad(**kw) == "magnitude"
    assert bad(l_max=mr.MAX_LOGODDS, l_min=-mr.MAX_LOGODDS, l_hit=mr.MAX_LOGODDS, l_miss=mr.MAX_LOGODDS) is None
    for kw in (dict(l_free=85), dict(l_free=90), dict(l_occ=351), dict(l_free=-201), dict(l_min=1, l_free=2), dict(l_max=-1, l_occ=-2, l_free=-40),
               dict(l_min=10, l_free=20, l_occ=30)):
        assert bad(**kw) == "order", kw
    assert bad(l_min=0, l_free=0, l_occ=1, l_max=1) is None
    assert not mr.pose_ok(pose_t(np.nan, 0.0)) and not mr.pose_ok(pose_t(0.0, INF)) and mr.pose_ok(pose_t(1e30, 0.0))
    assert mr.vehicle_cell(pose_t(1e30, 0.0), 0.5) is None and mr.vehicle_cell(pose_t(-0.2, 0.7), 0.5) == (-1, 1)
    assert mr.vehicle_cell(pose_t(536870911.0, 0.0), 0.5) is None and mr.vehicle_cell(pose_t(536870848.0, 0.0), 0.5) == (1073741696, 0)


GROUND_Q = mr.params(0.5, 50, 16)                 # 25 m x 8 m around the vehicle, inside the plane (x from -15 m, y within 5 m)
GROUND_TRANS = [(1.2, 0.6, 0.0), (-1.2, -0.6, 0.0)]
GROUND_POSES = [pose_t(20.0, 0.0), pose_t(21.3, 0.2), pose_t(22.6, 0.4)]


def test_the_sequences_satisfy_the_guards():
    for name, (seed, q, poses, scrolls) in SEQUENCES.items():
        h = restate_sequence(q, moved_clouds(seed, len(poses)), TRANS[:3], poses)
        mr.guards(h)
        if scrolls:
            mr.scroll_guards(h)
        if name == "saturating":                    # three frames saturate: clamps in every frame, cells at both limits
            assert all(i["clamped"] > 0 for _, _, i in h)
            assert (h[2][0]["logodds"] == q["l_max"]).any() and (h[2][0]["logodds"] == q["l_min"]).any()
    seed, q, poses = JUMP
    h = restate_sequence(q, moved_clouds(seed, 4), TRANS[:3], poses)
    mr.guards(h)
    mr.scroll_guards(h)
    assert h[1][2]["carried"] > 0 and h[2][2]["carried"] == 0 and h[2][2]["dropped"] > 0 and h[3][2]["carried"] > 0
    # a ground-only end, with the plane of tests/test_grid_map.py's ground scene taken as G by height
    clouds = []
    for k in range(3):
        A = tr.moved(tg.ground_scene(31 + k), GROUND_TRANS)
        low = A[:, 2] < 0.5
        clouds.append((A[~low], A[low]))
    h = restate_sequence(GROUND_Q, clouds, GROUND_TRANS, GROUND_POSES)
    mr.guards(h, ground=True)
    mr.scroll_guards(h)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def configure(cm, q):
    cm.map_configure(q["cell"], q["nx"], q["ny"], q["z_band"], q["l_hit"], q["l_miss"], q["l_min"], q["l_max"], q["l_free"], q["l_occ"],
                     q["max_range_cells"])


def info_tuple(info):
    return (tuple(info.anchor), info.nx, info.ny, info.n_frames, info.sensors_cast, info._pad)


def want_info(i):
    return (i["anchor"], i["nx"], i["ny"], i["n_frames"], i["sensors_cast"], 0)


def read_map(cm, info):
    """What the context holds after an integration: the info of every call, the table, the image, the device table."""
    table, i1 = cm.map()
    image, i2 = cm.map_occupancy()
    ptr, i3 = cm.map_device()
    assert ptr and info_tuple(i1) == info_tuple(i2) == info_tuple(i3) == info_tuple(info)
    d = np.zeros_like(table)
    assert tg.hip_rt().hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(table.nbytes), 2) == 0
    return table, image, d


def compare(got, want, label):
    (table, image, dev), (t, img, i) = got, want
    nx, ny = i["nx"], i["ny"]
    assert table.dtype == t.dtype and table.shape == t.shape == (ny, nx) and image.dtype == np.int8 and image.shape == (ny, nx)
    if table.tobytes() != t.tobytes():
        bad = np.argwhere(table.view(np.uint64) != t.view(np.uint64))
        iy, ix = bad[0][:2]
        raise AssertionError(f"{label}: {len(bad)} of {nx * ny} cells differ, first ({ix}, {iy}): got {table[iy, ix]} want {t[iy, ix]}")
    assert image.tobytes() == img.tobytes(), label
    assert dev.tobytes() == t.tobytes(), label


def run_sequence(cm, q, frames, poses, trans, n_cap, params=None, ground=False, guard=True, scrolls=False, configure_first=True):
    """Frame by frame: merge, integrate, read everything back, restate from the same context's host clouds. The guards on the
    restatement's history first, then every byte of every frame."""
    params = params or MergeParams(**COARSE)
    if configure_first:
        configure(cm, q)
    ref = mr.MapVectorised(q)
    got, history = [], []
    for parts, P in zip(frames, poses):
        tg.run_frame(cm, tr.clouds_of(parts, trans), params)
        A, G = tg.host_clouds(cm, n_cap, ground)
        info = cm.map_integrate(P)
        got.append((read_map(cm, info), info_tuple(info)))
        history.append(ref.integrate(A, G, tg.sensor_of(A), tg.sensor_of(G), trans, P))
        i = history[-1][2]
        print(f"map {q['nx']} x {q['ny']} frame {i['n_frames']} anchor {i['anchor']}: A {len(A)} G {len(G)} rays {i['n_rays']} steps "
              f"{i['steps']} longest {i['longest']} cast {i['sensors_cast']:b} clamped {i['clamped']} carried {i['carried']} dropped "
              f"{i['dropped']} hit-over-pass {i['hit_over_pass']} ground-only {i['ground_only']} image "
              f"{np.bincount(history[-1][1].ravel().astype(int) + 1, minlength=102)[[0, 1, 101]].tolist()}")
    if guard:
        mr.guards(history, ground)
    if scrolls:
        mr.scroll_guards(history)
    for k, ((g, gi), want) in enumerate(zip(got, history)):
        assert gi == want_info(want[2]), (k, gi, want_info(want[2]))
        compare(g, want, f"frame {k}")
    return history


def n_cap_of(frames):
    return max(sum(len(p) for p in parts) for parts in frames)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequences(name):
    seed, q, poses, scrolls = SEQUENCES[name]
    frames = frames_of(seed, len(poses))
    n_cap = n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = run_sequence(cm, q, frames, poses, TRANS[:3], n_cap, scrolls=scrolls)
        if name == "yaw_pitch_z":                  # P2 * z matters: without it another table
            A = tr.moved(frames[0])
            flat = poses[0].copy()
            flat[:2, 2] = 0.0
            other = restate_sequence(q, [(A, NO_G)], TRANS[:3], [flat])
            assert other[0][0].tobytes() != h[0][0].tobytes()
        if name == "saturating":
            assert all(i["clamped"] > 0 for _, _, i in h)


@pytest.mark.gpu
def test_a_jump_larger_than_the_window_restarts_everything():
    seed, q, poses = JUMP
    frames = frames_of(seed, 4)
    n_cap = n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = run_sequence(cm, q, frames, poses, TRANS[:3], n_cap, scrolls=True)
        assert h[2][2]["carried"] == 0 and h[2][2]["dropped"] > 0 and h[3][2]["carried"] > 0
        assert h[2][0]["n_obs"].max() == 1                                  # every cell of the third frame started anew


@pytest.mark.gpu
def test_one_by_one():
    frames = frames_of(64, 3)
    n_cap = n_cap_of(frames)
    q = mr.params(45.0, 1, 1, l_hit=85, l_max=200)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = run_sequence(cm, q, frames, [pose_t(0, 0), pose_t(1.0, 1.0), pose_t(50.0, 0.0)], TRANS[:3], n_cap, guard=False)
        # L = 0 for every ray: three hits per frame, clamped in the second; the third frame is another cell
        assert [int(t["logodds"][0, 0]) for t, _, _ in h] == [200, 200, 200] and [int(t["n_obs"][0, 0]) for t, _, _ in h] == [1, 2, 1]
        assert [i["anchor"] for _, _, i in h] == [(0, 0), (0, 0), (1, 0)]


@pytest.mark.gpu
def test_2048_by_2048_with_a_few_hundred_points():
    frames = frames_of(67, 3, 3, 100)
    n_cap = n_cap_of(frames)
    q = mr.params(0.02, 2048, 2048)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = run_sequence(cm, q, frames, [pose_t(0.0, 0.0), pose_t(0.31, -0.17), pose_t(0.9, 0.4)], TRANS[:3], n_cap, scrolls=True)
        assert all(i["n_rays"] > 200 for _, _, i in h) and h[0][2]["steps"] > 100_000


@pytest.mark.gpu
def test_with_ground_removal():
    frames = [tg.ground_scene(31 + k) for k in range(3)]
    n_cap = n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params([tg.FRONT, tg.FRONT]))
        h = run_sequence(cm, GROUND_Q, frames, GROUND_POSES, GROUND_TRANS, n_cap, MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=1, **tg.ROI),
                         ground=True, scrolls=True)
        assert all(i["ground_only"] > 0 for _, _, i in h)                   # ground ends count as misses


@pytest.mark.gpu
def test_with_statistical_outlier_removal():
    frames = frames_of(80, 3)
    for k, parts in enumerate(frames):
        rng = np.random.default_rng(5 + k)
        loose = np.concatenate([rng.uniform(8.0, 14.0, (40, 2)), rng.uniform(25.0, 38.0, (40, 1))], axis=1)   # inside the window, far above
        parts[0] = np.concatenate([parts[0], tg.tagged(loose, 0)])                         # loose points: removed, no evidence
    n_cap = n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        cm.set_statistical_outlier(8, 0.5)
        run_sequence(cm, Q64, frames, SEQUENCES["fractional"][2], TRANS[:3], n_cap, scrolls=True)
        assert cm.sor_stats().n_removed > 0


@pytest.mark.gpu
def test_with_deskew():
    """The points move with the ego-motion; the origins stay the translations that were set, and the pose is the one at t_ref."""
    frames = frames_of(83, 3)
    n_cap = n_cap_of(frames)
    t_ref = 1_700_000_000_000_000_000
    m = capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000 * (s + 1) for s in range(3)])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        cm.set_ego_motion(m)
        h = run_sequence(cm, Q64, frames, SEQUENCES["whole_cells"][2], TRANS[:3], n_cap, scrolls=True)
        other = restate_sequence(Q64, [(tr.moved(frames[0]), NO_G)], TRANS[:3], SEQUENCES["whole_cells"][2][:1])
        assert other[0][0].tobytes() != h[0][0].tobytes()                    # the points did move


@pytest.mark.gpu
def test_with_a_crop_box():
    frames = frames_of(86, 3)
    n_cap = n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        # (the box ends inside the window: only a scroll of several metres drops observed cells)
        h = run_sequence(cm, Q64, frames, [pose_t(0.2, 0.1), pose_t(7.9, -6.4), pose_t(15.3, -12.7)], TRANS[:3], n_cap,
                         MergeParams(**COARSE, crop_min=(-10.0, -12.0, -1.0), crop_max=(12.0, 10.0, 5.0)), scrolls=True)
        assert all(0 < i["n_rays"] < 2500 for _, _, i in h)


@pytest.mark.gpu
def test_a_sensor_whose_origin_leaves_the_window():
    """A 16 x 16 window of 0.5 m cells. Sensor 2 sits 3.8 m ahead: window column 15 while the vehicle is at the start of its cell,
    column 16 — outside — once the vehicle has moved 0.3 m within that cell, column 15 again in the next cell. Its hits count."""
    trans = [TRANS[0], TRANS[1], (3.8, 0.1, 1.8)]
    frames = frames_of(89, 3)
    n_cap = n_cap_of(frames)
    q = mr.params(0.5, 16, 16)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = run_sequence(cm, q, frames, [pose_t(0.0, 0.0), pose_t(0.3, 0.0), pose_t(0.6, 0.0)], trans, n_cap, scrolls=True)
        assert [i["sensors_cast"] for _, _, i in h] == [7, 3, 7]
        A = tr.moved(frames[1], trans)
        without = restate_sequence(q, [(A[tg.sensor_of(A) != 2], NO_G)], trans, [pose_t(0.3, 0.0)])
        alone = restate_sequence(q, [(A, NO_G)], trans, [pose_t(0.3, 0.0)])
        assert without[0][0].tobytes() != alone[0][0].tobytes()              # the sensor that cast nothing still hit


@pytest.mark.gpu
def test_max_range_around_the_longest_ray():
    frames = frames_of(92, 1)
    n_cap = n_cap_of(frames)
    dry = restate_sequence(Q64, [(tr.moved(frames[0]), NO_G)], TRANS[:3], [pose_t(0.2, 0.1)])
    longest = dry[0][2]["longest"]
    assert longest > 20
    tables = {}
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        for rng_cells in (longest - 1, longest, longest + 1, 1):
            q = dict(Q64, max_range_cells=rng_cells)
            h = run_sequence(cm, q, frames, [pose_t(0.2, 0.1)], TRANS[:3], n_cap, guard=rng_cells > 1)
            tables[rng_cells] = h[0][0].tobytes()
            assert h[0][2]["longest"] == longest
    assert tables[longest] == tables[longest + 1] == dry[0][0].tobytes() and tables[longest - 1] != tables[longest] != tables[1]


def refused(cm, call, *args, text=None):
    with pytest.raises(capi.CloudMergeError) as e:
        call(*args)
    assert e.value.status == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)
    if text:
        assert text in cm._lib.cm_last_error(cm._ctx), cm._lib.cm_last_error(cm._ctx)


@pytest.mark.gpu
def test_refusals_capacity_and_what_configure_clears():
    frames = frames_of(95, 2)
    n_cap = n_cap_of(frames)
    sensors = tr.clouds_of(frames[0])
    params = MergeParams(**COARSE)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        refused(cm, cm.map_integrate, None)                                  # no result, no map
        refused(cm, cm.map)
        refused(cm, cm.map_occupancy)
        refused(cm, cm.map_device)
        tg.run_frame(cm, sensors, params)
        refused(cm, cm.map_integrate, None, text=b"cm_map_configure")        # a result, no configured map
        # every parameter refusal of the restatement's validator is the library's, and nothing it accepts is refused
        ok = mr.params(0.5, 8, 8)
        big = mr.MAX_LOGODDS + 1
        cases = ([dict(cell=v) for v in (0.0, -0.5, np.nan, INF, 1e-39)] + [dict(nx=0), dict(ny=0), dict(nx=2049, ny=2048), dict(nx=2 ** 31, ny=2)] +
                 [dict(z_band=b) for b in ((np.nan, 1.0), (0.0, np.nan), (1.0, 0.5))] + [dict(l_hit=0), dict(l_miss=0), dict(l_hit=big),
                 dict(l_min=-big), dict(l_max=big), dict(l_free=85), dict(l_occ=351), dict(l_free=-201), dict(l_min=1, l_free=2),
                 dict(l_max=-1, l_occ=-2, l_free=-40)])
        for kw in cases:
            q = dict(ok, **kw)
            assert mr.refusal(q) is not None
            refused(cm, configure, cm, q)
        refused(cm, cm.map_integrate, None, text=b"cm_map_configure")        # a refused configure call configured nothing
        for q in (ok, mr.params(0.5, 2048, 2048), dict(ok, l_min=0, l_free=0, l_occ=1, l_max=1), dict(ok, z_band=(1.0, 1.0))):
            assert mr.refusal(q) is None
            configure(cm, q)
        configure(cm, Q64)
        # a configured map is clear: every cell {0, 0}, the image -1, no frame integrated
        table, info = cm.map()
        image, _ = cm.map_occupancy()
        assert info_tuple(info) == ((0, 0), 64, 64, 0, 0, 0) and not table.view(np.uint8).any() and (image == -1).all()
        for bad in (pose_t(np.nan, 0.0), pose_t(0.0, INF), pose_rot(np.nan, 0.0, (0, 0, 0))):
            refused(cm, cm.map_integrate, bad, text=b"finite")
        refused(cm, cm.map_integrate, pose_t(1e30, 0.0), text=b"cell")       # a vehicle cell that does not exist
        refused(cm, cm.map_integrate, pose_t(0.0, -536870912.0), text=b"cell")
        assert cm.map()[1].n_frames == 0
        info = cm.map_integrate(pose_t(0.2, 0.1))
        assert info.n_frames == 1
        refused(cm, cm.map_integrate, pose_t(0.2, 0.1), text=b"already")     # each frame at most once
        refused(cm, cm.map_integrate, pose_t(5.0, 5.0), text=b"already")
        table, info = cm.map()
        assert info.n_frames == 1 and table["n_obs"].any()
        # a destination that is too small: CM_CAPACITY, nothing copied
        out = np.zeros(64 * 64, capi.MAP_DTYPE)
        img = np.full(64 * 64, 7, np.int8)
        for cap in (64 * 64 - 1, 0):
            assert cm._lib.cm_map_copy(cm._ctx, out.ctypes.data, cap, None) == capi.CAPACITY and not out.view(np.uint8).any()
            assert cm._lib.cm_map_occupancy_copy(cm._ctx, img.ctypes.data, cap, None) == capi.CAPACITY and (img == 7).all()
        assert cm._lib.cm_map_copy(cm._ctx, out.ctypes.data, 64 * 64, None) == capi.OK and out.tobytes() == table.tobytes()
        # a frame in flight, and results that have no frame's clouds behind them
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        refused(cm, cm.map_integrate, None, text=b"flight")
        refused(cm, cm.map)
        refused(cm, configure, cm, Q64)
        assert cm.wait().status == capi.OK
        cm.submit_all(sensors)
        assert cm.merge_voxelize(MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)).status == capi.GRID_OVERFLOW
        refused(cm, cm.map_integrate, None)
        cm.submit_all(sensors)
        assert cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40)).status == capi.OK
        refused(cm, cm.map_integrate, None)
        assert cm.map()[0].tobytes() == table.tobytes()                      # none of it touched the map
        # cm_map_configure clears the map; NULL frees it
        configure(cm, Q64)
        table, info = cm.map()
        assert info.n_frames == 0 and not table.view(np.uint8).any() and (cm.map_occupancy()[0] == -1).all()
        cm.map_configure(None)
        refused(cm, cm.map)
        refused(cm, cm.map_integrate, None)


@pytest.mark.gpu
def test_the_map_survives_merges_and_ray_calls_and_changes_no_frame():
    frames = frames_of(98, 3)
    n_cap = n_cap_of(frames)
    params = MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=1)
    grid = ((-24.0, -24.0), 0.5, 96, 96)
    poses = SEQUENCES["fractional"][2]
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_OCCUPANCY) as cm, \
            capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_OCCUPANCY) as never:
        configure(cm, Q64)
        ref = mr.MapVectorised(Q64)
        dry = restate_sequence(Q64, moved_clouds(98, 3), TRANS[:3], poses)     # (plain frames: merged() is the moved parts)
        mr.guards(dry)
        mr.scroll_guards(dry)
        history = []
        for k, (parts, P) in enumerate(zip(frames, poses)):
            outs = []
            for c in (cm, never):
                res = tg.run_frame(c, tr.clouds_of(parts), params)
                cells, counts = c.cells(res.n_out)
                outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes(),
                             c.merged(n_cap).tobytes()))
            assert outs[0] == outs[1]                   # the frame after an integration: that of a context that never had a map
            if k:
                assert cm.map()[0].tobytes() == want[0].tobytes()            # the merge left the map alone
            A, G = tg.host_clouds(cm, n_cap, False)
            want = ref.integrate(A, G, tg.sensor_of(A), tg.sensor_of(G), TRANS[:3], P)
            history.append(want)
            rays_before = cm.grid_rays(*grid).tobytes()
            cleared_before = cm.grid_ray_occupancy().tobytes()
            info = cm.map_integrate(P)
            compare(read_map(cm, info), want, f"frame {k}")
            # the ray tables of the context are what they were, and another ray call gives the same bytes and leaves the map alone
            assert cm.grid_ray_occupancy().tobytes() == cleared_before
            assert cm.grid_rays(*grid).tobytes() == rays_before == never.grid_rays(*grid).tobytes()
            assert cm.grid_occupancy().tobytes() == never.grid_occupancy().tobytes()
            compare(read_map(cm, info), want, f"frame {k} after a ray call")
        assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(history, dry))


@pytest.mark.gpu
def test_stage_names_under_profile():
    frames = frames_of(101, 1)
    n_cap = n_cap_of(frames)
    sensors = tr.clouds_of(frames[0])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_PROFILE) as cm:
        configure(cm, Q64)
        tg.run_frame(cm, sensors, MergeParams(**COARSE))
        assert not any("map" in n for n, _ in cm.stage_times())
        cm.map_integrate(pose_t(0.2, 0.1))
        names = [n for n, _ in cm.stage_times()]
        assert names == ["map_clear", "k_map_mark", "k_ray_cast", "k_map_update"], names
        assert all(ms >= 0.0 for _, ms in cm.stage_times())
        tg.run_frame(cm, sensors, MergeParams(**COARSE))                 # a frame's own list never holds the call's stages
        assert not any("map" in n for n, _ in cm.stage_times())


# ---- a steady-state call allocates nothing: the counts of the test build, as tests/test_ctx_memory.py takes them -------------
def case_steady_state():
    frames = frames_of(104, 4)
    n_cap = n_cap_of(frames)
    poses = [pose_t(0.0, 0.0), pose_t(0.7, 0.3), pose_t(1.9, -0.4), pose_t(60.0, 0.0)]
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        totals = []
        for k, (parts, P) in enumerate(zip(frames, poses)):
            tg.run_frame(cm, tr.clouds_of(parts), MergeParams(**COARSE))
            if k == 0:
                before_configure = capi.device_allocations()
                configure(cm, Q64)                       # every buffer of the map is taken here:
                after_configure = capi.device_allocations()
                assert [a - b for a, b in zip(after_configure, before_configure)] == [5, 5]    # two state tables, image, bitmaps, ray table
            before = capi.device_allocations()
            cm.map_integrate(P)
            cm.map()
            cm.map_occupancy()
            cm.map_device()
            after = capi.device_allocations()
            print(f"frame {k}: before {before} after {after}")
            totals.append((before, after))
        assert all(b == a for b, a in totals), totals                        # no integrate or read allocates, the first included
        assert totals[1][0] == totals[3][1], totals                         # nor does a frame between them
        live = capi.device_allocations()[0]
        cm.map_configure(None)
        assert capi.device_allocations()[0] == live - 5                      # NULL parameters give all five back


@pytest.mark.gpu
def test_a_steady_state_integration_allocates_nothing():
    assert os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")), "the test build is missing"
    env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK")}
    env.update(CM_LIB_VARIANT="testhooks", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_occupancy_map", "steady_state"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    {"steady_state": case_steady_state}[sys.argv[1]]()
