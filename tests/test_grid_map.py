"""The 2-D grid map of the frame: cm_result_grid_map / _device, cm_grid_occupancy_copy (include/cloudmerge.h,
cm_kernels_grid.hip).

The bar on the GPU: every byte of the table and of the occupancy image equal to the restatement (tests/grid_ref.py:
grid_vectorised) fed with the same context's merged() and ground() host copies. There is no tolerance: every field is an
integer count or an extreme, and none depends on an order. No test passes vacuously: before the device's table is looked at,
the restatement's own output must hold all three states and a cell with n >= 2 whose points come from two sensors (the sensor
is written into every point's intensity, which every stage carries through), and with ground removal on a cell with
n_ground > 0 and n > 0. Points are placed by hand to guarantee it.

The frames are a few thousand points, with one exception that is stated where it is made: the quantile route is only taken
by frames large enough for two bucket passes, so the two-frame case runs cfg2's stream at 150 000 points per sensor, the size
tests/test_boxes.py reaches that route with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import grid_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
F32 = np.float32
INF = float("inf")
NAN_BITS = 0x7FC00000
NAMES = ("cm_result_grid_map", "cm_result_grid_map_device", "cm_grid_occupancy_copy")


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_grid_structs_match_header(tmp_path):
    fields_p = ["origin", "cell", "nx", "ny", "z_min", "z_max", "obstacle_height", "min_points"]
    fields_c = ["n", "n_ground", "z_lo", "z_hi", "g_lo", "g_hi", "i_max", "state"]
    items = (["sizeof(cm_grid_params)"] + [f"offsetof(cm_grid_params,{f})" for f in fields_p] + ["sizeof(cm_grid_cell)"] +
             [f"offsetof(cm_grid_cell,{f})" for f in fields_c])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, B = capi.GridParams, capi.GridCell
    want = ([C.sizeof(P)] + [getattr(P, f).offset for f in fields_p] + [C.sizeof(B)] + [getattr(B, f).offset for f in fields_c])
    assert got == want and got[0] == 36 and got[9] == 32
    assert got[1:9] == [0, 8, 12, 16, 20, 24, 28, 32]                  # no implicit padding
    d = capi.GRID_DTYPE
    assert [d.fields[f][1] for f in fields_c] == want[10:] and d == gr.GRID_DTYPE and d.itemsize == 32


def test_constants_mirror_the_header():
    text = open(HEADER).read()

    def define(name):
        m = re.search(r"#define\s+" + name + r"\s+(.+)", text)
        assert m, name
        return eval(m.group(1).split("/*")[0].replace("u", ""))
    assert define("CM_GRID_MAX_CELLS") == capi.GRID_MAX_CELLS == gr.MAX_CELLS == 1 << 22
    assert define("CM_GRID_UNKNOWN") == capi.GRID_UNKNOWN == gr.UNKNOWN == 0
    assert define("CM_GRID_FREE") == capi.GRID_FREE == gr.FREE == 1
    assert define("CM_GRID_OCCUPIED") == capi.GRID_OCCUPIED == gr.OCCUPIED == 2
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.grid_params((0.0, 0.0), 0.5, 4, 4)
    out = np.zeros(16, capi.GRID_DTYPE)
    n = C.c_uint64(7)
    ptr = C.c_void_p()
    assert L.cm_result_grid_map(None, C.byref(p), out.ctypes.data, 16) == capi.BAD_ARG
    assert L.cm_result_grid_map(None, None, None, 0) == capi.BAD_ARG
    assert L.cm_result_grid_map_device(None, C.byref(p), C.byref(ptr), C.byref(n)) == capi.BAD_ARG
    assert L.cm_grid_occupancy_copy(None, None, 0, C.byref(n)) == capi.BAD_ARG
    assert not out.view(np.uint8).any()


# ---- the clouds ---------------------------------------------------------------------------------------------------------
N_SENSORS = 3


def tagged(xyz, sensor, rng=None):
    """(n, 4): the points with the sensor in their intensity, sensor + 10 * k (k random: i_max has something to choose)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    k = rng.integers(0, 20, len(xyz)) if rng is not None else np.zeros(len(xyz))
    return np.concatenate([xyz, (sensor + 10.0 * k)[:, None]], axis=1).astype(F32)


def sensor_of(pts4):
    return np.where(np.isnan(pts4[:, 3]), -1, np.mod(pts4[:, 3], 10)).astype(np.int64)


def scene(seed, n_per=1500, extent=(-20.0, 20.0)):
    """Per sensor: flat returns everywhere (z within 5 cm), poles of up to 2 m on a tenth of the area, and by hand two points
    of every sensor in the cell around (1.05, 1.05) — one flat, one 1 m up — and one flat pair around (-3.05, 2.05)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(N_SENSORS):
        flat = np.concatenate([rng.uniform(*extent, (n_per, 2)), rng.uniform(0.0, 0.05, (n_per, 1))], axis=1)
        base = rng.uniform(extent[0], extent[1], (n_per // 40, 2))
        poles = np.concatenate([np.repeat(base, 4, axis=0) + rng.uniform(0, 0.04, (len(base) * 4, 2)),
                                rng.uniform(0.0, 2.0, (len(base) * 4, 1))], axis=1)
        hand = np.array([[1.05, 1.05, 0.01 * s], [1.05 + 0.01 * s, 1.04, 1.0], [-3.05, 2.05, 0.02], [-3.04, 2.04, 0.03 + 0.01 * s]])
        out.append(tagged(np.concatenate([flat, poles, hand]), s, rng))
    return out


def clouds_of(parts):
    return [xyzi_cloud(p[:, :3], p[:, 3]) for p in parts]


def both(A, G, *args, **kw):
    a, ai = gr.grid_vectorised(A, G, *args, **kw)
    b, bi = gr.grid_loop(A, G, *args, **kw)
    assert a.tobytes() == b.tobytes() and ai.tobytes() == bi.tobytes()
    return a, ai


def holds_what_it_must(want, A, G, origin, cell, nx, ny, z_band, ground):
    """The conditions that keep a comparison from being vacuous, on the restatement's own output."""
    assert set(want["state"].ravel().tolist()) == {gr.UNKNOWN, gr.FREE, gr.OCCUPIED}
    A = gr.a4(A)
    idx, ok = gr.cells_of(A, origin, cell, nx, ny, *z_band)
    tag = sensor_of(A[ok])
    lo = np.full(nx * ny, 99); hi = np.full(nx * ny, -1)
    np.minimum.at(lo, idx[tag >= 0], tag[tag >= 0])
    np.maximum.at(hi, idx[tag >= 0], tag[tag >= 0])
    assert ((hi > lo) & (lo < 99) & (want["n"].ravel() >= 2)).any(), "no cell with points of two sensors"
    if ground:
        assert ((want["n_ground"] > 0) & (want["n"] > 0)).any(), "no cell with ground and non-ground points"


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def face_points(origin, cell, nx, ny, sensor=0):
    """Points on cell faces, on the grid's four outer edges, just inside and on the far edges, at +-0 heights in one cell, at
    both band limits of (-1, 2.5) and one ulp outside them, a NaN intensity beside finite ones and a cell with none but NaN."""
    ox, oy, c = F32(origin[0]), F32(origin[1]), F32(cell)
    i1, i2, i12 = sensor + 10.0, sensor + 20.0, sensor + 120.0
    xs = [F32(ox + F32(k) * c) for k in range(0, nx + 1)]              # every face and both outer edges of x
    ys = [F32(oy + F32(k) * c) for k in range(0, ny + 1)]
    far_x, far_y = xs[-1], ys[-1]
    pts = [(x, F32(oy + c * F32(0.5)), 0.1, i1) for x in xs] + [(F32(ox + c * F32(0.5)), y, 0.1, i2) for y in ys]
    pts += [(np.nextafter(far_x, F32(-INF)), ys[0], 0.2, i1), (far_x, ys[0], 0.2, i2),
            (xs[0], np.nextafter(far_y, F32(-INF)), 0.2, i1), (xs[0], far_y, 0.2, i2),
            (np.nextafter(ox, F32(-INF)), ys[0], 0.2, i1), (xs[0], np.nextafter(oy, F32(-INF)), 0.2, i2)]
    mid = (F32(ox + c * F32(1.5)), F32(oy + c * F32(1.5)))
    pts += [(mid[0], mid[1], 0.0, i1), (mid[0], mid[1], -0.0, i2)]     # +-0 in one cell
    edge = (F32(ox + c * F32(2.5)), F32(oy + c * F32(0.5)))
    pts += [(edge[0], edge[1], -1.0, np.nan), (edge[0], edge[1], 2.5, i12), (edge[0], edge[1], 2.5000002, i1),
            (edge[0], edge[1], -1.0000001, i2)]
    only_nan = (F32(ox + c * F32(3.5)), F32(oy + c * F32(1.5)))         # (a cell no face point above can fall into)
    pts += [(only_nan[0], only_nan[1], 0.3, np.nan), (only_nan[0], only_nan[1], 0.4, np.nan)]
    return np.array(pts, F32)


# (all but the second lie outside the scenes below, which span +-20 m)
HAND_GRIDS = [((30.0, 24.0), 0.1, 7, 5), ((0.0, 0.0), 0.25, 3, 3), ((100.0, -100.0), 0.5, 4, 4), ((-31.0, -31.0), 1e-3, 5, 6)]


def test_the_two_restatements_agree():
    rng = np.random.default_rng(3)
    parts = scene(1, n_per=300, extent=(-3.0, 3.0))
    A = np.concatenate(parts)
    G = A[rng.random(len(A)) < 0.3] + F32([0.0, 0.0, -0.2, 0.0])
    for origin, cell, nx, ny in HAND_GRIDS:
        A = np.concatenate([A, face_points(origin, cell, nx, ny)])
    A = np.concatenate([A, F32([[-0.0, -0.0, 0.5, 0.0], [-0.0, 0.0, 0.6, 1.0]])])       # x = origin - 0.0f at origin 0
    seen = set()
    for origin, cell, nx, ny in HAND_GRIDS + [((-3.0, -3.0), 0.5, 12, 12), ((-3.0, -3.0), 6.0, 1, 1)]:
        for band, h, mp in (((-INF, INF), 0.3, 1), ((-1.0, 2.5), 0.0, 1), ((0.0, 0.0), 0.3, 2), ((-INF, 0.04), 0.02, 3)):
            for g in (G, G[:0]):
                t, img = both(A, g, origin, cell, nx, ny, band, h, mp)
                seen |= set(t["state"].ravel().tolist())
                assert np.array_equal(img, gr.IMAGE_OF_STATE[t["state"]])
                assert t["n"].sum() <= len(A) and t["n_ground"].sum() <= len(g)
    assert seen == {0, 1, 2}
    # a cell of 1e-37 overflows t to inf everywhere but at the origin itself
    t, _ = both(A, G[:0], (float(A[0, 0]), float(A[0, 1])), 1e-37, 2, 2)
    assert t["n"].sum() >= 1 and t["n"][0, 0] == t["n"].sum()


def test_known_answers_on_a_3_by_2_grid():
    """origin (0, 0), cell 1: x in [0, 3), y in [0, 2). Band [-1, 2], obstacle_height 0.5, min_points 2."""
    nan = np.nan
    A = F32([[0.5, 0.5, 0.0, 3.0], [0.25, 0.75, 1.0, 7.0],           # cell (0,0): 2 points, 1 m apart -> OCCUPIED
             [1.5, 0.5, 0.25, nan], [1.0, 0.0, 0.5, nan],            # cell (1,0): on its two lower faces, 0.25 apart -> FREE, i_max NaN
             [2.5, 0.5, 0.0, 1.0],                                   # cell (2,0): one point < min_points -> UNKNOWN
             [0.5, 1.5, 2.0, 5.0], [0.5, 1.5, -1.0, 4.0],            # cell (0,1): both band limits, 3 m apart -> OCCUPIED
             [0.5, 1.5, 2.5, 9.0],                                   #             above the band: not counted
             [3.0, 0.5, 0.0, 1.0], [0.5, 2.0, 0.0, 1.0], [-0.001, 0.5, 0.0, 1.0],   # outside
             [2.5, 1.5, 0.7, 2.0]])                                  # cell (2,1): with two ground points below -> OCCUPIED
    G = F32([[2.5, 1.25, 0.1, 8.0], [2.25, 1.5, 0.15, 6.0],          # cell (2,1)
             [1.5, 1.5, 0.0, 1.0], [1.25, 1.75, 0.05, 2.0]])         # cell (1,1): ground only -> FREE
    t, img = both(A, G, (0.0, 0.0), 1.0, 3, 2, (-1.0, 2.0), 0.5, 2)
    assert t.shape == (2, 3)
    assert t["n"].tolist() == [[2, 2, 1], [2, 0, 1]] and t["n_ground"].tolist() == [[0, 0, 0], [0, 2, 2]]
    assert t["state"].tolist() == [[2, 1, 0], [2, 1, 2]] and img.tolist() == [[100, 0, -1], [100, 0, 100]]
    same = lambda a, b: np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))
    q = F32(np.uint32(NAN_BITS).view(F32))
    assert same(t["z_lo"], [[0.0, 0.25, 0.0], [-1.0, q, 0.7]]) and same(t["z_hi"], [[1.0, 0.5, 0.0], [2.0, q, 0.7]])
    assert same(t["g_lo"], [[q, q, q], [q, 0.0, 0.1]]) and same(t["g_hi"], [[q, q, q], [q, 0.05, 0.15]])
    assert same(t["i_max"], [[7.0, q, 1.0], [5.0, 2.0, 8.0]])
    # the same cell at obstacle_height 0.7: 0.7 - 0.1 rounds below it -> FREE
    t2, _ = both(A, G, (0.0, 0.0), 1.0, 3, 2, (-1.0, 2.0), 0.7, 2)
    assert t2["state"].tolist() == [[2, 1, 0], [2, 1, 1]]
    # +-0: the minimum is -0, the maximum +0
    z = F32([[0.5, 0.5, 0.0, 0.0], [0.5, 0.5, -0.0, -0.0]])
    t3, _ = both(z, z[:0], (0.0, 0.0), 1.0, 1, 1)
    assert same(t3["z_lo"], [[-0.0]]) and same(t3["z_hi"], [[0.0]]) and same(t3["i_max"], [[0.0]])


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def hip_rt():
    try:
        return C.CDLL("libamdhip64.so.7")
    except OSError:
        return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def host_clouds(cm, n_cap, ground):
    A = gr.a4(cm.merged(n_cap))
    G = gr.a4(cm.ground(n_cap)) if ground else np.zeros((0, 4), F32)
    return A, G


def check(cm, n_cap, origin, cell, nx, ny, z_band=(-INF, INF), obstacle_height=0.3, min_points=1, ground=False, clouds=None,
          vacuous_ok=False):
    A, G = clouds if clouds is not None else host_clouds(cm, n_cap, ground)
    want, image = gr.grid_vectorised(A, G, origin, cell, nx, ny, z_band, obstacle_height, min_points)
    states = np.bincount(want["state"].ravel(), minlength=3).tolist()
    print(f"grid {nx} x {ny} cell {cell} origin {origin} band {z_band} h {obstacle_height} min {min_points}: A {len(A)} G {len(G)} "
          f"counted {int(want['n'].sum())} + {int(want['n_ground'].sum())} states {states} largest n {int(want['n'].max())}")
    if not vacuous_ok:
        holds_what_it_must(want, A, G, origin, cell, nx, ny, z_band, ground)
    got = cm.grid_map(origin, cell, nx, ny, z_band, obstacle_height, min_points)
    assert got.dtype == want.dtype and got.shape == want.shape == (ny, nx)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64).reshape(ny, nx, 4) != want.view(np.uint64).reshape(ny, nx, 4))
        iy, ix = bad[0][:2]
        raise AssertionError(f"{len(set(map(tuple, bad[:, :2].tolist())))} of {nx * ny} cells differ, first ({ix}, {iy}): "
                             f"got {got[iy, ix]} want {want[iy, ix]}")
    occ = cm.grid_occupancy()
    assert occ.dtype == np.int8 and occ.shape == (ny, nx) and occ.tobytes() == image.tobytes()
    ptr, n = cm.grid_map_device(origin, cell, nx, ny, z_band, obstacle_height, min_points)
    assert n == nx * ny and ptr
    d = np.zeros_like(want)
    assert hip_rt().hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(want.nbytes), 2) == 0
    assert d.tobytes() == want.tobytes() and cm.grid_occupancy().tobytes() == image.tobytes()
    return want, image


COARSE = dict(leaf=(0.5,) * 3, min_points_per_voxel=0)


def run_frame(cm, sensors, params):
    cm.submit_all(sensors)
    res = cm.merge_voxelize(params)
    assert res.status == capi.OK
    return res


@pytest.fixture(scope="module")
def edge_frame():
    """scene() and, on sensors 0 and 1, the hand-placed points of every HAND_GRIDS entry."""
    parts = scene(2)
    for k, (origin, cell, nx, ny) in enumerate(HAND_GRIDS):
        parts[k % 2] = np.concatenate([parts[k % 2], face_points(origin, cell, nx, ny, k % 2)])
    parts[1] = np.concatenate([parts[1], F32([[-0.0, -0.0, 0.5, 1.0], [-0.0, 0.0, 0.6, 11.0]])])
    # z = -0 and z = +0 in one cell. The transform's fp32 sum ((m20*x + m21*y) + m22*z) + t_z keeps a -0 only where every term
    # is -0: x and y negative (0 * x = -0) and a translation of -0.0, which sensor 1 gets.
    parts[1] = np.concatenate([parts[1], F32([[-40.3, -40.3, -0.0, 1.0], [-40.3, -40.3, 0.0, 11.0]])])
    n_cap = sum(len(p) for p in parts)
    sensors = clouds_of(parts)
    sensors[1].t_xyz = (0.0, 0.0, -0.0)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        run_frame(cm, sensors, MergeParams(**COARSE))
        A, G = host_clouds(cm, n_cap, False)
        assert len(A) == n_cap
        yield cm, n_cap, (A, G)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", HAND_GRIDS, ids=lambda g: f"{g[2]}x{g[3]}")
def test_faces_and_edges_of_the_hand_grids(edge_frame, grid):
    cm, n_cap, clouds = edge_frame
    origin, cell, nx, ny = grid
    for band, h, mp in (((-1.0, 2.5), 0.3, 1), ((-INF, INF), 0.0, 2)):
        want, _ = check(cm, n_cap, origin, cell, nx, ny, band, h, mp, clouds=clouds, vacuous_ok=True)
        assert want["n"].sum() >= nx + ny                               # the hand-placed points are in it
        if band[0] == -1.0:                                             # both band limits counted, one ulp outside not
            assert ((want["z_lo"] == F32(-1.0)) & (want["z_hi"] == F32(2.5))).any()
        else:
            assert ((want["z_lo"] == F32(-1.0000001)) & (want["z_hi"] == F32(2.5000002))).any()
        if nx >= 4 and origin != (0.0, 0.0):                            # a cell with only NaN intensities, one with a NaN beside finite
            assert ((want["n"] >= 2) & np.isnan(want["i_max"])).any()
            assert (want["i_max"] >= 120.0).any()


# (one cell holds everything: one state; 67 x 3 at 0.5 m, 513 x 257 at 8 cm and 80 x 80 hold all three and the hand-placed cell)
SIZES = [((-20.0, -20.0), 40.0, 1, 1), ((-15.0, 0.5), 0.5, 67, 3), ((-20.0, -10.0), 40.0 / 513, 513, 257), ((-20.0, -20.0), 0.5, 80, 80)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", SIZES, ids=lambda g: f"{g[2]}x{g[3]}")
def test_grid_sizes(edge_frame, grid):
    cm, n_cap, clouds = edge_frame
    origin, cell, nx, ny = grid
    check(cm, n_cap, origin, cell, nx, ny, clouds=clouds, vacuous_ok=(nx == 1))
    check(cm, n_cap, origin, cell, nx, ny, (-0.5, 1.5), 0.0, 2, clouds=clouds, vacuous_ok=True)


@pytest.mark.gpu
def test_minus_zero_and_an_overflowing_t(edge_frame):
    cm, n_cap, clouds = edge_frame
    A = clouds[0]
    want, _ = check(cm, n_cap, (0.0, 0.0), 0.5, 8, 8, clouds=clouds, vacuous_ok=True)
    assert want["n"][0, 0] >= 2                                         # x = -0.0f at origin 0: cell 0
    # z = -0 and z = +0 in one cell, both in the frame's own cloud: the minimum is -0, the maximum +0
    zs = A[(A[:, 0] == F32(-40.3)) & (A[:, 1] == F32(-40.3)), 2]
    assert sorted(zs.view(np.uint32).tolist()) == [0, 0x80000000]
    want, _ = check(cm, n_cap, (-41.0, -41.0), 1.0, 2, 2, clouds=clouds, vacuous_ok=True)
    assert want["n"][0, 0] == 2 and want["z_lo"][0, 0].view(np.uint32) == 0x80000000 and want["z_hi"][0, 0].view(np.uint32) == 0
    # cell 1e-37: inv is finite, t is +-inf for every point but those at the origin itself
    p = A[np.argmax(A[:, 0])]
    want, _ = check(cm, n_cap, (float(p[0]), float(p[1])), 1e-37, 2, 2, clouds=clouds, vacuous_ok=True)
    assert want["n"][0, 0] >= 1 and want["n"].sum() == want["n"][0, 0]


@pytest.mark.gpu
def test_contention_in_one_cell():
    """One cell takes every point of three sensors, 2 tiles and 100 points each; a second cell takes one point."""
    rng = np.random.default_rng(7)
    m = 2 * 4096 + 100
    parts = [tagged(np.concatenate([rng.uniform(5.0, 5.49, (m, 2)), rng.uniform(-1.0, 3.0, (m, 1))], axis=1), s, rng)
             for s in range(N_SENSORS)]
    allp = np.concatenate(parts)
    parts[2] = np.concatenate([parts[2], F32([[9.25, 9.25, 0.5, 42.0]])])
    parts[0] = np.concatenate([parts[0], F32([[2.25, 2.25, 0.1, 0.0]])])            # a FREE cell, of two sensors
    parts[1] = np.concatenate([parts[1], F32([[2.3, 2.3, 0.15, 1.0]])])
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        want, _ = check(cm, n_cap, (0.0, 0.0), 0.5, 20, 20, min_points=2)
        assert want["n"][10, 10] == 3 * m and want["n"].sum() == 3 * m + 3 and want["state"][4, 4] == gr.FREE
        assert want["z_lo"][10, 10] == allp[:, 2].min() and want["z_hi"][10, 10] == allp[:, 2].max()
        assert want["i_max"][10, 10] == allp[:, 3].max()
        one = want[18, 18]
        assert one["n"] == 1 and one["state"] == gr.UNKNOWN and one["z_lo"] == one["z_hi"] == F32(0.5) and one["i_max"] == 42.0
        # every cell of the tile's table taken: more distinct cells in a tile than the workgroup's table has slots
        check(cm, n_cap, (5.0, 5.0), 0.5 / 64, 64, 64, vacuous_ok=True)


@pytest.mark.gpu
def test_sparse_large_grid(edge_frame):
    cm, n_cap, clouds = edge_frame
    want, image = check(cm, n_cap, (-50.0, -50.0), 0.1, 1000, 1000, clouds=clouds)
    empty = (want["n"] == 0) & (want["n_ground"] == 0)
    assert empty.sum() > 990_000
    assert (want["state"][empty] == gr.UNKNOWN).all() and (image[empty] == -1).all()
    for f in ("z_lo", "z_hi", "g_lo", "g_hi", "i_max"):
        assert (want[f][empty].view(np.uint32) == NAN_BITS).all()


# ground removal: tests/test_ground.py's slabs and region, a plane with boxes on it
ROI = dict(crop_min=(-15.0, -5.0, -0.5), crop_max=(60.0, 5.0, 3.0))
FRONT = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]


def ground_scene(seed, n_per=2500):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(2):
        gx, gy = rng.uniform(-15, 60, n_per), rng.uniform(-5, 5, n_per)
        plane = np.stack([gx, gy, -0.05 + 0.01 * gx + 0.02 * gy + 0.03 * rng.standard_normal(n_per)], axis=1)
        base = np.stack([rng.uniform(-10, 55, 12), rng.uniform(-4, 4, 12)], axis=1)
        boxes = np.concatenate([np.repeat(base, 40, axis=0) + rng.uniform(0, 0.8, (480, 2)), rng.uniform(0.9, 2.4, (480, 1))], axis=1)
        boxes[:, 2] += 0.01 * boxes[:, 0]
        # by hand: in the cell around (10.25, 1.25) three points on the plane and two 1.5 m above it, per sensor
        hand = np.array([[10.2, 1.2, 0.07], [10.3, 1.3, 0.08], [10.25, 1.25, 0.075], [10.22, 1.27, 1.6], [10.28, 1.21, 1.7 + 0.01 * s]])
        out.append(tagged(np.concatenate([plane, boxes, hand]), s, rng))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("height", [0.0, 0.3])
def test_with_ground_removal(height):
    parts = ground_scene(31)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params([FRONT, FRONT]))
        run_frame(cm, clouds_of(parts), MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=1, **ROI))
        A, G = host_clouds(cm, n_cap, True)
        assert len(G) > n_cap // 2 and len(A) > 500
        want, _ = check(cm, n_cap, (-15.0, -5.0), 0.5, 150, 20, obstacle_height=height, ground=True, clouds=(A, G))
        if height == 0.0:                                                # any non-ground return occupies its cell
            assert ((want["state"] == gr.OCCUPIED) == (want["n"] > 0)).all()
        check(cm, n_cap, (-15.0, -5.0), 0.5, 150, 20, (-0.2, 1.65), height, 3, ground=True, clouds=(A, G))


@pytest.mark.gpu
def test_with_statistical_outlier_removal():
    parts = scene(4)
    parts[0] = np.concatenate([parts[0], tagged(np.random.default_rng(5).uniform(25.0, 38.0, (40, 3)), 0)])   # loose points: removed
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        cm.set_statistical_outlier(8, 0.5)
        res = run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_SOR and cm.sor_stats().n_removed > 0
        A, G = host_clouds(cm, n_cap, False)
        assert len(A) == n_cap - cm.sor_stats().n_removed
        want, _ = check(cm, n_cap, (-20.0, -20.0), 0.5, 120, 120, clouds=(A, G))
        assert want["n"].sum() == len(A) < n_cap                                     # removed points are not counted


@pytest.mark.gpu
def test_with_deskew():
    parts = scene(5)
    n_cap = sum(len(p) for p in parts)
    t_ref = 1_700_000_000_000_000_000
    m = capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000 * (s + 1) for s in range(N_SENSORS)])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        cm.set_ego_motion(m)
        res = run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_MOTION
        A, G = host_clouds(cm, n_cap, False)
        assert not np.array_equal(A[:, :3], np.concatenate(parts)[:, :3])             # the points did move
        check(cm, n_cap, (-24.0, -24.0), 2.0, 24, 24, clouds=(A, G))


@pytest.mark.gpu
def test_with_a_crop_box():
    parts = scene(6)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE, crop_min=(-10.0, -12.0, -1.0), crop_max=(12.0, 10.0, 1.2)))
        A, G = host_clouds(cm, n_cap, False)
        assert 0 < len(A) < n_cap // 2
        want, _ = check(cm, n_cap, (-20.0, -20.0), 0.5, 80, 80, clouds=(A, G))
        assert want["n"].sum() == len(A) and not want["n"][:16].any() and not want["n"][:, 65:].any()


@pytest.mark.gpu
def test_first_and_second_frame_of_a_context():
    """cfg2's moving stream at 5 cm with a crop box: the first frame takes the fixed-grid passes, the second the quantile
    pass (only a frame large enough for two bucket passes does: 150 000 points per sensor, as in tests/test_boxes.py)."""
    n_per = 150_000
    n_cap = 4 * n_per
    hand = F32([[1.05, 1.05, 0.0, 0.0], [1.06, 1.04, 1.0, 0.0], [1.04, 1.06, 0.3, 0.0]])
    seen = []
    with capi.CloudMerger(max_points_total=n_cap + 8, max_sensors=6, flags=capi.FLAG_OCCUPANCY) as cm:
        for k in range(2):
            sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
            for s in range(2):
                sensors.append(xyzi_cloud(hand[:, :3], hand[:, 3] + s))
            params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
            res = run_frame(cm, sensors, params)
            seen.append(res.path_flags)
            A, G = host_clouds(cm, n_cap + 8, False)
            # (the stream's intensities carry no sensor: only the hand-placed points are told apart, the rest is masked)
            tags = A.copy()
            tags[:-6, 3] = np.nan
            want, _ = gr.grid_vectorised(A, G, (-25.0, -25.0), 0.25, 200, 200, (-25.0, 25.0), 0.3, 1)
            holds_what_it_must(want, tags, G, (-25.0, -25.0), 0.25, 200, 200, (-25.0, 25.0), False)
            check(cm, n_cap + 8, (-25.0, -25.0), 0.25, 200, 200, (-25.0, 25.0), clouds=(A, G), vacuous_ok=True)
        assert seen[0] & capi.PATH_BUCKET and not seen[0] & capi.PATH_QUANTILE and seen[1] & capi.PATH_QUANTILE, seen


@pytest.mark.gpu
def test_growing_shrinking_repeating_and_later_frames():
    frames = [clouds_of(scene(10 + k)) for k in range(2)]
    n_cap = sum(c.n for c in frames[0])
    params = MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=1)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS, flags=capi.FLAG_OCCUPANCY) as cm, \
            capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS, flags=capi.FLAG_OCCUPANCY) as fresh:
        run_frame(cm, frames[0], params)
        run_frame(fresh, frames[0], params)
        clouds = host_clouds(cm, n_cap, False)
        small, _ = check(cm, n_cap, (-24.0, -24.0), 2.0, 24, 24, clouds=clouds)
        large, _ = check(cm, n_cap, (-24.0, -24.0), 0.125, 384, 384, clouds=clouds)           # grows
        again, _ = check(cm, n_cap, (-24.0, -24.0), 2.0, 24, 24, clouds=clouds)               # shrinks
        assert again.tobytes() == small.tobytes() and large.shape == (384, 384)
        assert cm.grid_map((-24.0, -24.0), 2.0, 24, 24).tobytes() == small.tobytes()          # repeats
        assert cm.grid_map((-24.0, -24.0), 2.0, 24, 24, obstacle_height=1.5).tobytes() != small.tobytes()
        outs = []
        for c in (cm, fresh):
            res = run_frame(c, frames[1], params)
            cells, counts = c.cells(res.n_out)
            outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes(),
                         c.merged(n_cap).tobytes()))
        assert outs[0] == outs[1]


def refused(cm, origin=(0.0, 0.0), cell=0.5, nx=8, ny=8, z_band=(-INF, INF), obstacle_height=0.3, min_points=1):
    for call in (cm.grid_map, cm.grid_map_device):
        with pytest.raises(capi.CloudMergeError) as e:
            call(origin, cell, nx, ny, z_band, obstacle_height, min_points)
        assert e.value.status == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)


def occupancy_refused(cm):
    n = C.c_uint64(99)
    buf = np.full(64, 7, np.int8)
    assert cm._lib.cm_grid_occupancy_copy(cm._ctx, buf.ctypes.data, 64, C.byref(n)) == capi.BAD_ARG
    assert n.value == 0 and (buf == 7).all() and cm._lib.cm_last_error(cm._ctx)


@pytest.mark.gpu
def test_refusals_and_capacity():
    sensors = clouds_of(scene(12))
    n_cap = sum(c.n for c in sensors)
    params = MergeParams(**COARSE)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS) as cm:
        refused(cm)                                                                # no result yet
        occupancy_refused(cm)
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        refused(cm)
        assert b"flight" in cm._lib.cm_last_error(cm._ctx)
        assert cm.wait().status == capi.OK
        occupancy_refused(cm)                                                      # no grid call yet
        for origin in ((np.nan, 0.0), (0.0, INF), (-INF, 0.0)):
            refused(cm, origin=origin)
        for cell in (0.0, -0.5, np.nan, INF, -INF, 1e-39):                         # (1e-39: finite and > 0, its fp32 inverse is inf)
            refused(cm, cell=cell)
        for nx, ny in ((0, 8), (8, 0), (2049, 2048), (2 ** 32 - 1, 2 ** 32 - 1), (2 ** 31, 2)):
            refused(cm, nx=nx, ny=ny)
        for band in ((np.nan, 1.0), (0.0, np.nan), (1.0, 0.5), (INF, -INF)):
            refused(cm, z_band=band)
        for h in (-0.1, np.nan, INF):
            refused(cm, obstacle_height=h)
        refused(cm, min_points=0)
        p = capi.CloudMerger.grid_params((0.0, 0.0), 0.5, 8, 8)
        assert cm._lib.cm_result_grid_map(cm._ctx, None, None, 0) == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)
        occupancy_refused(cm)                                                      # still no grid call that was not refused
        # what is allowed: infinite band limits, a band of one value, 2048 x 2048 cells, obstacle_height 0
        assert cm.grid_map((0.0, 0.0), 0.5, 8, 8, (-INF, INF), 0.0).shape == (8, 8)
        assert cm.grid_map((0.0, 0.0), 0.5, 8, 8, (0.5, 0.5)).shape == (8, 8)
        assert cm.grid_map((-20.0, -20.0), 0.02, 2048, 2048).shape == (2048, 2048)
        # a destination that is too small: CM_CAPACITY, nothing copied, the table and the image stay in the context
        want, image = check(cm, n_cap, (-20.0, -20.0), 0.5, 80, 80)
        out = np.zeros(6400, capi.GRID_DTYPE)
        p = capi.CloudMerger.grid_params((-20.0, -20.0), 0.5, 80, 80)
        for cap in (6399, 0):
            assert cm._lib.cm_result_grid_map(cm._ctx, C.byref(p), out.ctypes.data, cap) == capi.CAPACITY
            assert cm._lib.cm_last_error(cm._ctx) and not out.view(np.uint8).any()
            assert cm.grid_occupancy().tobytes() == image.tobytes()
        n = C.c_uint64(0)
        buf = np.full(6400, 7, np.int8)
        assert cm._lib.cm_grid_occupancy_copy(cm._ctx, buf.ctypes.data, 6399, C.byref(n)) == capi.CAPACITY
        assert n.value == 6400 and (buf == 7).all()
        assert cm._lib.cm_result_grid_map(cm._ctx, C.byref(p), out.ctypes.data, 6400) == capi.OK
        assert out.tobytes() == want.tobytes()
        # results that have no frame's clouds behind them, and the image after the next merge
        cm.submit_all(sensors)
        assert cm.merge_voxelize(MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)).status == capi.GRID_OVERFLOW
        refused(cm)
        occupancy_refused(cm)
        cm.submit_all(sensors)
        assert cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40)).status == capi.OK
        refused(cm)
        run_frame(cm, sensors, params)
        occupancy_refused(cm)                                                      # the next merge dropped the image
        check(cm, n_cap, (-20.0, -20.0), 0.5, 80, 80)


@pytest.mark.gpu
def test_stage_names_under_profile():
    sensors = clouds_of(scene(13))
    n_cap = sum(c.n for c in sensors)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=N_SENSORS, flags=capi.FLAG_PROFILE) as cm:
        run_frame(cm, sensors, MergeParams(**COARSE))
        assert not any(n.startswith("k_grid_") for n, _ in cm.stage_times())
        cm.grid_map((-20.0, -20.0), 0.5, 80, 80)
        names = [n for n, _ in cm.stage_times()]
        assert "k_grid_bin" in names and "k_grid_finish" in names and names.index("k_grid_bin") < names.index("k_grid_finish"), names
        assert all(ms >= 0.0 for _, ms in cm.stage_times())
        run_frame(cm, sensors, MergeParams(**COARSE))                    # a frame's own list never holds the call's stages
        assert not any(n.startswith("k_grid_") for n, _ in cm.stage_times())
