"""Free-space ray casting over the grid map: cm_result_grid_rays / _device, cm_grid_ray_occupancy_copy (include/cloudmerge.h,
cm_kernels_rays.hip).

The bar on the GPU: every byte of the ray table, of the cleared image and of the device-pointer variant equal to the restatement
(tests/rays_ref.py: rays_vectorised) fed with the same context's merged() and ground() host copies, the per-point sensor (the
tag tests/test_grid_map.py's scenes carry in the intensity) and the translations the sensors were given. There is no tolerance:
every quantity is an integer count over a set of distinct rays. No comparison is vacuous: rays_ref.guards is asserted on the
restatement's own output first wherever the scene can satisfy it, and test_the_scenes_satisfy_the_guards checks on the CPU
that the named seeds do."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import grid_ref as gr
from tests import rays_ref as rr
from tests import test_grid_map as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
DEVICE_H = os.path.join(ROOT, "cloud_merger_amd", "csrc", "cm_device.h")
F32 = np.float32
INF = float("inf")
NAMES = ("cm_result_grid_rays", "cm_result_grid_rays_device", "cm_grid_ray_occupancy_copy")
TRANS = [(1.2, 0.6, 1.8), (-1.2, 0.6, 1.8), (1.2, -0.6, 1.8), (-1.2, -0.6, 1.8)]
COARSE = tg.COARSE


def device_define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", open(DEVICE_H).read())
    assert m, name
    return int(m.group(1))


RAY_RUN = device_define("CM_RAY_RUN")                    # bitmap words of one k_ray_cast workgroup
RAY_HASH = 1 << device_define("CM_RAY_HASH_BITS")        # slots of its LDS table


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_ray_structs_match_header(tmp_path):
    items = ["sizeof(cm_ray_params)", "offsetof(cm_ray_params,min_pass)", "offsetof(cm_ray_params,max_range_cells)",
             "sizeof(cm_grid_ray_cell)", "offsetof(cm_grid_ray_cell,n_pass)", "offsetof(cm_grid_ray_cell,n_end)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, B = capi.RayParams, capi.GridRayCell
    want = [C.sizeof(P), P.min_pass.offset, P.max_range_cells.offset, C.sizeof(B), B.n_pass.offset, B.n_end.offset]
    assert got == want == [8, 0, 4, 8, 0, 4]
    d = capi.RAY_DTYPE
    assert d == rr.RAY_DTYPE and d.itemsize == 8 and [d.fields[f][1] for f in ("n_pass", "n_end")] == [0, 4]
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.grid_params((0.0, 0.0), 0.5, 4, 4)
    r = capi.RayParams(1, 0)
    out = np.zeros(16, capi.RAY_DTYPE)
    n = C.c_uint64(7)
    ptr = C.c_void_p()
    assert L.cm_result_grid_rays(None, C.byref(p), C.byref(r), out.ctypes.data, 16) == capi.BAD_ARG
    assert L.cm_result_grid_rays(None, None, None, None, 0) == capi.BAD_ARG
    assert L.cm_result_grid_rays_device(None, C.byref(p), None, C.byref(ptr), C.byref(n)) == capi.BAD_ARG
    assert L.cm_grid_ray_occupancy_copy(None, None, 0, C.byref(n)) == capi.BAD_ARG
    assert not out.view(np.uint8).any()


# ---- the clouds ---------------------------------------------------------------------------------------------------------
def scene(seed, n_sensors=3, n_per=1500, extent=(-20.0, 20.0)):
    """Per sensor, in its own frame: flat returns everywhere (z within 5 cm) and poles of up to 2 m on a tenth of the area; the
    sensor is in every point's intensity (tests/test_grid_map.py: tagged)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_sensors):
        flat = np.concatenate([rng.uniform(*extent, (n_per, 2)), rng.uniform(0.0, 0.05, (n_per, 1))], axis=1)
        base = rng.uniform(extent[0], extent[1], (n_per // 40, 2))
        poles = np.concatenate([np.repeat(base, 4, axis=0) + rng.uniform(0, 0.04, (len(base) * 4, 2)),
                                rng.uniform(0.0, 2.0, (len(base) * 4, 1))], axis=1)
        out.append(tg.tagged(np.concatenate([flat, poles]), s, rng))
    return out


def clouds_of(parts, trans=TRANS):
    return [xyzi_cloud(p[:, :3], p[:, 3], t_xyz=trans[s]) for s, p in enumerate(parts)]


def moved(parts, trans=TRANS):
    """What the frame makes of the parts under pure translations: fp32 x + t per component."""
    out = []
    for s, p in enumerate(parts):
        q = p.copy()
        q[:, :3] = (p[:, :3] + F32(trans[s])[None, :]).astype(F32)
        out.append(q)
    return np.concatenate(out)


def restate(A, G, trans, origin, cell, nx, ny, z_band=(-INF, INF), obstacle_height=0.3, min_points=1, min_pass=1, max_range_cells=0,
            loop=False):
    f = rr.rays_loop if loop else rr.rays_vectorised
    return f(A, G, tg.sensor_of(A), tg.sensor_of(G), [t[:2] for t in trans], origin, cell, nx, ny, z_band, obstacle_height,
             min_points, min_pass, max_range_cells)


NO_G = np.zeros((0, 4), F32)


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def test_the_two_restatements_agree():
    seen = 0
    for seed, (origin, cell, nx, ny) in enumerate([((-6.0, -6.0), 0.5, 24, 24), ((-5.0, -3.0), 0.75, 13, 9), ((-6.0, 0.0), 1.0, 12, 1),
                                                   ((0.0, -6.0), 1.0, 1, 12), ((1.0, 0.5), 1.0, 1, 1), ((2.0, -6.0), 0.25, 30, 40)]):
        parts = scene(20 + seed, 3, 120, (-6.0, 6.0))
        A = moved(parts)
        rng = np.random.default_rng(seed)
        pick = rng.random(len(A)) < 0.3
        G, A = A[pick] + F32([0.0, 0.0, -0.2, 0.0]), A[~pick]
        for band, mp, min_pass, rng_cells in (((-INF, INF), 1, 1, 0), ((1.8, 2.5), 2, 2, 0), ((-INF, INF), 1, 1, 3), ((-INF, INF), 1, 3, 1)):
            for g in (G, NO_G):
                a, ai, info = restate(A, g, TRANS[:3], origin, cell, nx, ny, band, 0.3, mp, min_pass, rng_cells)
                b, bi, info_b = restate(A, g, TRANS[:3], origin, cell, nx, ny, band, 0.3, mp, min_pass, rng_cells, loop=True)
                assert a.tobytes() == b.tobytes() and ai.tobytes() == bi.tobytes() and info["steep"] == info_b["steep"]
                assert info["base"].tobytes() == info_b["base"].tobytes()
                assert a["n_end"].sum() == info["n_rays"] and (rng_cells == 0 or a["n_pass"].sum() <= rng_cells * info["n_rays"])
                seen += info["n_rays"]
    assert seen > 2000                                                   # rays walked by both, over all cases


def one_ray(o, e, nx=5, ny=4, max_range_cells=0):
    """The n_pass table of one ray on an nx x ny grid of unit cells at the origin, by both restatements and by walk()."""
    A = F32([[e[0] + 0.5, e[1] + 0.5, 0.0, 0.0]])
    trans = [(o[0] + 0.5, o[1] + 0.5, 0.0)]
    t, _, _ = restate(A, NO_G, trans, (0.0, 0.0), 1.0, nx, ny, max_range_cells=max_range_cells)
    u, _, _ = restate(A, NO_G, trans, (0.0, 0.0), 1.0, nx, ny, max_range_cells=max_range_cells, loop=True)
    assert t.tobytes() == u.tobytes() and t["n_end"].sum() == 1 and t["n_end"][e[1], e[0]] == 1
    w = np.zeros((ny, nx), int)
    for x, y in rr.walk(o, e, max_range_cells):
        w[y, x] += 1
    assert w.tolist() == t["n_pass"].tolist()
    return t["n_pass"].tolist()


def test_known_answers_on_a_5_by_4_grid():
    # an axis-aligned ray (0,1) -> (4,1): the origin is crossed, the end is not
    assert one_ray((0, 1), (4, 1)) == [[0, 0, 0, 0, 0], [1, 1, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert one_ray((2, 3), (2, 0)) == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]
    # an exact diagonal (0,0) -> (3,3)
    assert one_ray((0, 0), (3, 3)) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    # dx = 2, dy = 1 from (1,1): k = 1 is (2, 1 + rdiv(1, 2)): the tie 1/2 goes away from zero, to row 2
    assert one_ray((1, 1), (3, 2)) == [[0, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    # dx = -2, dy = 1 from (3,1): the mirror image
    assert one_ray((3, 1), (1, 2)) == [[0, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]
    # dx = 2, dy = -1 from (1,2): the tie goes down
    assert one_ray((1, 2), (3, 1)) == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
    # dx = 4, dy = 1: rdiv(k, 4) = 0, 0, 1 (the tie at k = 2), 1
    assert one_ray((0, 0), (4, 1)) == [[1, 1, 0, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    # L = 0 crosses nothing; max_range_cells cuts the walk from the origin's end
    assert one_ray((2, 2), (2, 2)) == [[0] * 5] * 4
    assert one_ray((0, 1), (4, 1), max_range_cells=2) == [[0, 0, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert one_ray((0, 1), (4, 1), max_range_cells=9) == one_ray((0, 1), (4, 1), max_range_cells=4) == one_ray((0, 1), (4, 1))
    # two rays of two sensors to one cell, and the cleared image: the UNKNOWN cells they cross are FREE at min_pass 1, the
    # doubly crossed one alone at min_pass 2; the OCCUPIED end cell stays 100
    A = F32([[4.5, 1.5, 0.0, 0.0], [4.5, 1.5, 1.0, 1.0]])
    # (sensor 1 walks (0,3), (1,2), (2,2), (3,1): dx = 4, dy = -2, the ties at k = 1 and k = 3 go down)
    trans = [(0.5, 1.5, 0.0), (0.5, 3.5, 0.0)]
    t, img, info = restate(A, NO_G, trans, (0.0, 0.0), 1.0, 5, 4)
    assert t["n_pass"].tolist() == [[0, 0, 0, 0, 0], [1, 1, 1, 2, 0], [0, 1, 1, 0, 0], [1, 0, 0, 0, 0]]
    assert t["n_end"].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 2], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert img.tolist() == [[-1, -1, -1, -1, -1], [0, 0, 0, 0, 100], [-1, 0, 0, -1, -1], [0, -1, -1, -1, -1]]
    assert info["base_image"].tolist() == [[-1] * 5, [-1, -1, -1, -1, 100], [-1] * 5, [-1] * 5]
    _, img2, _ = restate(A, NO_G, trans, (0.0, 0.0), 1.0, 5, 4, min_pass=2)
    assert img2.tolist() == [[-1] * 5, [-1, -1, -1, 0, 100], [-1] * 5, [-1] * 5]


def test_mirroring_and_swapping_mirror_the_counts():
    """What the rounding rule buys: a half rounds away from zero on either side, so the walk has no preferred direction."""
    rng = np.random.default_rng(5)
    nx, ny = 11, 8
    ix, iy = rng.integers(0, nx, 60), rng.integers(0, ny, 60)
    s = rng.integers(0, 2, 60)
    o = [(3, 2), (9, 6)]

    def table(ix, iy, o, nx, ny):
        A = np.stack([ix + 0.5, iy + 0.5, np.zeros(len(ix)), s], axis=1).astype(F32)
        t, img, _ = restate(A, NO_G, [(x + 0.5, y + 0.5, 0.0) for x, y in o], (0.0, 0.0), 1.0, nx, ny)
        return t, img

    t, img = table(ix, iy, o, nx, ny)
    assert t["n_pass"].sum() > 200
    tx, imgx = table(nx - 1 - ix, iy, [(nx - 1 - x, y) for x, y in o], nx, ny)
    ty, imgy = table(ix, ny - 1 - iy, [(x, ny - 1 - y) for x, y in o], nx, ny)
    ts, imgs = table(iy, ix, [(y, x) for x, y in o], ny, nx)
    for f in ("n_pass", "n_end"):
        assert np.array_equal(tx[f], t[f][:, ::-1]) and np.array_equal(ty[f], t[f][::-1, :]) and np.array_equal(ts[f], t[f].T)
    assert np.array_equal(imgx, img[:, ::-1]) and np.array_equal(imgy, img[::-1]) and np.array_equal(imgs, img.T)


def test_no_ray_leaves_the_grid_or_crosses_a_cell_twice():
    nx, ny = 9, 7
    for ox in range(nx):
        for oy in range(ny):
            for ex in range(nx):
                for ey in range(ny):
                    w = rr.walk((ox, oy), (ex, ey))
                    L = max(abs(ex - ox), abs(ey - oy))
                    assert len(w) == L == len(set(w)) and (ex, ey) not in w and (L == 0 or w[0] == (ox, oy))
                    assert all(0 <= x < nx and 0 <= y < ny for x, y in w)
                    # the closed form, with Python's integers
                    rdiv = lambda a: (1 if a > 0 else -1 if a < 0 else 0) * ((2 * abs(a) + L) // (2 * L))
                    assert w == [(ox + rdiv(k * (ex - ox)), oy + rdiv(k * (ey - oy))) for k in range(L)]


# The grids of the GPU tests on scene(2) (three sensors) and scene(3, 4) (four): the guards must hold on each.
SCENE_GRIDS = [((-20.0, -20.0), 40.0 / 64, 64, 64), ((-30.0, -30.0), 0.15, 400, 400), ((-50.0, -50.0), 0.1, 1000, 1000)]


def test_the_scenes_satisfy_the_guards():
    A3, A4 = moved(scene(2)), moved(scene(3, 4))
    for origin, cell, nx, ny in SCENE_GRIDS:
        A, trans = (A4, TRANS) if nx == 400 else (A3, TRANS[:3])
        t, img, info = restate(A, NO_G, trans, origin, cell, nx, ny)
        rr.guards(t, img, info)
    for seed in (4, 5, 6, 10, 11, 12, 13):
        t, img, info = restate(moved(scene(seed)), NO_G, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96)
        rr.guards(t, img, info)
    for origin, cell, nx, ny in SHAPES[:4]:                                   # too small for the guards: they do cast
        _, _, info = restate(A3, NO_G, TRANS[:3], origin, cell, nx, ny)
        assert info["n_rays"] >= (3 if nx * ny == 1 else 6)
    t, img, info = restate(designed_cloud(), NO_G, DESIGNED_TRANS, *DESIGNED_GRIDS[0])
    assert info["ties"] > 0 and info["steep"] > 0 and info["two_sensors"] > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def run_frame(cm, sensors, params):
    return tg.run_frame(cm, sensors, params)


def check(cm, n_cap, trans, origin, cell, nx, ny, z_band=(-INF, INF), obstacle_height=0.3, min_points=1, min_pass=1, max_range_cells=0,
          ground=False, clouds=None, guard=True):
    A, G = clouds if clouds is not None else tg.host_clouds(cm, n_cap, ground)
    want, cleared, info = restate(A, G, trans, origin, cell, nx, ny, z_band, obstacle_height, min_points, min_pass, max_range_cells)
    print(f"rays {nx} x {ny} cell {cell} origin {origin} min_pass {min_pass} range {max_range_cells}: A {len(A)} G {len(G)} rays "
          f"{info['n_rays']} steps {int(want['n_pass'].sum())} largest n_pass {int(want['n_pass'].max())} ties {info['ties']} steep "
          f"{info['steep']} two-sensor cells {info['two_sensors']} image {np.bincount(cleared.ravel().astype(int) + 1, minlength=102)[[0, 1, 101]].tolist()}")
    if guard:
        rr.guards(want, cleared, info, min_pass)
    args = (origin, cell, nx, ny, z_band, obstacle_height, min_points, min_pass, max_range_cells)
    got = cm.grid_rays(*args)
    assert got.dtype == want.dtype and got.shape == want.shape == (ny, nx)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        iy, ix = bad[0][:2]
        raise AssertionError(f"{len(bad)} of {nx * ny} cells differ, first ({ix}, {iy}): got {got[iy, ix]} want {want[iy, ix]}")
    occ = cm.grid_ray_occupancy()
    assert occ.dtype == np.int8 and occ.shape == (ny, nx) and occ.tobytes() == cleared.tobytes()
    # step 1: the context's grid table and image are those of the same parameters
    assert cm.grid_occupancy().tobytes() == info["base_image"].tobytes()
    ptr, n = cm.grid_rays_device(*args)
    assert n == nx * ny and ptr
    d = np.zeros_like(want)
    assert tg.hip_rt().hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(want.nbytes), 2) == 0
    assert d.tobytes() == want.tobytes() and cm.grid_ray_occupancy().tobytes() == cleared.tobytes()
    return want, cleared, info


@pytest.fixture(scope="module")
def scene_frame():
    parts = scene(2)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        A, G = tg.host_clouds(cm, n_cap, False)
        assert len(A) == n_cap and np.array_equal(A, moved(parts))
        yield cm, n_cap, (A, G)


# 1 x 1: L = 0 for every ray. One row, one column, 3 x 2: too small for every guard. The others hold them all.
SHAPES = [((-20.0, -20.0), 45.0, 1, 1), ((-20.0, 0.5), 0.5, 83, 1), ((1.0, -20.0), 0.5, 1, 79), ((-20.0, -20.0), 15.0, 3, 2),
          SCENE_GRIDS[0], SCENE_GRIDS[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("grid", SHAPES, ids=lambda g: f"{g[2]}x{g[3]}")
def test_grid_shapes(scene_frame, grid):
    cm, n_cap, clouds = scene_frame
    origin, cell, nx, ny = grid
    want, _, info = check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, clouds=clouds, guard=nx * ny >= 4096)
    assert info["n_rays"] >= (3 if nx * ny == 1 else 6)
    if nx * ny == 1:
        assert want["n_pass"].sum() == 0 and want["n_end"][0, 0] == 3


@pytest.mark.gpu
def test_min_pass_and_range_on_the_scene(scene_frame):
    cm, n_cap, clouds = scene_frame
    origin, cell, nx, ny = SCENE_GRIDS[0]
    want, img1, _ = check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, clouds=clouds)
    top = int(want["n_pass"].max())
    _, img2, _ = check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, min_pass=2, clouds=clouds)
    _, img3, info = check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, min_pass=top + 1, clouds=clouds, guard=False)
    assert img3.tobytes() == info["base_image"].tobytes() and (img2 == 0).sum() < (img1 == 0).sum()      # nothing is cleared
    for rng_cells in (1, 7):
        w, _, info = check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, max_range_cells=rng_cells, clouds=clouds, guard=False)
        assert 0 < w["n_pass"].sum() <= rng_cells * info["n_rays"] and w["n_end"].tobytes() == want["n_end"].tobytes()
    # a band and min_points: the ray set follows the grid's counted points
    check(cm, n_cap, TRANS[:3], origin, cell, nx, ny, (1.8, 2.6), 0.0, 2, clouds=clouds, guard=False)


@pytest.mark.gpu
def test_400_by_400_on_four_sensors():
    parts = scene(3, 4)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        origin, cell, nx, ny = SCENE_GRIDS[1]
        check(cm, n_cap, TRANS, origin, cell, nx, ny)


@pytest.mark.gpu
def test_2048_by_2048_with_a_few_hundred_points():
    parts = scene(8, 3, 100)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        want, _, info = check(cm, n_cap, TRANS[:3], (-20.48, -20.48), 0.02, 2048, 2048)
        assert info["n_rays"] > 200 and want["n_pass"].sum() > 100_000


# One designed frame. Sensor 0 (translation 0, 0: exactly on a cell face of both grids) has a point in every cell of a 9 x 7
# block around it — all eight octants, the four axes, the block's corners, its own cell (L = 0) — a second point in one of them,
# and one in each corner of the larger grid. Sensor 1 (translation -0.0, -0.0) has points in five cells sensor 0 reaches too, and one
# far above the band in a cell of its own. Sensor 2's translation is outside every grid, sensor 3's is NaN (all of its points
# become NaN and are dropped): both cast nothing, and sensor 2's points are counted by the base map all the same.
DESIGNED_TRANS = [(0.0, 0.0, 0.0), (-0.0, -0.0, 0.0), (100.0, 0.0, 0.0), (np.nan, 0.0, 0.0)]
DESIGNED_GRIDS = [((-4.0, -3.0), 1.0, 9, 7), ((0.0, 0.0), 1.0, 5, 4), ((-8.0, -7.0), 1.0, 17, 13)]


def designed_parts():
    xs, ys = np.meshgrid(np.arange(-4, 5), np.arange(-3, 4))
    block = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5, np.zeros(xs.size)], axis=1)
    s0 = np.concatenate([block, [[2.25, 1.75, 1.0]], [[-7.5, -6.5, 0.0], [8.5, -6.5, 0.0], [-7.5, 5.5, 0.0], [8.5, 5.5, 0.0]]])
    s1 = np.array([[2.5, 1.5, 0.5], [-3.5, 2.5, 0.0], [0.5, 0.5, 0.0], [4.5, 3.5, 0.2], [-1.5, -2.5, 0.0], [6.5, 2.5, 50.0]])
    s2 = np.array([[1.5, 2.5, 0.1], [-2.5, 0.5, 0.1], [7.5, 4.5, 0.1]]) - np.array([100.0, 0.0, 0.0])
    s3 = np.array([[1.5, 1.5, 0.0], [2.5, 2.5, 0.0]])
    return [tg.tagged(p, s) for s, p in enumerate((s0, s1, s2, s3))]


def designed_cloud():
    A = moved(designed_parts(), DESIGNED_TRANS)
    return A[np.isfinite(A[:, 0])]


@pytest.fixture(scope="module")
def designed_frame():
    parts = designed_parts()
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=4 * 4096, max_sensors=4) as cm:
        run_frame(cm, clouds_of(parts, DESIGNED_TRANS), MergeParams(**COARSE))
        A, G = tg.host_clouds(cm, n_cap, False)
        assert len(A) == n_cap - 2 and np.array_equal(A, designed_cloud())
        yield cm, n_cap, (A, G)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", DESIGNED_GRIDS, ids=lambda g: f"{g[2]}x{g[3]}")
def test_designed_geometry(designed_frame, grid):
    cm, n_cap, clouds = designed_frame
    origin, cell, nx, ny = grid
    band = (-1.0, 5.0)
    want, cleared, info = check(cm, n_cap, DESIGNED_TRANS, origin, cell, nx, ny, band, clouds=clouds, guard=False)
    assert info["ties"] > 0 and info["two_sensors"] > 0 and (nx == 5 or info["steep"] > 0)
    o = rr.origin_cells([t[:2] for t in DESIGNED_TRANS], origin, cell, nx, ny)
    assert o[0] is not None and o[0] == o[1] and o[2] is None and o[3] is None          # the face, -0.0, outside, NaN
    ox, oy = o[0]
    assert want["n_end"][oy, ox] == 2                                                    # the end cell that is the origin cell
    assert want["n_end"].max() == 2 and info["base"]["n"].max() >= 3                     # two points of a sensor in a cell: one ray
    # sensor 2's points are counted by the map and cast nothing; sensor 1's point above the band is no ray
    assert info["base"]["n"].sum() > want["n_end"].sum()
    if nx == 9:
        assert info["n_rays"] == 63 + 5 and want["n_end"].sum() == 68 and info["base"]["n"].sum() == 64 + 5 + 2
        assert want["n_pass"][oy, ox] == 62 + 4                                          # every ray but the two of L = 0
        longest = 4
        for rng_cells in (longest - 1, longest, longest + 1, 1):
            w, _, _ = check(cm, n_cap, DESIGNED_TRANS, origin, cell, nx, ny, band, max_range_cells=rng_cells, clouds=clouds, guard=False)
            assert (w.tobytes() == want.tobytes()) == (rng_cells >= longest)
        for min_pass in (2, int(want["n_pass"].max()) + 1):
            check(cm, n_cap, DESIGNED_TRANS, origin, cell, nx, ny, band, min_pass=min_pass, clouds=clouds, guard=False)
    if nx == 17:                                                                          # a ray to each corner of the grid
        assert all(want["n_end"][y, x] == 1 for x, y in ((0, 0), (16, 0), (0, 12), (16, 12)))
    # without the band the point 50 m up is a ray of sensor 1
    w2, _, i2 = check(cm, n_cap, DESIGNED_TRANS, origin, cell, nx, ny, clouds=clouds, guard=False)
    assert i2["n_rays"] == info["n_rays"] + (1 if nx == 17 else 0)


@pytest.mark.gpu
def test_contention_and_a_full_lds_table():
    """25 000 points of one sensor in distinct cells of a 160 x 160 grid, the sensor in the middle: every ray crosses the origin
    cell. The first run of bitmap words (CM_RAY_RUN * 32 cells, 6.4 rows at the far edge) is full, and its rays cross more
    distinct cells than the workgroup's table has slots."""
    nx = ny = 160
    o = (80, 80)
    cells = np.array([c for c in range(nx * ny) if c != o[0] + o[1] * nx][:25_000])
    pts = np.stack([cells % nx + 0.5, cells // nx + 0.5, np.zeros(len(cells))], axis=1)
    rng = np.random.default_rng(9)
    trans = [(80.5, 80.5, 0.0)]
    common = tg.tagged(pts[rng.permutation(len(pts))], 0)
    parts = [common - F32([80.5, 80.5, 0.0, 0.0])]                                 # (exact in fp32, and so is the way back)
    assert np.array_equal(moved(parts, trans), common)
    run_cells = RAY_RUN * 32
    sub = common[np.isin((common[:, 0].astype(int) + common[:, 1].astype(int) * nx), np.arange(run_cells))]
    t_sub, _, _ = restate(sub, NO_G, trans, (0.0, 0.0), 1.0, nx, ny)
    assert len(sub) == run_cells and int((t_sub["n_pass"] > 0).sum()) > RAY_HASH, (int((t_sub["n_pass"] > 0).sum()), RAY_HASH)
    with capi.CloudMerger(max_points_total=len(cells), max_sensors=1) as cm:
        run_frame(cm, clouds_of(parts, trans), MergeParams(**COARSE))
        want, _, info = check(cm, len(cells), trans, (0.0, 0.0), 1.0, nx, ny, guard=False)
        assert info["n_rays"] == 25_000 == want["n_pass"][o[1], o[0]] and want["n_end"].max() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("height", [0.0, 0.3])
def test_with_ground_removal(height):
    parts = tg.ground_scene(31)
    trans = [(1.2, 0.6, 0.0), (-1.2, -0.6, 0.0)]
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params([tg.FRONT, tg.FRONT]))
        run_frame(cm, clouds_of(parts, trans), MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=1, **tg.ROI))
        A, G = tg.host_clouds(cm, n_cap, True)
        assert len(G) > n_cap // 4 and len(A) > 500
        want, _, info = check(cm, n_cap, trans, (-15.0, -5.0), 0.5, 150, 20, obstacle_height=height, ground=True, clouds=(A, G))
        # ground points cast: cells that hold ground returns only are end cells
        only_g = (info["base"]["n"] == 0) & (info["base"]["n_ground"] > 0)
        assert only_g.any() and (want["n_end"][only_g] > 0).all()
        _, _, without = restate(A, NO_G, trans, (-15.0, -5.0), 0.5, 150, 20, obstacle_height=height)
        assert without["n_rays"] < info["n_rays"]


@pytest.mark.gpu
def test_with_statistical_outlier_removal():
    parts = scene(4)
    loose = np.random.default_rng(5).uniform(24.0, 36.0, (40, 3))
    parts[0] = np.concatenate([parts[0], tg.tagged(loose, 0)])                             # loose points: removed, no ray
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        cm.set_statistical_outlier(8, 0.5)
        res = run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_SOR and cm.sor_stats().n_removed > 0
        A, G = tg.host_clouds(cm, n_cap, False)
        assert len(A) == n_cap - cm.sor_stats().n_removed
        want, _, info = check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.5, 128, 128, clouds=(A, G))
        everything = moved(parts)
        _, _, with_removed = restate(everything, NO_G, TRANS[:3], (-24.0, -24.0), 0.5, 128, 128)
        assert with_removed["n_rays"] > info["n_rays"]                                     # a removed point would have been a ray


@pytest.mark.gpu
def test_with_deskew():
    """The points move with the ego-motion; the origins stay the translations that were set."""
    parts = scene(5)
    n_cap = sum(len(p) for p in parts)
    t_ref = 1_700_000_000_000_000_000
    m = capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000 * (s + 1) for s in range(3)])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        cm.set_ego_motion(m)
        res = run_frame(cm, clouds_of(parts), MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_MOTION
        A, G = tg.host_clouds(cm, n_cap, False)
        assert not np.array_equal(A[:, :3], moved(parts)[:, :3])                           # the points did move
        check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96, clouds=(A, G))
        # an origin of the identity the descriptor carries under deskew would be another table
        a, _, _ = restate(A, G, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96)
        b, _, _ = restate(A, G, [(0.0, 0.0, 0.0)] * 3, (-24.0, -24.0), 0.5, 96, 96)
        assert a.tobytes() != b.tobytes()


@pytest.mark.gpu
def test_with_a_crop_box():
    parts = scene(6)
    n_cap = sum(len(p) for p in parts)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        run_frame(cm, clouds_of(parts), MergeParams(**COARSE, crop_min=(-10.0, -12.0, -1.0), crop_max=(12.0, 10.0, 5.0)))
        A, G = tg.host_clouds(cm, n_cap, False)
        assert 0 < len(A) < n_cap // 2
        want, _, _ = check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96, clouds=(A, G))
        assert not want["n_end"][:24].any() and not want["n_pass"][:, 72:].any()


@pytest.mark.gpu
def test_frames_of_a_context_growing_shrinking_and_what_stays_untouched():
    frames = [clouds_of(scene(10 + k)) for k in range(2)]
    n_cap = sum(c.n for c in frames[0])
    params = MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=1)
    grid = ((-24.0, -24.0), 0.5, 96, 96)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_OCCUPANCY) as cm, \
            capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_OCCUPANCY) as never:
        run_frame(cm, frames[0], params)
        run_frame(never, frames[0], params)
        clouds = tg.host_clouds(cm, n_cap, False)
        small, small_img, _ = check(cm, n_cap, TRANS[:3], *grid, clouds=clouds)                              # the first frame
        large, _, _ = check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.125, 384, 384, clouds=clouds)           # grows
        again, again_img, _ = check(cm, n_cap, TRANS[:3], *grid, clouds=clouds)                              # shrinks
        assert again.tobytes() == small.tobytes() and again_img.tobytes() == small_img.tobytes() and large.shape == (384, 384)
        assert cm.grid_rays(*grid).tobytes() == small.tobytes()                                               # repeats
        assert cm.grid_rays(*grid, min_pass=3).tobytes() == small.tobytes()
        assert cm.grid_ray_occupancy().tobytes() != small_img.tobytes()
        # the grid map after a ray call: the bytes of a context that never cast rays; and a grid call drops the ray image
        assert cm.grid_map(*grid).tobytes() == never.grid_map(*grid).tobytes()
        assert cm.grid_occupancy().tobytes() == never.grid_occupancy().tobytes()
        ray_image_refused(cm)
        cm.grid_rays(*grid)
        # the frame after a ray call: byte for byte that of such a context
        outs = []
        for c in (cm, never):
            res = run_frame(c, frames[1], params)
            cells, counts = c.cells(res.n_out)
            outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes(),
                         c.merged(n_cap).tobytes()))
        assert outs[0] == outs[1]
        ray_image_refused(cm)                                                                                  # the merge dropped it
        check(cm, n_cap, TRANS[:3], *grid)                                                                     # the second frame
        assert cm.grid_map(*grid).tobytes() == never.grid_map(*grid).tobytes()


def refused(cm, origin=(0.0, 0.0), cell=0.5, nx=8, ny=8, z_band=(-INF, INF), obstacle_height=0.3, min_points=1, min_pass=1):
    for call in (cm.grid_rays, cm.grid_rays_device):
        with pytest.raises(capi.CloudMergeError) as e:
            call(origin, cell, nx, ny, z_band, obstacle_height, min_points, min_pass)
        assert e.value.status == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)


def ray_image_refused(cm):
    n = C.c_uint64(99)
    buf = np.full(64, 7, np.int8)
    assert cm._lib.cm_grid_ray_occupancy_copy(cm._ctx, buf.ctypes.data, 64, C.byref(n)) == capi.BAD_ARG
    assert n.value == 0 and (buf == 7).all() and cm._lib.cm_last_error(cm._ctx)


@pytest.mark.gpu
def test_refusals_and_capacity():
    parts = scene(12)
    sensors = clouds_of(parts)
    n_cap = sum(c.n for c in sensors)
    params = MergeParams(**COARSE)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        refused(cm)                                                                # no result yet
        ray_image_refused(cm)
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        refused(cm)
        assert b"flight" in cm._lib.cm_last_error(cm._ctx)
        assert cm.wait().status == capi.OK
        ray_image_refused(cm)                                                      # no ray call yet
        cm.grid_map((0.0, 0.0), 0.5, 8, 8)
        ray_image_refused(cm)                                                      # a grid call is not one
        for origin in ((np.nan, 0.0), (0.0, INF), (-INF, 0.0)):
            refused(cm, origin=origin)
        for cell in (0.0, -0.5, np.nan, INF, -INF, 1e-39):
            refused(cm, cell=cell)
        for nx, ny in ((0, 8), (8, 0), (2049, 2048), (2 ** 32 - 1, 2 ** 32 - 1), (2 ** 31, 2)):
            refused(cm, nx=nx, ny=ny)
        for band in ((np.nan, 1.0), (0.0, np.nan), (1.0, 0.5), (INF, -INF)):
            refused(cm, z_band=band)
        for h in (-0.1, np.nan, INF):
            refused(cm, obstacle_height=h)
        refused(cm, min_points=0)
        refused(cm, min_pass=0)
        assert b"min_pass" in cm._lib.cm_last_error(cm._ctx)
        p = capi.CloudMerger.grid_params((-24.0, -24.0), 0.5, 96, 96)
        assert cm._lib.cm_result_grid_rays(cm._ctx, None, None, None, 0) == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)
        ray_image_refused(cm)                                                      # still no ray call that was not refused
        # NULL ray parameters are {1, 0}
        want, cleared, _ = check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96)
        out = np.zeros(96 * 96, capi.RAY_DTYPE)
        assert cm._lib.cm_result_grid_rays(cm._ctx, C.byref(p), None, out.ctypes.data, 96 * 96) == capi.OK
        assert out.tobytes() == want.tobytes() and cm.grid_ray_occupancy().tobytes() == cleared.tobytes()
        # a destination that is too small: CM_CAPACITY, nothing copied, the tables stay in the context
        out[:] = 0
        r = capi.RayParams(1, 0)
        for cap in (96 * 96 - 1, 0):
            assert cm._lib.cm_result_grid_rays(cm._ctx, C.byref(p), C.byref(r), out.ctypes.data, cap) == capi.CAPACITY
            assert cm._lib.cm_last_error(cm._ctx) and not out.view(np.uint8).any()
            assert cm.grid_ray_occupancy().tobytes() == cleared.tobytes()
        n = C.c_uint64(0)
        buf = np.full(96 * 96, 7, np.int8)
        assert cm._lib.cm_grid_ray_occupancy_copy(cm._ctx, buf.ctypes.data, 96 * 96 - 1, C.byref(n)) == capi.CAPACITY
        assert n.value == 96 * 96 and (buf == 7).all()
        # results that have no frame's clouds behind them, and the image after the next merge
        cm.submit_all(sensors)
        assert cm.merge_voxelize(MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)).status == capi.GRID_OVERFLOW
        refused(cm)
        ray_image_refused(cm)
        cm.submit_all(sensors)
        assert cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40)).status == capi.OK
        refused(cm)
        run_frame(cm, sensors, params)
        ray_image_refused(cm)
        check(cm, n_cap, TRANS[:3], (-24.0, -24.0), 0.5, 96, 96)


@pytest.mark.gpu
def test_stage_names_under_profile():
    sensors = clouds_of(scene(13))
    n_cap = sum(c.n for c in sensors)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3, flags=capi.FLAG_PROFILE) as cm:
        run_frame(cm, sensors, MergeParams(**COARSE))
        assert not any("ray" in n for n, _ in cm.stage_times())
        cm.grid_map((-24.0, -24.0), 0.5, 96, 96)
        assert not any("ray" in n for n, _ in cm.stage_times())
        cm.grid_rays((-24.0, -24.0), 0.5, 96, 96)
        names = [n for n, _ in cm.stage_times()]
        order = ["grid_clear", "k_grid_bin", "k_grid_finish", "ray_clear", "k_ray_mark", "k_ray_cast", "k_ray_finish"]
        assert [n for n in names if n in order] == order, names
        assert all(ms >= 0.0 for _, ms in cm.stage_times())
        run_frame(cm, sensors, MergeParams(**COARSE))                    # a frame's own list never holds the call's stages
        assert not any("ray" in n or n.startswith("k_grid_") for n, _ in cm.stage_times())
