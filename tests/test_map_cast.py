"""The cast layer: cm_map_cast_configure, cm_map_cast_evaluate, cm_map_cast_evaluate_mcl, cm_map_cast_copy, cm_map_cast_device,
cm_cast_directions (include/cloudmerge.h, cm_kernels_cast.hip).

The bar on the GPU: every byte of the rays, of the device-pointer variant and every field of the info equal to the restatement
(tests/cast_ref.py, the plain walk with Python's integer division) fed with the library's own image, map info and
traj_directions(), in both modes of the device walk (the default, which skips by the distance field, and CM_CAST_PLAIN). There
is no tolerance. Maps are put in place with cm_map_load and cm_map_cost_update: no frames are needed. On the CPU the skip rule
is run against the plain walk exhaustively on small windows and the kernel's quotient without a division against Python's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi
from tests import cast_ref as kr
from tests import map_ref as mpr
from tests import test_grid_map as tg
from tests import test_map_match as tmm
from tests import test_occupancy_map as tm
from tests import traj_ref as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
NAMES = ("cm_map_cast_configure", "cm_map_cast_evaluate", "cm_map_cast_evaluate_mcl", "cm_map_cast_copy", "cm_map_cast_device", "cm_cast_directions")
CAST_TYPES = (capi.CastParams, capi.CastInfo)        # (a library without the layer fails every test here, at import)
F32 = np.float32
CELL = tmm.CELL
NX, NY = tmm.NX, tmm.NY                              # 96 x 80
MQ = mpr.params(CELL, NX, NY)
ANCHOR = tmm.anchor_of(NX, NY)
INFO = ("n_poses", "n_bearings", "n_max", "n_hit", "n_off_map", "n_no_origin")


def q_of(max_poses=64, n_bearings=64, range_cells=40, flags=0):
    return dict(max_poses=max_poses, n_bearings=n_bearings, range_cells=range_cells, flags=flags)


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_cast_structs_and_constants_match_header(tmp_path):
    structs = {"cm_cast_params": (capi.CastParams, ["max_poses", "n_bearings", "range_cells", "flags"]),
               "cm_cast_info": (capi.CastInfo, list(INFO))}
    names = ["CM_CAST_MAX_POSES", "CM_CAST_MAX_BEARINGS", "CM_CAST_MAX_RANGE_CELLS", "CM_CAST_MAX_RAYS", "CM_CAST_PLAIN", "CM_CAST_MAX", "CM_CAST_HIT",
             "CM_CAST_OFF_MAP", "CM_CAST_NO_ORIGIN"]
    items, want = [], []
    for s, (T, fields) in structs.items():
        items += [f"sizeof({s})"] + [f"offsetof({s},{f})" for f in fields]
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    for s, dt in (("cm_cast_pose", capi.CAST_POSE_DTYPE), ("cm_cast_ray", capi.CAST_RAY_DTYPE)):
        items += [f"sizeof({s})"] + [f"offsetof({s},{f})" for f in dt.names]
        want += [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%llu ",(unsigned long long)({it}));' for it in items + names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(want)] == want
    assert want == [16, 0, 4, 8, 12, 24, 0, 4, 8, 12, 16, 20, 12, 0, 4, 8, 8, 0, 2, 3, 4, 6]
    assert got[len(want):] == [capi.CAST_MAX_POSES, capi.CAST_MAX_BEARINGS, capi.CAST_MAX_RANGE_CELLS, capi.CAST_MAX_RAYS, capi.CAST_PLAIN, capi.CAST_MAX,
                               capi.CAST_HIT, capi.CAST_OFF_MAP, capi.CAST_NO_ORIGIN]
    assert got[len(want):] == [kr.MAX_POSES, kr.MAX_BEARINGS, kr.MAX_RANGE_CELLS, kr.MAX_RAYS, kr.PLAIN, kr.S_MAX, kr.S_HIT, kr.S_OFF_MAP, kr.S_NO_ORIGIN]
    assert got[len(want):] == [65536, 4096, 1024, 1 << 24, 1, 0, 1, 2, 3]
    assert kr.POSE == capi.CAST_POSE_DTYPE and kr.RAY == capi.CAST_RAY_DTYPE
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.CastParams(4, 4, 4, 0)
    info = capi.CastInfo(9, 9, 9, 9, 9, 9)
    before = bytes(info)
    rays = np.full(16, 7, capi.CAST_RAY_DTYPE)
    poses = np.zeros(4, capi.CAST_POSE_DTYPE)
    keep = rays.tobytes()
    a = C.c_void_p(5)
    assert L.cm_map_cast_configure(None, C.byref(p), None) == capi.BAD_ARG and L.cm_map_cast_configure(None, None, None) == capi.BAD_ARG
    assert L.cm_map_cast_evaluate(None, poses.ctypes.data, 4, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cast_evaluate_mcl(None, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cast_copy(None, rays.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cast_device(None, C.byref(a), C.byref(info)) == capi.BAD_ARG
    assert rays.tobytes() == keep and bytes(info) == before and a.value == 5


@pytest.mark.parametrize("range_cells", [1, 2, 255, 1024])
def test_the_direction_table_against_the_restatement(range_cells):
    got, want = capi.cast_directions(range_cells), kr.directions(range_cells, tj.table())
    assert got.dtype == np.int16 and got.shape == (4096, 2) and got.tobytes() == want.tobytes()
    assert np.asarray(capi.traj_directions()).tobytes() == np.asarray(tj.table(), F32).tobytes()
    L = np.abs(got.astype(np.int64)).max(axis=1)
    assert L.min() >= 1 and L.max() == range_cells and np.abs(got).max() <= range_cells
    assert got[0].tolist() == [range_cells, 0] and got[1024].tolist() == [0, range_cells] and got[2048].tolist() == [-range_cells, 0]
    assert got[512, 0] == got[512, 1] and (got[2048:] == -got[:2048]).all()


def test_the_direction_table_refusals():
    L = capi.load()
    buf = np.full((4096, 2), 7, np.int16)
    assert L.cm_cast_directions(0, buf.ctypes.data, 4096) == capi.BAD_ARG and L.cm_cast_directions(1025, buf.ctypes.data, 4096) == capi.BAD_ARG
    assert L.cm_cast_directions(5, None, 4096) == capi.BAD_ARG and L.cm_cast_directions(5, buf.ctypes.data, 4095) == capi.CAPACITY
    assert (buf == 7).all()


def test_refusals_of_the_restatement():
    assert kr.refusal(q_of()) is None
    for kw in REFUSED_PARAMS:
        assert kr.refusal(q_of(**kw)) is not None, kw
    for kw in ACCEPTED_PARAMS:
        assert kr.refusal(q_of(**kw)) is None, kw


REFUSED_PARAMS = [dict(max_poses=0), dict(max_poses=65537), dict(n_bearings=0), dict(n_bearings=4097), dict(range_cells=0), dict(range_cells=1025),
                  dict(max_poses=4097, n_bearings=4096), dict(max_poses=65536, n_bearings=257), dict(flags=2), dict(flags=1 << 31), dict(flags=3)]
ACCEPTED_PARAMS = [dict(max_poses=1), dict(max_poses=65536, n_bearings=256), dict(max_poses=4096, n_bearings=4096), dict(n_bearings=1), dict(range_cells=1),
                   dict(range_cells=1024), dict(flags=1)]


# ---- CPU: the skip rule against the plain walk, exhaustively ---------------------------------------------------------------------
def small_windows():
    rng = np.random.default_rng(3)
    empty = np.full((20, 24), -1, np.int8)
    single = empty.copy()
    single[7, 13] = 100
    dense = np.where(rng.random((20, 24)) < 0.2, 100, np.where(rng.random((20, 24)) < 0.5, 0, -1)).astype(np.int8)
    sparse = np.where(rng.random((17, 9)) < 0.04, 100, 0).astype(np.int8)
    row = np.where(rng.random((1, 24)) < 0.1, 100, -1).astype(np.int8)
    walls = np.zeros((12, 19), np.int8)
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = 100
    walls[1:8, 9] = 100
    return dict(empty=empty, single=single, dense=dense, sparse=sparse, row=row, walls=walls)


@pytest.mark.parametrize("name", list(small_windows()))
@pytest.mark.parametrize("range_cells", [1, 7, 40])
def test_the_skip_rule_against_the_plain_walk_exhaustively(name, range_cells):
    """Every origin of the window and every one of the 4096 entries: entries with equal (dx, dy) are one ray, so the distinct
    pairs are walked and every entry is compared through its pair. The capped rule (the device's byte table) rides along."""
    image = small_windows()[name]
    ny, nx = image.shape
    E = kr.directions(range_cells, tj.table()).astype(np.int64)
    pairs, inverse = np.unique(E, axis=0, return_inverse=True)
    assert len(pairs[inverse.reshape(-1)]) == 4096 and (pairs[inverse.reshape(-1)] == E).all()
    oy, ox = (v.reshape(-1) for v in np.mgrid[0:ny, 0:nx])
    OX, OY = np.repeat(ox, len(pairs)), np.repeat(oy, len(pairs))
    DX, DY = np.tile(pairs[:, 0], len(ox)), np.tile(pairs[:, 1], len(ox))
    dist2 = kr.dist2_of(image)
    plain = kr.walk_plain(image, OX, OY, DX, DY)
    for cap in (None, 255, 3):
        skip = kr.walk_skip(image, dist2, OX, OY, DX, DY, cap)
        for a, b in zip(plain[:4], skip[:4]):
            assert (a == b).all()
        assert (skip[4] <= plain[4]).all()
    print(f"{name} range {range_cells}: {len(OX)} rays, reads per ray plain {plain[4].mean():.2f} skip {kr.walk_skip(image, dist2, OX, OY, DX, DY)[4].mean():.2f}")
    if name == "empty":
        assert set(plain[1].tolist()) <= {kr.S_MAX, kr.S_OFF_MAP}
    if name == "single":
        assert (plain[1] == kr.S_HIT).sum() > 0 and ((plain[1] == kr.S_HIT) == ((OX + plain[2] == 13) & (OY + plain[3] == 7))).all()


# ---- CPU: the kernel's quotient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_the_quotient_without_a_division_on_a_strided_sweep(ulps):
    """rdiv(k * d, L) = (2 k d + L) div 2 L by one fp32 product and one correction (cm_cast_math.hpp), for every L <= 1024 with k
    and d on strides, with the reciprocal as rounded and one unit either side (the hardware's is within one unit)."""
    for L in range(1, 1025):
        d = np.unique(np.concatenate([np.arange(0, L + 1, 13), [min(1, L), max(L - 1, 0), L]]))
        k = np.unique(np.concatenate([np.arange(0, L + 1, 3), [L]]))
        K, D = np.meshgrid(k, d)
        assert (kr.minor_cell(K, D, L, ulps) == (2 * K * D + L) // (2 * L)).all(), L


@pytest.mark.parametrize("L", [1, 2, 3, 1023, 1024])
@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_the_quotient_next_to_every_multiple(L, ulps):
    """All (k, d) with 2 k d + L within 2 of a multiple of 2 L: where a rounding error in the product could change the floor."""
    K, D = np.meshgrid(np.arange(L + 1), np.arange(L + 1))
    m = (2 * K * D + L) % (2 * L)
    near = (m <= 2) | (m >= 2 * L - 2)
    assert near.sum() >= 2
    assert (kr.minor_cell(K[near], D[near], L, ulps) == (2 * K[near] * D[near] + L) // (2 * L)).all()
    # and the other divisions of the kernel: the last step inside the window and the pose of a ray index
    n = np.arange(0, 1 << 21, 61)
    for d in (2, 2 * L, 2 * L - 1 if L > 1 else 3):
        rd = (F32(1.0) / F32(d)).astype(F32) if ulps == 0 else np.nextafter(F32(1.0) / F32(d), F32(np.inf if ulps > 0 else -np.inf))
        assert (kr.quot(n, d, rd) == n // d).all()
    r = np.concatenate([np.arange(0, 1 << 24, 4099), [(1 << 24) - 1]])
    for nb in (1, 63, 64, 65, 360, 4095, 4096):
        rd = F32(1.0) / F32(nb)
        rd = rd if ulps == 0 else np.nextafter(rd, F32(np.inf if ulps > 0 else -np.inf))
        sel = r // nb < 65536
        assert (kr.quot(r[sel], nb, rd) == r[sel] // nb).all()


# ---- CPU: a room by hand ---------------------------------------------------------------------------------------------------------
def test_a_room_by_hand():
    """A closed room of 10 x 10 cells: walls on x, y = 0 and 9, the pose in cell (3, 5), range_cells 20. The four axis rays
    run 20 cells and the diagonals rint(20 * 0.70710677) = 14; every one meets a wall first."""
    image = np.zeros((10, 10), np.int8)
    image[0, :] = image[9, :] = image[:, 0] = image[:, 9] = 100
    anchor = (-5, -5)
    pose = kr.poses_of([((anchor[0] + 3 + 0.5) * 0.5, (anchor[1] + 5 + 0.5) * 0.5, 0)])
    bearings = [e << 20 for e in (0, 1024, 2048, 3072, 512, 1536, 2560, 3584)]
    rays, info = kr.cast(image, 0.5, anchor, q_of(1, 8, 20), bearings, pose, tj.table())
    want = [(6, 1, 6, 0),                              # +x: the wall x = 9 is 6 cells away
            (4, 1, 0, 4),                              # +y: the wall y = 9
            (3, 1, -3, 0),                             # -x: the wall x = 0
            (5, 1, 0, -5),                             # -y: the wall y = 0
            (4, 1, 4, 4),                              # +x+y: (7, 9) on the wall y = 9
            (3, 1, -3, 3),                             # -x+y: (0, 8) on the wall x = 0
            (3, 1, -3, -3),                            # -x-y: (0, 2)
            (5, 1, 5, -5)]                             # +x-y: (8, 0)
    assert [(int(r["k"]), int(r["status"]), int(r["jx"]), int(r["jy"])) for r in rays[0]] == want
    assert info == dict(n_poses=1, n_bearings=8, n_max=0, n_hit=8, n_off_map=0, n_no_origin=0)
    assert kr.ranges(rays, 0.5)[0, :4].tolist() == [3.0, 2.0, 1.5, 2.5]
    # the same pose without the room: the axis rays leave the window, one step before the first cell outside
    rays, info = kr.cast(np.full((10, 10), -1, np.int8), 0.5, anchor, q_of(1, 8, 20), bearings, pose, tj.table())
    assert [(int(r["k"]), int(r["status"])) for r in rays[0]] == [(6, 2), (4, 2), (3, 2), (5, 2), (4, 2), (3, 2), (3, 2), (5, 2)]
    # and with range_cells 3 every ray ends at its last step
    rays, info = kr.cast(np.full((10, 10), -1, np.int8), 0.5, anchor, q_of(1, 8, 3), bearings, pose, tj.table())
    assert [(int(r["k"]), int(r["status"]), int(r["jx"]), int(r["jy"])) for r in rays[0]][:5] == [(3, 0, 3, 0), (3, 0, 0, 3), (3, 0, -3, 0), (3, 0, 0, -3), (2, 0, 2, 2)]


# ---- GPU ------------------------------------------------------------------------------------------------------------------
_tab = []


def TAB():
    if not _tab:
        _tab.append(capi.traj_directions())
    return _tab[0]


def table_of(image, q=MQ):
    """A state table whose image (the map's step 8) is `image`."""
    t = np.zeros(image.shape, capi.MAP_DTYPE)
    t["logodds"] = np.where(image == 100, q["l_occ"], np.where(image == 0, q["l_free"], 0))
    t["n_obs"] = (image != -1).astype(np.uint32)
    return t


def load(cm, image, anchor=ANCHOR, q=MQ):
    cm.map_load(table_of(image, q), anchor)
    cm.map_cost_update()
    got, info = cm.map_occupancy()
    assert got.tobytes() == image.astype(np.int8).tobytes() and tuple(info.anchor) == tuple(anchor)


def world(ix, iy, anchor=ANCHOR, cell=CELL):
    """The centre of window cell (ix, iy) in the world frame."""
    return ((anchor[0] + ix + 0.5) * cell, (anchor[1] + iy + 0.5) * cell)


def pose_rows(cells, hs, anchor=ANCHOR, cell=CELL):
    return kr.poses_of([world(ix, iy, anchor, cell) + (h,) for (ix, iy), h in zip(cells, hs)])


def check(cm, q, bearings, poses, cell=CELL):
    """One evaluate in both modes against the restatement: rays, device pointer, info. Returns the restatement's rays."""
    image, minfo = cm.map_occupancy()
    want, winfo = kr.cast(image, cell, tuple(minfo.anchor), q, bearings, poses, TAB())
    for plain in (False, True):
        cm.map_cast_configure(q["max_poses"], q["n_bearings"], q["range_cells"], plain, bearings)
        info = cm.map_cast(poses)
        got, i1 = cm.map_cast_rays()
        ptr, i2 = cm.map_cast_device()
        assert bytes(info) == bytes(i1) == bytes(i2)
        for f in INFO:
            assert getattr(info, f) == winfo[f], (plain, f, getattr(info, f), winfo[f])
        if got.tobytes() != want.tobytes():
            bad = np.argwhere(got != want)
            p, a = bad[0]
            raise AssertionError(f"plain {plain}: {len(bad)} of {got.size} rays differ, first pose {p} bearing {a}: got {got[p, a]} want {want[p, a]}")
        dev = np.zeros_like(got)
        assert ptr and tg.hip_rt().hipMemcpy(C.c_void_p(dev.ctypes.data), C.c_void_p(ptr), C.c_size_t(dev.nbytes), 2) == 0
        assert dev.tobytes() == want.tobytes()
        names = [n for n, _ in cm.stage_times()]
        assert names[0] == "cast_upload" and names[-1] == "k_cast_rays" and set(names) <= {"cast_upload", "k_cast_steps", "k_cast_rays"}
        assert ("k_cast_steps" in names) == (not plain)    # (the first evaluate after a configure call builds the table)
    return want


def room_image():
    """Outer walls 4..91 x 4..75, an inner wall at x = 40 with a doorway of one cell at y = 30, free inside, unknown outside."""
    img = np.full((NY, NX), -1, np.int8)
    img[5:75, 5:91] = 0
    img[4, 4:92] = img[75, 4:92] = 100
    img[4:76, 4] = img[4:76, 91] = 100
    img[5:75, 40] = 100
    img[30, 40] = 0
    return img


def random_image(pct, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((NY, NX)) * 100 < pct, 100, np.where(rng.random((NY, NX)) < 0.5, 0, -1)).astype(np.int8)


def random_poses(n, seed, margin=3):
    """Poses anywhere in the window and up to `margin` cells beyond its edges, off the cell centres, any heading."""
    rng = np.random.default_rng(seed)
    x = (ANCHOR[0] + rng.uniform(-margin, NX + margin, n)) * CELL
    y = (ANCHOR[1] + rng.uniform(-margin, NY + margin, n)) * CELL
    return kr.poses_of(list(zip(x, y, rng.integers(0, 1 << 32, n))))


@pytest.fixture(scope="module")
def ctx():
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        tm.configure(cm, MQ)
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        yield cm


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["room", 0, 1, 5, 20])
def test_rooms_and_random_maps(ctx, scene):
    load(ctx, room_image() if scene == "room" else random_image(scene, 40 + scene))
    want = check(ctx, q_of(300, 64, 60), None, random_poses(300, 7))
    st = want["status"]
    assert (st == kr.S_NO_ORIGIN).any() and (st == kr.S_OFF_MAP).any()
    assert (st == kr.S_HIT).any() == (scene != 0) and ((st == kr.S_MAX).any() or scene == 20)
    if scene == "room":                                # through the doorway and nowhere else: a ray along y = 30 from the left room ends on the far wall
        ray = check(ctx, q_of(2, 1, 80), [0], pose_rows([(10, 30), (10, 31)], [0, 0]))
        assert [(int(r["k"]), int(r["status"])) for r in ray[:, 0]] == [(80, kr.S_MAX), (30, kr.S_HIT)]
        ray = check(ctx, q_of(1, 1, 100), [0], pose_rows([(10, 30)], [0]))
        assert (int(ray[0, 0]["k"]), int(ray[0, 0]["status"]), int(ray[0, 0]["jx"])) == (81, kr.S_HIT, 81)


@pytest.mark.gpu
@pytest.mark.parametrize("range_cells", [1, 37, 1024])
def test_all_headings_from_one_pose(ctx, range_cells):
    load(ctx, room_image())
    every = [e << 20 for e in range(4096)]
    want = check(ctx, q_of(1, 4096, range_cells), every, pose_rows([(60, 33)], [0]))
    assert ((want["status"] == kr.S_HIT).all() if range_cells == 1024 else (want["status"] == kr.S_MAX).any())
    load(ctx, random_image(1, 9))
    check(ctx, q_of(2, 4096, range_cells), every, pose_rows([(47, 41), (0, 79)], [0x7FFFF, 0x80000]))


@pytest.mark.gpu
def test_skip_ties_on_the_diagonal(ctx):
    """A lone occupied cell at (j, j) from the origin on the exact diagonal: dist2 at the origin is exactly 2 j^2 and the
    smallest j with 2 j^2 >= dist2 lands on it."""
    assert capi.cast_directions(40)[512].tolist() == [28, 28]
    for j in (1, 2, 3, 11):
        img = np.zeros((NY, NX), np.int8)
        img[20 + j, 30 + j] = 100
        load(ctx, img)
        assert ctx.map_cost()[1][20, 30] == 2 * j * j
        want = check(ctx, q_of(1, 2, 40), [512 << 20, 2560 << 20], pose_rows([(30, 20)], [0]))
        assert (int(want[0, 0]["k"]), int(want[0, 0]["status"]), int(want[0, 0]["jx"]), int(want[0, 0]["jy"])) == (j, kr.S_HIT, j, j)
        assert (int(want[0, 1]["k"]), int(want[0, 1]["status"])) == (20, kr.S_OFF_MAP)


@pytest.mark.gpu
def test_an_obstacle_at_the_end_of_a_ray_and_one_beyond(ctx):
    axes = [e << 20 for e in (0, 1024, 2048, 3072)]
    for R, beyond, status in ((25, 0, kr.S_HIT), (25, 1, kr.S_MAX), (1, 0, kr.S_HIT), (1, 1, kr.S_MAX)):
        img = np.full((NY, NX), -1, np.int8)
        for sx, sy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            img[40 + sy * (R + beyond), 48 + sx * (R + beyond)] = 100
        load(ctx, img)
        want = check(ctx, q_of(1, 4, R), axes, pose_rows([(48, 40)], [0]))
        assert [(int(r["k"]), int(r["status"])) for r in want[0]] == [(R, status)] * 4
    d = int(capi.cast_directions(30)[512, 0])          # the diagonal of range_cells 30 ends d cells out on both axes
    for beyond, status in ((0, kr.S_HIT), (1, kr.S_MAX)):
        img = np.zeros((NY, NX), np.int8)
        img[40 + d + beyond, 48 + d + beyond] = 100
        load(ctx, img)
        want = check(ctx, q_of(1, 1, 30), [512 << 20], pose_rows([(48, 40)], [0]))
        assert (int(want[0, 0]["k"]), int(want[0, 0]["status"])) == (d, status)


@pytest.mark.gpu
def test_neighbouring_and_grazing_cells(ctx):
    img = np.zeros((NY, NX), np.int8)
    img[41, 55] = img[39, 60] = 100                    # beside the +x ray from (48, 40), not on it
    img[45, 47] = img[46, 48] = 100                    # (47, 45) and (48, 46) touch at a corner only: the -x+y diagonal from (50, 43) passes between
    load(ctx, img)
    want = check(ctx, q_of(2, 1, 20), [0], pose_rows([(48, 40), (50, 43)], [0, 1536 << 20]))
    assert [(int(r["k"]), int(r["status"])) for r in want[:, 0]] == [(20, kr.S_MAX), (14, kr.S_MAX)]
    cells = [(50 - k, 43 + k) for k in range(15)]
    assert (47, 46) in cells and (48, 45) in cells and (48, 46) not in cells and (47, 45) not in cells
    want = check(ctx, q_of(2, 64, 20), None, pose_rows([(48, 40), (50, 43)], [123456789, 987654321]))
    assert (want["status"] == kr.S_HIT).any()


@pytest.mark.gpu
def test_origins(ctx):
    img = random_image(5, 77)
    img[0, 0] = img[NY - 1, NX - 1] = 0
    img[0, NX - 1] = img[NY - 1, 0] = -1
    img[50, 50] = 100
    load(ctx, img)
    cells = [(50, 50), (0, 0), (NX - 1, 0), (0, NY - 1), (NX - 1, NY - 1), (-1, 40), (NX, 40), (40, -1), (40, NY), (-1, -1), (NX, NY)]
    poses = pose_rows(cells, [0] * len(cells))
    special = kr.poses_of([(np.nan, 0.0, 1), (0.0, np.nan, 2), (np.inf, 0.0, 3), (0.0, -np.inf, 4), (1e30, 0.0, 5), (0.0, -1e30, 6), (1.1e8, 0.0, 7)])
    poses = np.concatenate([poses, special])
    want = check(ctx, q_of(len(poses), 16, 30), None, poses)
    assert (want[0]["status"] == kr.S_HIT).all() and (want[0]["k"] == 0).all() and (want[0]["jx"] == 0).all()
    assert (want[1:5]["status"] != kr.S_NO_ORIGIN).all() and (want[1:5]["status"] == kr.S_OFF_MAP).any()
    assert (want[5:]["status"] == kr.S_NO_ORIGIN).all() and want[5:].tobytes() == np.tile(np.array([(0, 3, 0, 0, 0)], kr.RAY), (len(poses) - 5, 16)).tobytes()


@pytest.mark.gpu
def test_window_edges(ctx):
    load(ctx, np.full((NY, NX), -1, np.int8))
    eight = [e << 20 for e in range(0, 4096, 512)]
    want = check(ctx, q_of(1, 8, 1024), eight, pose_rows([(48, 40)], [0]))
    assert (want["status"] == kr.S_OFF_MAP).all()
    assert [int(k) for k in want[0]["k"]] == [47, 39, 39, 39, 48, 40, 40, 40]
    cells = [(0, 0), (NX - 1, 0), (0, NY - 1), (NX - 1, NY - 1), (0, 40), (NX - 1, 40), (48, 0), (48, NY - 1), (1, 1), (NX - 2, NY - 2)]
    check(ctx, q_of(len(cells), 65, 200), None, pose_rows(cells, list(range(0, 10 << 28, 1 << 28))))
    check(ctx, q_of(len(cells), 63, 3), None, pose_rows(cells, [0] * len(cells)))


@pytest.mark.gpu
def test_a_long_window():
    """2048 x 8 cells with range_cells 1024: along the row over an empty map (dist2 is CM_MAP_DIST_NONE everywhere) and with
    one obstacle at step 1024."""
    nx, ny = 2048, 8
    q = mpr.params(CELL, nx, ny)
    anchor = tmm.anchor_of(nx, ny)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        tm.configure(cm, q)
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        img = np.full((ny, nx), -1, np.int8)
        load(cm, img, anchor, q)
        assert (cm.map_cost()[1] == capi.MAP_DIST_NONE).all()
        poses = pose_rows([(3, 2), (1023, 5), (2044, 7), (1500, 0)], [0, 0, 2048 << 20, 2048 << 20], anchor)
        want = check(cm, q_of(4, 1, 1024), [0], poses)
        assert [(int(r["k"]), int(r["status"])) for r in want[:, 0]] == [(1024, 0), (1024, 0), (1024, 0), (1024, 0)]
        want = check(cm, q_of(4, 5, 1024), [0, 1 << 20, 0xFFF00000, 1 << 30, 3 << 30], poses)
        assert (want["status"] == kr.S_OFF_MAP).any()
        img[2, 3 + 1024] = img[7, 2044 - 1024] = 100
        img[5, 1023 + 1025 - 1] = 100
        load(cm, img, anchor, q)
        want = check(cm, q_of(4, 1, 1024), [0], poses)
        assert [(int(r["k"]), int(r["status"])) for r in want[:, 0]] == [(1024, 1), (1024, 1), (1024, 1), (1024, 0)]
        assert [int(v) for v in want[:, 0]["jx"]] == [1024, 1024, -1024, -1024]


@pytest.mark.gpu
@pytest.mark.parametrize("n_poses", [1, 63, 64, 65, 130])
def test_pose_counts(ctx, n_poses):
    load(ctx, random_image(5, 21))
    check(ctx, q_of(130, 33, 50), None, random_poses(n_poses, n_poses))


@pytest.mark.gpu
@pytest.mark.parametrize("n_bearings", [1, 63, 65, 4096])
def test_bearing_counts_and_lists(ctx, n_bearings):
    load(ctx, random_image(5, 22))
    poses = random_poses(5, n_bearings, margin=0)
    even = check(ctx, q_of(5, n_bearings, 45), None, poses)
    listed = check(ctx, q_of(5, n_bearings, 45), kr.even_bearings(n_bearings), poses)      # the NULL list against its formula
    assert even.tobytes() == listed.tobytes()
    rng = np.random.default_rng(n_bearings)
    b = rng.integers(0, 1 << 32, n_bearings, dtype=np.uint64)
    b[0] = 0xFFFFFFFF
    b[n_bearings // 2] = b[0]
    b[-1] = b[n_bearings // 3]                         # repeats
    check(ctx, q_of(5, n_bearings, 45), b, poses)


@pytest.mark.gpu
def test_the_ranges_and_yaw_poses(ctx):
    load(ctx, room_image())
    ctx.map_cast_configure(4, 8, 30)
    rows = [world(60, 33) + (0.3,), world(20, 50) + (-2.0,), world(60, 33) + (7.0,)]
    info = ctx.map_cast(rows)
    assert (info.n_poses, info.n_bearings) == (3, 8)
    poses = kr.poses_of([(x, y, kr.heading(yaw)) for x, y, yaw in rows])
    assert [capi.cast_heading(v) for v in (0.3, -2.0, 7.0)] == [int(h) for h in poses["h"]]
    image, minfo = ctx.map_occupancy()
    want, _ = kr.cast(image, CELL, tuple(minfo.anchor), q_of(4, 8, 30), None, poses, TAB())
    ranges, rays, _ = ctx.map_cast_ranges()
    assert rays.tobytes() == want.tobytes() and ranges.dtype == np.float64 and ranges.tobytes() == kr.ranges(want, CELL).tobytes()


@pytest.mark.gpu
def test_casting_from_the_particles():
    from tests import test_map_mcl as tml
    with capi.CloudMerger(max_points_total=16384, max_sensors=2, flags=capi.FLAG_PROFILE) as cm:
        tml.build_room(cm)
        tml.frame(cm, tml.body_points(tml.scan_of(tml.TRUTH0)))
        cm.map_mcl_configure(300, 256, 64, 0.1, 0.5, 8.0, 0.5, True, 5)
        q = q_of(300, 16, 50)
        image, minfo = cm.map_occupancy()

        def particles_cast(read_weights):
            parts = cm.map_mcl_particles()
            keep_w = cm.map_mcl_weights()[0].tobytes() if read_weights else None
            poses = np.zeros(len(parts), kr.POSE)
            poses["x"], poses["y"], poses["h"] = parts["x"], parts["y"], parts["h"]
            want, winfo = kr.cast(image, CELL, tuple(minfo.anchor), q, None, poses, TAB())
            for plain in (False, True):
                cm.map_cast_configure(q["max_poses"], q["n_bearings"], q["range_cells"], plain)
                info = cm.map_cast_particles()
                got, _ = cm.map_cast_rays()
                assert got.tobytes() == want.tobytes() and [getattr(info, f) for f in INFO] == [winfo[f] for f in INFO]
                cm.map_cast(poses)
                assert cm.map_cast_rays()[0].tobytes() == want.tobytes()
                assert cm.map_mcl_particles().tobytes() == parts.tobytes()
                if read_weights:
                    assert cm.map_mcl_weights()[0].tobytes() == keep_w
                else:
                    tm.refused(cm, cm.map_mcl_weights, text=b"stale")
            return want

        cm.map_cast_configure(q["max_poses"], q["n_bearings"], q["range_cells"])
        tm.refused(cm, cm.map_cast_particles, text=b"not initialised")
        cm.map_mcl_init_pose(tml.TRUTH0[0], tml.TRUTH0[1], tml.TRUTH0[2], 0.3, 0.3, 0.1)
        first = particles_cast(False)
        assert (first["status"] == kr.S_HIT).any()
        cm.map_mcl_predict(0.1, 0.0, 0.05, 0.03, 0.03, 0.02)
        assert cm.map_mcl_update().resampled == 1
        second = particles_cast(True)
        assert second.tobytes() != first.tobytes()
        cm.map_cast_configure(299, 16, 50)
        tm.refused(cm, cm.map_cast_particles, text=b"max_poses")
        cm.map_mcl_configure(None)
        tm.refused(cm, cm.map_cast_particles, text=b"cm_map_mcl_configure")


@pytest.mark.gpu
def test_refusals_and_staleness():
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        L = cm._lib
        poses = pose_rows([(10, 10), (20, 20)], [0, 1])
        tm.refused(cm, cm.map_cast_configure, 4, 4, 4, text=b"cm_map_configure")
        tm.configure(cm, MQ)
        tm.refused(cm, cm.map_cast_configure, 4, 4, 4, text=b"cm_map_cost_configure")
        tm.refused(cm, cm.map_cast, poses, text=b"cm_map_cost_configure")
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        tm.refused(cm, cm.map_cast, poses, text=b"cm_map_cast_configure")
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_cast_configure")
        for kw in REFUSED_PARAMS:
            q = q_of(**kw)
            p = capi.CastParams(q["max_poses"], q["n_bearings"], q["range_cells"], q["flags"])
            assert L.cm_map_cast_configure(cm._ctx, C.byref(p), None) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
            tm.refused(cm, cm.map_cast, poses, text=b"cm_map_cast_configure")      # a refused configure call leaves no layer
        for kw in ACCEPTED_PARAMS:
            q = q_of(**kw)
            if q["max_poses"] * q["n_bearings"] > 1 << 20:
                continue                               # (the largest tables are not allocated here)
            p = capi.CastParams(q["max_poses"], q["n_bearings"], q["range_cells"], q["flags"])
            assert L.cm_map_cast_configure(cm._ctx, C.byref(p), None) == capi.OK, kw
        cm.map_cast_configure(4, 4, 10)
        tm.refused(cm, cm.map_cast, poses, text=b"stale")                          # no dist2 yet
        tm.refused(cm, cm.map_cast_rays, text=b"since cm_map_cast_configure")      # stale since the configure call
        cm.map_cost_update()                                                       # (the map holds no frame, which is allowed)
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_cost_update")
        tm.refused(cm, cm.map_cast_device, text=b"stale")
        assert cm.map()[1].n_frames == 0 and tuple(cm.map()[1].anchor) == (0, 0)
        poses = pose_rows([(10, 10), (20, 20)], [0, 1], (0, 0))                    # (the anchor of a map without a frame)
        info = cm.map_cast(poses)
        assert info.n_hit == 0 and info.n_no_origin == 0 and info.n_max + info.n_off_map == 8
        assert cm.map_cast_rays()[0].shape == (2, 4)
        keep = capi.CastInfo(9, 9, 9, 9, 9, 9)
        assert L.cm_map_cast_evaluate(cm._ctx, poses.ctypes.data, 0, C.byref(keep)) == capi.BAD_ARG and b"max_poses" in L.cm_last_error(cm._ctx)
        assert L.cm_map_cast_evaluate(cm._ctx, poses.ctypes.data, 5, C.byref(keep)) == capi.BAD_ARG
        assert L.cm_map_cast_evaluate(cm._ctx, None, 2, C.byref(keep)) == capi.BAD_ARG and b"poses" in L.cm_last_error(cm._ctx)
        assert bytes(keep) == bytes(capi.CastInfo(9, 9, 9, 9, 9, 9))
        assert cm.map_cast_rays()[0].shape == (2, 4)                               # a refused evaluate leaves the rays readable
        # a short destination copies nothing and still writes the info
        buf = np.full(8, 7, capi.CAST_RAY_DTYPE)
        assert L.cm_map_cast_copy(cm._ctx, buf.ctypes.data, 7, C.byref(keep)) == capi.CAPACITY and (buf == np.full(8, 7, capi.CAST_RAY_DTYPE)).all()
        assert bytes(keep) == bytes(info)
        assert L.cm_map_cast_copy(cm._ctx, None, 8, None) == capi.BAD_ARG
        # stale from every load and cost update until the next evaluate
        img = random_image(5, 3)
        cm.map_load(table_of(img), ANCHOR)
        poses = pose_rows([(10, 10), (20, 20)], [0, 1])
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_load")
        tm.refused(cm, cm.map_cast, poses, text=b"stale")
        cm.map_cost_update()
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_cost_update")
        tm.refused(cm, cm.map_cast_device, text=b"cm_map_cost_update")
        cm.map_cast(poses)
        cm.map_cast_rays()
        # ... and from an integration
        tg.run_frame(cm, tmm.clouds_of(tmm.parts_of([[(5, 5)]], NX, NY))[0][:1], tg_params())
        cm.map_cast_rays()                                                         # a merge alone changes nothing the layer reads
        cm.map_integrate(None)
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_integrate")
        tm.refused(cm, cm.map_cast, poses, text=b"stale")
        cm.map_cost_update()
        cm.map_cast(poses)
        # the configure calls of the cost layer and of the map free the layer
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_cast_configure")
        cm.map_cast_configure(4, 4, 10)
        tm.configure(cm, MQ)
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        tm.refused(cm, cm.map_cast, poses, text=b"cm_map_cast_configure")
        cm.map_cast_configure(4, 4, 10)
        cm.map_cast_configure(None)
        tm.refused(cm, cm.map_cast_rays, text=b"cm_map_cast_configure")


def tg_params():
    from tests import test_map_cost as tc
    return tc.PARAMS


@pytest.mark.gpu
def test_a_frame_in_flight_is_refused():
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, MQ)
        cm.map_cost_configure(0.0, 0.3, 3.0, False)
        cm.map_cost_update()
        cm.map_cast_configure(4, 4, 10)
        poses = pose_rows([(10, 10)], [0])
        cm.map_cast(poses)
        sensors = tmm.clouds_of(tmm.parts_of([[(5, 5)]], NX, NY))[0][:1]
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(tg_params()))
        for call in (lambda: cm.map_cast(poses), lambda: cm.map_cast_configure(4, 4, 10), lambda: cm.map_cast_configure(None), cm.map_cast_rays,
                     cm.map_cast_device, cm.map_cast_particles):
            tm.refused(cm, call, text=b"flight")
        assert cm.wait().status == capi.OK
        assert cm.map_cast_rays()[0].shape == (1, 4)   # a merge alone makes nothing stale


@pytest.mark.gpu
def test_a_cast_changes_no_other_layer():
    from tests import test_map_mcl as tml
    with capi.CloudMerger(max_points_total=16384, max_sensors=2, flags=capi.FLAG_PROFILE) as cm:
        tml.build_room(cm)
        cm.map_plan_configure(50, 205, True)
        cm.map_traj_configure(3, 3, 4, [(0.1, 0.0)], 1, 1, True)
        cm.map_frontier_configure()
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
        tml.frame(cm, tml.body_points(tml.scan_of(tml.TRUTH0)))
        cm.map_plan_update(2.05, 1.05)
        cm.map_traj_evaluate(0.05, 0.05, 0.0, (0.0, 1.0), (-1.0, 1.0), 0.1)
        cm.map_frontier_update()
        cm.map_match(tm.pose_t(0.1, 0.0))

        def state():
            table, info = cm.map()
            cost, dist2, _ = cm.map_cost()
            return (table.tobytes(), cm.map_occupancy()[0].tobytes(), tm.info_tuple(info), cost.tobytes(), dist2.tobytes(), cm.map_cost_table().tobytes(),
                    cm.map_plan()[0].tobytes(), cm.map_traj()[0].tobytes(), bytes(cm.map_traj()[1]), cm.map_frontier_labels()[0].tobytes(),
                    cm.map_match_scores()[0].tobytes(), bytes(cm.map_match_scores()[1]), cm.merged(16384).tobytes())

        before = state()
        check(cm, q_of(40, 33, 70), None, random_poses(40, 1))
        assert state() == before                       # nothing went stale either: every read above still answers
        cm.map_cast_configure(None)
        assert state() == before
        tml.frame(cm, tml.body_points(tml.scan_of(tml.TRUTH0)))
        assert not any("cast" in n for n, _ in cm.stage_times())
