"""Oriented bounding boxes of the clusters: cm_box_directions, cm_result_cluster_boxes / _device (include/cloudmerge.h,
cm_kernels_box.hip).

The bar on the GPU: every byte of the box table equal to the restatement (tests/box_ref.py: boxes_vectorised) fed with the
frame's own result, the call's own cluster tables and the direction table cm_box_directions returns. There is no tolerance:
min / max are order-free and the one floating sum has a defined order. No test passes vacuously: before the device's table is
looked at, the restatement's own output must hold at least two valid boxes, two distinct angles and one that is not 0.

Bounds that are this file's own: the direction table against numpy's cos / sin is 1 ulp (two correctly-or-nearly-so rounded
libms, each then rounded to fp32, can differ by one float); the heading recovered by the restatement is 3 degrees: at 1 degree
steps and 2 cm noise on sides of 4.5 and 1.8 m the fit lands within about 1.6 degrees, and the bound leaves the voxel grid room."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import box_ref as br
from tests import cluster_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
F32 = np.float32
NONE = cr.NONE
AREA, CLOSENESS = capi.BOX_AREA, capi.BOX_CLOSENESS
SPLIT = 1024                                   # CM_BOX_SPLIT (cm_device.h): above it a cluster goes chunk-wise


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_box_structs_match_header(tmp_path):
    fields_p = ["cluster", "n_angles", "criterion", "d_min", "_pad"]
    fields_b = ["center", "size", "yaw", "angle", "score", "flags", "_pad"]
    items = (["sizeof(cm_box_params)"] + [f"offsetof(cm_box_params,{f})" for f in fields_p] + ["sizeof(cm_cluster_box)"] +
             [f"offsetof(cm_cluster_box,{f})" for f in fields_b])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, B = capi.BoxParams, capi.ClusterBox
    want = ([C.sizeof(P)] + [getattr(P, f).offset for f in fields_p] + [C.sizeof(B)] + [getattr(B, f).offset for f in fields_b])
    assert got == want and got[0] == 32 and got[6] == 48
    d = capi.BOX_DTYPE
    assert [d.fields[f][1] for f in fields_b] == want[7:] and d == br.BOX_DTYPE


def test_constants_mirror_the_header():
    text = open(HEADER).read()

    def define(name):
        m = re.search(r"#define\s+" + name + r"\s+(\S+)", text)
        assert m, name
        return float(m.group(1).rstrip("uf"))
    assert define("CM_BOX_MAX_ANGLES") == capi.BOX_MAX_ANGLES == br.MAX_ANGLES == 180
    assert define("CM_BOX_CHUNK") == capi.BOX_CHUNK == br.CHUNK == 256
    assert define("CM_BOX_MAX_EXTENT") == capi.BOX_MAX_EXTENT == float(br.MAX_EXTENT) == 1.0e6
    assert define("CM_BOX_AREA") == capi.BOX_AREA == br.AREA == 0
    assert define("CM_BOX_CLOSENESS") == capi.BOX_CLOSENESS == br.CLOSENESS == 1
    assert define("CM_BOX_VALID") == capi.BOX_VALID == br.VALID == 1
    for name in ("cm_box_directions", "cm_result_cluster_boxes", "cm_result_cluster_boxes_device"):
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.box_params(0.5)
    out = np.zeros(4, capi.BOX_DTYPE)
    n = C.c_uint64(7)
    assert L.cm_result_cluster_boxes(None, C.byref(p), out.ctypes.data, 4, C.byref(n)) == capi.BAD_ARG
    assert L.cm_result_cluster_boxes(None, None, None, 0, None) == capi.BAD_ARG
    ptr = C.c_void_p()
    assert L.cm_result_cluster_boxes_device(None, C.byref(p), C.byref(ptr), C.byref(n)) == capi.BAD_ARG


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_directions():
    L = capi.load()
    for n in (1, 2, 63, 64, 65, 90, 179, 180):
        d = capi.box_directions(n)
        assert d.shape == (n, 2) and d.dtype == F32
        assert d[0].tobytes() == F32([1.0, 0.0]).tobytes()            # exactly (1, +0)
        w = br.directions_numpy(n)
        assert ulps(np.ascontiguousarray(d), w).max() <= 1, n
        assert (d[:, 0] > 0).all() and (d[1:, 1] > 0).all() and (np.diff(d[:, 1]) > 0).all()
    buf = np.full((8, 2), 7.0, F32)
    assert L.cm_box_directions(8, buf.ctypes.data, 7) == capi.CAPACITY and (buf == 7.0).all()
    assert L.cm_box_directions(8, buf.ctypes.data, 8) == capi.OK and buf[0, 0] == 1.0
    assert L.cm_box_directions(0, buf.ctypes.data, 8) == capi.BAD_ARG
    assert L.cm_box_directions(181, buf.ctypes.data, 1000) == capi.BAD_ARG
    assert L.cm_box_directions(8, None, 8) == capi.BAD_ARG
    with pytest.raises(capi.CloudMergeError):
        capi.box_directions(0)


# ---- CPU: the two restatements ------------------------------------------------------------------------------------------
def both(xyz, groups, dirs, criterion=CLOSENESS, d_min=0.01):
    table, indices = br.tables_of(xyz, groups)
    a = br.boxes_vectorised(xyz, table, indices, dirs, criterion, d_min)
    b = br.boxes_loop(xyz, table, indices, dirs, criterion, d_min)
    assert a.tobytes() == b.tobytes()
    return a


def rot(xy, th):
    c, s = np.cos(th), np.sin(th)
    return np.stack([xy[:, 0] * c - xy[:, 1] * s, xy[:, 0] * s + xy[:, 1] * c], axis=1)


def test_the_two_restatements_agree():
    rng = np.random.default_rng(5)
    dirs = capi.box_directions(12)
    parts, groups, at = [], [], 0
    sizes = [1, 2, 3, 7, 40, 255, 256, 257, 513]
    for k, m in enumerate(sizes):                                        # random blobs at random headings, near and far
        c = rng.uniform(-50, 50, 2) * (1.0 if k % 2 else 200.0)
        p = rot(rng.uniform(0, 1, (m, 2)) * [4.5, 1.8], rng.uniform(0, np.pi)) + c
        parts.append(np.concatenate([p, rng.uniform(-1, 1, (m, 1))], axis=1))
        groups.append(range(at, at + m)); at += m
    # adversarial: duplicates, members on the box's own corners, a line along a tried heading, tiny extents
    dup = np.tile([[3.0, 4.0, 5.0]], (5, 1))
    corners = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1]], float) + [10, 10, 0]
    t = np.arange(9)[:, None] * 0.25
    lined = np.concatenate([t * float(dirs[3, 0]), t * float(dirs[3, 1]), 0 * t], axis=1) - [7, 7, 0]
    tiny = np.array([[1e-30, 0, 0], [0, 1e-30, 0], [1e-38, 1e-38, 0]], float)
    for p in (dup, corners, lined, tiny):
        parts.append(p); groups.append(range(at, at + len(p))); at += len(p)
    xyz = np.concatenate(parts).astype(F32)
    order = rng.permutation(len(xyz))                                    # members are lists of indices, not ranges
    inv = np.argsort(order)
    xyz, groups = xyz[order], [[int(inv[j]) for j in g] for g in groups]
    for crit, d_min in ((AREA, 0.0), (CLOSENESS, 0.01), (CLOSENESS, 1e-30), (CLOSENESS, 10.0)):
        got = both(xyz, groups, dirs, crit, d_min)
        assert (got["flags"] == 1).all()
        if d_min in (0.0, 0.01):
            assert len(set(got["angle"].tolist())) >= 5
        elif d_min == 10.0:                                              # above every distance: one long tie, angle 0
            assert not got["angle"].any()
        # (at 1e-30 the members on the rectangle itself, 1e30 each, leave the others no say: few headings differ)
    assert both(xyz, groups, dirs, CLOSENESS, 0.01).tobytes() != both(xyz, groups, dirs, AREA).tobytes()


# ---- CPU: known answers --------------------------------------------------------------------------------------------------
def lattice(nx, ny, step=0.5, origin=(2.0, 3.0, 1.0), nz=1):
    k = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return (k * step + np.array(origin)).astype(F32)


@pytest.mark.parametrize("crit", [AREA, CLOSENESS])
def test_axis_aligned_lattice_at_one_angle_is_the_cluster_tables_box(crit):
    xyz = lattice(9, 4, nz=3)
    table, _ = br.tables_of(xyz, [range(len(xyz))])
    b = both(xyz, [range(len(xyz))], capi.box_directions(1), crit)[0]
    mn, mx = table[0]["min"], table[0]["max"]
    assert b["flags"] == 1 and b["angle"] == 0 and b["yaw"] == 0
    assert np.array_equal(b["size"], mx - mn) and np.array_equal(b["size"], F32([4.0, 1.5, 1.0]))
    assert np.array_equal(b["center"], F32([4.0, 3.75, 1.5]))           # halves of multiples of 0.5: exact
    assert b["score"] == (-6.0 if crit == AREA else b["score"]) and np.isfinite(b["score"])


def test_single_member_and_all_duplicates():
    xyz = F32([[5, 6, 7], [1, 2, 3], [1, 2, 3], [1, 2, 3]])
    for crit in (AREA, CLOSENESS):
        got = both(xyz, [[0], [1, 2, 3]], capi.box_directions(90), crit, 0.01)
        for b, c, m in zip(got, ([5, 6, 7], [1, 2, 3]), (1, 3)):
            assert b["flags"] == 1 and b["angle"] == 0 and b["yaw"] == 0 and not b["size"].any()
            assert np.array_equal(b["center"], F32(c))
            assert b["score"] == (0.0 if crit == AREA else m * (1.0 / float(F32(0.01))))


def test_square_lattice_under_area_resolves_its_tie_to_angle_0():
    xyz = lattice(6, 6)
    b = both(xyz, [range(36)], capi.box_directions(90), AREA)[0]
    assert b["angle"] == 0 and np.array_equal(b["size"], F32([2.5, 2.5, 0.0])) and b["score"] == -6.25
    # two members on the diagonal: area 0 at 45 degrees, which 90 angles hold exactly once
    b = both(F32([[0, 0, 0], [2, 2, 0]]), [[0, 1]], capi.box_directions(90), AREA)[0]
    assert b["angle"] == 45 and b["size"][1] <= 1e-6 and abs(b["size"][0] - 2 * np.sqrt(2)) < 1e-6


def test_extent_of_1e6_or_more_is_not_valid():
    xyz = F32([[0, 0, 0], [1.0e6, 1, 0], [0, 50, 0], [999_999.9375, 51, 0], [0, 100, 0], [1, 100 + 1.0e6, 2]])
    got = both(xyz, [[0, 1], [2, 3], [4, 5]], capi.box_directions(16))
    assert got["flags"].tolist() == [0, 1, 0] and got["angle"].tolist()[0] == 0 and got["angle"].tolist()[2] == 0
    for b in (got[0], got[2]):
        assert np.isnan(b["center"]).all() and np.isnan(b["size"]).all() and np.isnan(b["yaw"]) and np.isnan(b["score"])
    assert np.isfinite(got[1]["center"]).all() and np.isfinite(got[1]["score"])
    # not finite: a z extent that overflows
    big = F32([[0, 0, -3e38], [1, 1, 3e38]])
    assert both(big, [[0, 1]], capi.box_directions(4))["flags"][0] == 0


# ---- CPU: the restatement recovers headings ------------------------------------------------------------------------------
L_LEN, L_WID = 4.5, 1.8


def l_shape(rng, heading, n=160, noise=0.02):
    """The two visible sides of a 4.5 x 1.8 m box seen from outside its corner, 2 cm range noise."""
    n1 = int(round(n * L_LEN / (L_LEN + L_WID)))
    a = np.stack([rng.uniform(0, L_LEN, n1), np.zeros(n1)], axis=1)
    b = np.stack([np.zeros(n - n1), rng.uniform(0, L_WID, n - n1)], axis=1)
    xy = np.concatenate([a, b]) + rng.normal(0, noise, (n, 2))
    return rot(xy, heading)


def filled(rng, heading, n=400):
    return rot(rng.uniform(0, 1, (n, 2)) * [L_LEN, L_WID], heading)


def shapes_cloud(make, seed, n_shapes=20, centre=(60.0, 60.0)):
    """n_shapes shapes at seeded headings in (0, 90) degrees on a lattice of 12 m: the cloud, its groups, the headings."""
    rng = np.random.default_rng(seed)
    heads = np.radians(rng.uniform(2.0, 88.0, n_shapes))
    parts, groups, at = [], [], 0
    for k, h in enumerate(heads):
        xy = make(rng, h) + [centre[0] + 12.0 * (k % 5), centre[1] + 12.0 * (k // 5)]
        parts.append(np.concatenate([xy, rng.uniform(0, 1.5, (len(xy), 1))], axis=1))
        groups.append(range(at, at + len(xy))); at += len(xy)
    return np.concatenate(parts).astype(F32), groups, heads


def recovered(make, seed, crit):
    xyz, groups, heads = shapes_cloud(make, seed)
    table, indices = br.tables_of(xyz, groups)
    got = br.boxes_vectorised(xyz, table, indices, capi.box_directions(90), crit, 0.01)
    err = [br.heading_error_deg(b["yaw"], h) for b, h in zip(got, heads)]
    print(f"criterion {crit}: heading error max {max(err):.2f} deg, mean {np.mean(err):.2f} deg over {len(err)} shapes")
    assert (got["flags"] == 1).all()
    return max(err), got


def test_l_shapes_are_recovered_within_3_degrees_under_closeness():
    worst, got = recovered(l_shape, 11, CLOSENESS)
    assert worst <= 3.0
    assert (np.abs(np.sort(got["size"][:, :2], axis=1) - [L_WID, L_LEN]) < 0.25).all()


@pytest.mark.parametrize("crit", [AREA, CLOSENESS])
def test_filled_rectangles_are_recovered_within_3_degrees(crit):
    worst, _ = recovered(filled, 12, crit)
    assert worst <= 3.0


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def hip_rt():
    try:
        return C.CDLL("libamdhip64.so.7")
    except OSError:
        return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def expected(cm, res, tol, lo=1, hi=NONE, n_angles=90, crit=CLOSENESS, d_min=0.01, vacuous_ok=False):
    """The restatement on the frame's own result and the call's own cluster tables, and the conditions that keep the
    comparison from being vacuous."""
    rec = cm.result(res.n_out)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    _, table, indices = cm.clusters(tol, lo, hi)
    want = br.boxes_vectorised(xyz, table, indices, capi.box_directions(n_angles), crit, d_min)
    valid = want[want["flags"] == 1]
    print(f"n_out {res.n_out} tol {tol} [{lo}, {hi}] angles {n_angles} criterion {crit}: clusters {len(table)} largest "
          f"{int(table['n_voxels'].max()) if len(table) else 0} valid {len(valid)} distinct angles {len(set(valid['angle'].tolist()))}")
    if not vacuous_ok:
        assert len(valid) >= 2
        if n_angles > 1:
            assert len(set(valid["angle"].tolist())) >= 2 and valid["angle"].any()
    return want, table


def check(cm, res, tol, lo=1, hi=NONE, n_angles=90, crit=CLOSENESS, d_min=0.01, vacuous_ok=False):
    assert res.status == capi.OK
    want, table = expected(cm, res, tol, lo, hi, n_angles, crit, d_min, vacuous_ok)
    got = cm.cluster_boxes(tol, lo, hi, n_angles, crit, d_min)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
        k = bad[0]
        raise AssertionError(f"{len(bad)} of {len(got)} boxes differ, first {bad[:8]} (members {table['n_voxels'][bad[:8]]}): "
                             f"got {got[k]} want {want[k]}")
    # the context holds the call's cluster tables
    _, cp, _, nc, _ = cm.clusters_device(tol, lo, hi)
    assert nc == len(want)
    # the device entry point: the same bytes
    ptr, n = cm.cluster_boxes_device(tol, lo, hi, n_angles, crit, d_min)
    assert n == len(want) and bool(ptr) == (len(want) > 0)
    if len(want):
        d = np.zeros_like(want)
        assert hip_rt().hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(want.nbytes), 2) == 0
        assert d.tobytes() == want.tobytes()
    return want, table


def snap(xyz, leaf):
    """The points moved to the centres of their voxels, one per voxel: every input point its own voxel whatever the
    rounding of the grid arithmetic."""
    cells = np.unique(np.floor(np.asarray(xyz, np.float64) / leaf).astype(np.int64), axis=0)
    return ((cells + 0.5) * leaf).astype(F32)


def submit_as_voxels(cm, xyz, leaf, min_pts=1):
    """Every input point its own voxel and every centroid an input bit for bit: asserted before anything else."""
    xyz = np.ascontiguousarray(xyz, F32)
    cm.submit(0, xyzi_cloud(xyz, np.ones(len(xyz), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=min_pts))
    assert res.status == capi.OK and res.n_out == len(xyz)
    rec = cm.result(res.n_out)
    got = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).view(np.uint32)
    key = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    assert np.array_equal(key(got), key(xyz.view(np.uint32)))
    return res


def blob(m, heading, rng, step=0.5):
    """m points of a lattice of `step`, rows of a random width, turned by `heading`: one component at a tolerance above
    the step, whatever the snap to voxel centres moves."""
    w = max(1, int(np.sqrt(m) * rng.uniform(0.6, 1.6)))
    k = np.arange(m)
    return rot(np.stack([(k % w) * step, (k // w) * step], axis=1), heading)


def sized_clusters(seed=4):
    """Clusters of 1, 2, 255, 256, 257, 512, 513, SPLIT and SPLIT + 1 members and 300 of 3 .. 40, 70 m and 16 m apart."""
    rng = np.random.default_rng(seed)
    big = [1, 2, 255, 256, 257, 512, 513, SPLIT, SPLIT + 1]
    small = rng.integers(3, 41, 300).tolist()
    parts = []
    for k, m in enumerate(big):
        parts.append(blob(m, rng.uniform(0, np.pi / 2), rng) + [70.0 * k, -100.0])
    for k, m in enumerate(small):                      # (the first few at 88.7 degrees: the last of 65 headings is 88.6)
        parts.append(blob(m, np.radians(88.7) if k < 4 else rng.uniform(0, np.pi / 2), rng) + [16.0 * (k % 25), 16.0 * (k // 25)])
    line = np.arange(41)[:, None] * 0.5 * np.array([[np.cos(np.radians(88.7)), np.sin(np.radians(88.7))]])
    parts.append(line + [-40.0, 0.0])                  # 20 m at that heading: under AREA the 65th heading wins it
    small.append(41)
    # heights within 0.2 m inside a cluster: with the snap's 0.07 m per point, lattice neighbours stay within 0.68 m
    xyz = np.concatenate([np.concatenate([xy, rng.uniform(0, 0.2, (len(xy), 1)) + 0.1 * (k % 9)], axis=1) for k, xy in enumerate(parts)])
    return snap(xyz, 0.1), sorted(big + small)


@pytest.fixture(scope="module")
def sized_frame():
    xyz, sizes = sized_clusters()
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        res = submit_as_voxels(cm, xyz, 0.1)
        yield cm, res, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("crit", [AREA, CLOSENESS], ids=["area", "closeness"])
def test_chunk_and_route_edges(sized_frame, crit):
    cm, res, sizes = sized_frame
    want, table = check(cm, res, 0.75, crit=crit)
    assert sorted(table["n_voxels"].tolist()) == sizes               # the clusters are the ones that were built
    assert (want["flags"] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_angles", [1, 63, 64, 65, 90, 180])
def test_lane_edges(sized_frame, n_angles):
    cm, res, _ = sized_frame
    check(cm, res, 0.75, n_angles=n_angles)
    want, _ = check(cm, res, 0.75, n_angles=n_angles, crit=AREA)
    # the 20 m line at 88.7 degrees is won by the heading next to it: the last one of 63, 64, 65 and 90
    assert want["angle"].max() >= min(int(round(88.7 / (90.0 / n_angles))), n_angles - 1) >= (n_angles > 1) * (n_angles - 3)


@pytest.mark.gpu
def test_d_min_and_the_size_filter(sized_frame):
    cm, res, _ = sized_frame
    a, _ = check(cm, res, 0.75, d_min=0.01)
    b, _ = check(cm, res, 0.75, d_min=0.3)
    assert a.tobytes() != b.tobytes()
    c, table = check(cm, res, 0.75, 3, SPLIT)                          # a filter that drops components at both ends
    assert len(c) == len(a) - 3 and table["n_voxels"].max() == SPLIT


def shapes_for_gpu(offset):
    a, _, _ = shapes_cloud(l_shape, 21, 10, centre=(60.0 + offset, 60.0 + offset))
    b, _, _ = shapes_cloud(filled, 22, 10, centre=(60.0 + offset, 100.0 + offset))
    return np.concatenate([a, b])


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 1.0e4], ids=["60m", "1e4m"])
def test_rotated_shapes(offset):
    xyz = snap(shapes_for_gpu(offset) * [1, 1, 0], 0.04)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1) as cm:
        res = submit_as_voxels(cm, xyz, 0.04)
        for crit in (CLOSENESS, AREA):
            want, table = check(cm, res, 1.0, 5, NONE, crit=crit)
            assert len(table) == 20 and len(set(want["angle"].tolist())) >= 8
            assert (np.abs(np.sort(want["size"][:, :2], axis=1) - [L_WID, L_LEN]).max(axis=1) < 0.4).sum() >= 15


@pytest.mark.gpu
def test_invalid_extent_beside_valid_ones():
    """Kilometres as the unit of thought: leaf 1000 m, tolerance 400 km. Four members 390 km apart span more than 1e6 m; a
    chain of 1400 members 1500 m apart does too and is a large cluster; five L-shapes of 8 members far from both are valid."""
    wide = np.stack([np.arange(4) * 3.9e5, np.zeros(4), np.zeros(4)], axis=1)
    chain = np.stack([np.arange(1400) * 1500.0, np.full(1400, -2.0e6), np.zeros(1400)], axis=1)
    tall = np.stack([np.zeros(4) - 1.0e6, np.arange(4) * 3.9e5, np.zeros(4)], axis=1) + [0, 3.0e6, 0]     # along y
    ell = np.array([[6000.0 * i, 0, 0] for i in range(6)] + [[0, 6000.0, 0], [0, 12000.0, 1000.0]])
    ok = [np.concatenate([rot(ell, 0.3 * (k + 2.5)), ell[:, 2:]], axis=1) + [4.0e6, 1.0e6 * k, 0] for k in range(-2, 3)]
    xyz = snap(np.concatenate([wide, chain, tall] + ok), 1000.0)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1) as cm:
        res = submit_as_voxels(cm, xyz, 1000.0)
        for crit in (CLOSENESS, AREA):
            want, table = check(cm, res, 4.0e5, crit=crit, d_min=1.0)
            assert sorted(table["n_voxels"].tolist()) == [4, 4] + [8] * 5 + [1400]
            assert sorted(table["n_voxels"][want["flags"] == 0].tolist()) == [4, 4, 1400]
            assert np.isnan(want["score"][want["flags"] == 0]).all()


# ---- GPU: frames on every route ------------------------------------------------------------------------------------------
def objects(seed=3, centre=(60.0, 60.0, 0.0)):
    """Forty blobs of 30 .. 3000 points, stretched and turned, on a 5 x 8 lattice of 6 m, far from the cfg2 scene."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(40):
        m = int(30 * 100 ** (k / 39))
        xy = rot(rng.normal(0, 1, (m, 2)) * [0.9, 0.25], rng.uniform(0, np.pi / 2))
        out.append(np.concatenate([xy, rng.normal(0, 0.25, (m, 1))], axis=1) + np.array(centre) + [6.0 * (k % 5), 6.0 * (k // 5), 0.0])
    return np.concatenate(out).astype(F32)


def frame_sensors(n_per=150_000):
    sensors, _ = synth.config2(n_per_sensor=n_per, min_pts=0)
    xyz = objects()
    sensors.append(xyzi_cloud(xyz, np.ones(len(xyz), F32)))
    return sensors, sum(s.n for s in sensors)


def run_frame(cm, sensors, params):
    cm.submit_all(sensors)
    return cm.merge_voxelize(params)


COARSE = dict(leaf=(0.5,) * 3, min_points_per_voxel=0)
CROP = dict(crop_min=(-40.0, -40.0, -10.0), crop_max=(100.0, 120.0, 10.0))


@pytest.mark.gpu
def test_general_route(monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert not res.path_flags & capi.PATH_BUCKET
        check(cm, res, 0.75, 3, 500)
        check(cm, res, 0.75, 3, 500, crit=AREA)


@pytest.mark.gpu
def test_fixed_grid_route(monkeypatch):
    monkeypatch.setenv("CM_QUANT", "0")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        check(cm, res, 0.75, 3, 500)
        check(cm, res, 0.75, 3, 500, crit=AREA)


@pytest.mark.gpu
def test_quantile_route():
    """cfg2's moving stream at 5 cm with a crop box: the frames after the first take the quantile pass."""
    n_per = 150_000
    seen = []
    with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for k in range(2):
            sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
            params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
            res = run_frame(cm, sensors, params)
            seen.append(res.path_flags)
        assert seen[-1] & capi.PATH_QUANTILE, seen
        check(cm, res, 0.1, 2, 2000)
        check(cm, res, 0.1, 2, 2000, crit=AREA)


# ---- GPU: one large cluster ----------------------------------------------------------------------------------------------
def snake(n=24_000, step=0.875, row=150, pitch=3.0):
    """tests/test_cluster.py's one-voxel-wide serpentine: n points `step` apart."""
    pts = []
    x = y = 0.0
    d = 1
    while len(pts) < n:
        for _ in range(row):
            pts.append((x, y)); x += d * step
        x -= d * step
        for _ in range(int(pitch / step)):
            y += step; pts.append((x, y))
        y += step
        d = -d
    return np.array([(px, py, 0.0) for px, py in pts[:n]], F32)


@pytest.mark.gpu
def test_a_snake_of_24000_voxels():
    turn = lambda p, th: np.concatenate([rot(p[:, :2].astype(np.float64), th), p[:, 2:]], axis=1)
    decoys = [turn(snake(600, row=40), 0.3) + [0, -200.0, 0], turn(snake(300, row=25), 1.1) + [0, -300.0, 0]]
    allp = np.concatenate([turn(snake(), 0.5) + [300.0, 0, 0]] + decoys).astype(F32)
    with capi.CloudMerger(max_points_total=len(allp), max_sensors=1) as cm:
        res = submit_as_voxels(cm, allp, 0.25, 0)
        for crit in (CLOSENESS, AREA):
            want, table = check(cm, res, 1.0, crit=crit)
            assert sorted(table["n_voxels"].tolist()) == [300, 600, 24_000]


# ---- GPU: refusals, capacity, determinism, non-interference ----------------------------------------------------------------
def refused(cm, tol=0.5, lo=1, hi=NONE, n_angles=90, crit=CLOSENESS, d_min=0.01):
    for call in (cm.cluster_boxes, cm.cluster_boxes_device):
        with pytest.raises(capi.CloudMergeError) as e:
            call(tol, lo, hi, n_angles, crit, d_min)
        assert e.value.status == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)
    p = capi.CloudMerger.box_params(tol, lo, hi, n_angles, crit, d_min)
    n = C.c_uint64(99)
    assert cm._lib.cm_result_cluster_boxes(cm._ctx, C.byref(p), None, 0, C.byref(n)) == capi.BAD_ARG and n.value == 0


@pytest.mark.gpu
def test_refusals():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:
        refused_raw = lambda: cm._lib.cm_result_cluster_boxes(cm._ctx, C.byref(capi.CloudMerger.box_params(0.5)), None, 0,
                                                              C.byref(C.c_uint64()))
        assert refused_raw() == capi.BAD_ARG and cm._lib.cm_last_error(cm._ctx)     # no result yet
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        assert refused_raw() == capi.BAD_ARG and b"flight" in cm._lib.cm_last_error(cm._ctx)
        res = cm.wait()
        assert res.status == capi.OK
        for tol in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):            # what cm_result_clusters refuses
            refused(cm, tol)
        refused(cm, 0.5, 0, 10)
        refused(cm, 0.5, 5, 4)
        for n_angles in (0, 181, 2 ** 32 - 1):
            refused(cm, n_angles=n_angles)
        for crit in (2, 2 ** 32 - 1):
            refused(cm, crit=crit)
        for d_min in (0.0, -0.01, float("nan"), float("inf")):
            refused(cm, d_min=d_min)
        n = C.c_uint64(99)
        assert cm._lib.cm_result_cluster_boxes(cm._ctx, None, None, 0, C.byref(n)) == capi.BAD_ARG and n.value == 0
        for d_min in (0.0, float("nan")):                                          # AREA ignores d_min
            assert len(cm.cluster_boxes(0.75, criterion=AREA, d_min=d_min)) >= 2
        check(cm, res, 0.75)                                                       # ... and a valid call afterwards succeeds
        res = run_frame(cm, sensors, MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0))
        assert res.status == capi.GRID_OVERFLOW                                    # no voxel grid
        refused(cm)
        cm.submit_all(sensors)
        res = cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40))
        assert res.status == capi.OK
        refused(cm)                                                                # a partial table
        res = run_frame(cm, sensors, params)
        check(cm, res, 0.75)


@pytest.mark.gpu
def test_capacity_and_zero_clusters():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:
        res = run_frame(cm, sensors, MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0))
        want, _ = expected(cm, res, 0.75, 2, 1000)
        k = len(want)
        p = capi.CloudMerger.box_params(0.75, 2, 1000)
        out = np.zeros(k, capi.BOX_DTYPE)
        for cap in (k - 1, 0, k):
            n = C.c_uint64(99)
            st = cm._lib.cm_result_cluster_boxes(cm._ctx, C.byref(p), out.ctypes.data if cap else None, cap, C.byref(n))
            assert st == (capi.CAPACITY if cap < k else capi.OK) and n.value == k, cap
            if cap < k:
                assert cm._lib.cm_last_error(cm._ctx) and not out.view(np.uint8).any()      # nothing was copied
        assert out.tobytes() == want.tobytes()
        # no component passes the filter: CM_OK, zero boxes, a NULL device pointer
        assert len(cm.cluster_boxes(0.75, res.n_out + 1, NONE)) == 0
        assert cm.cluster_boxes_device(0.75, res.n_out + 1, NONE) == (None, 0)


@pytest.mark.gpu
def test_deterministic_and_stage_names():
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        frame_stages = [n for n, _ in cm.stage_times()]
        assert not any(n.startswith("k_box_") for n in frame_stages)
        cm.clusters(0.75, 3, 500)
        cluster_stages = [n for n, _ in cm.stage_times()]
        a = cm.cluster_boxes(0.75, 3, 500)
        names = [n for n, _ in cm.stage_times()]
        # the cluster call's list, then the call's own: with more than 1024 clustered voxels the chunk-wise launches are made
        assert names[:len(cluster_stages)] == cluster_stages, names
        assert names[len(cluster_stages):] == ["k_box_fit", "k_box_extremes", "k_box_sums", "k_box_choose"], names
        cm.cluster_boxes(0.75, 3, 500, criterion=AREA)                   # no sums under AREA
        assert [n for n, _ in cm.stage_times()][len(cluster_stages):] == ["k_box_fit", "k_box_extremes", "k_box_choose"]
        cm.cluster_boxes(0.75, 233, 500)                                 # few clustered voxels: the fit alone
        assert [n for n, _ in cm.stage_times() if n.startswith("k_box_")] == ["k_box_fit"]
        assert a.tobytes() == cm.cluster_boxes(0.75, 3, 500).tobytes()
        for other in (dict(n_angles=45), dict(criterion=AREA), dict(d_min=0.2)):
            b = cm.cluster_boxes(0.75, 3, 500, **other)
            assert b.shape == a.shape and b.tobytes() != a.tobytes(), other
        assert cm.cluster_boxes(0.5, 3, 500).tobytes() != a.tobytes()
        run_frame(cm, sensors, MergeParams(**COARSE))                    # a frame's own list never holds the call's stages
        assert not any(n.startswith("k_box_") for n, _ in cm.stage_times())


@pytest.mark.gpu
def test_requests_do_not_change_later_frames():
    """Two identical 12-frame streams on two contexts; one asks for boxes after every frame."""
    n_per = 100_000
    runs = []
    for ask in (False, True):
        out = []
        with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for k in range(12):
                sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2, wide=(k == 7))
                if k % 4 == 3:
                    params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
                res = run_frame(cm, sensors, params)
                if ask:
                    crit = (AREA, CLOSENESS)[k % 2]
                    boxes = cm.cluster_boxes(0.1, 2, 5000, criterion=crit)
                    # (these clusters are mostly pairs, which under CLOSENESS tie at every heading: angle 0)
                    assert len(boxes) >= 2 and (boxes["flags"] == 1).all() and (crit == CLOSENESS or boxes["angle"].any())
                cells, counts = cm.cells(res.n_out)
                out.append((res.status, res.n_out, res.path_flags, cm.result(res.n_out).tobytes(), cells.tobytes(),
                            counts.tobytes()))
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {k} differs"
    assert any(f[2] & capi.PATH_QUANTILE for f in runs[0])
