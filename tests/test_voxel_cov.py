"""Per-voxel covariance of the result (NDT voxel statistics): cm_result_voxel_cov / cm_result_voxel_cov_device
(include/cloudmerge.h, cm_kernels_cov.hip).

The bar: count and mean bit for bit against the numpy restatement (tests/voxel_cov_ref.py) fed with the frame's own merged
cloud and cells, and so is the covariance of every voxel that was not inflated; what goes through an eigen-decomposition
(inflated covariance, eigenvalues, inverse) within tolerances. On every route, with the pre-stages, and without any effect
on later frames. eigh is another algorithm than the kernel's Jacobi, which makes this the independent cross-check and
makes it look away at the zero-eigenvalue boundary; tests/test_voxel_cov_edges.py compares whole entries byte for byte
with the kernel-order restatement (tests/voxel_cov_exact.py) on frames designed to live at that boundary."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, SensorCloud, xyzi_cloud
from tests import voxel_cov_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_cov_structs_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(cm_cov_params),'
                   'offsetof(cm_cov_params,eig_mult),sizeof(cm_voxel_cov),offsetof(cm_voxel_cov,mean),'
                   'offsetof(cm_voxel_cov,count),offsetof(cm_voxel_cov,cov),offsetof(cm_voxel_cov,icov),'
                   'offsetof(cm_voxel_cov,evals),offsetof(cm_voxel_cov,flags),sizeof(cm_result));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    V = capi.VoxelCov
    want = [C.sizeof(capi.CovParams), capi.CovParams.eig_mult.offset, C.sizeof(V), V.mean.offset, V.count.offset,
            V.cov.offset, V.icov.offset, V.evals.offset, V.flags.offset, C.sizeof(capi.Result)]
    assert got == want and got[2] == 80
    d = capi.VOXEL_COV_DTYPE
    assert [d.fields[k][1] for k in ("mean", "count", "cov", "icov", "evals", "flags")] == want[3:9]


def test_cov_flags_mirror_the_header():
    text = open(HEADER).read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(CM_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text)}
    assert capi.COV_VALID == defines["CM_COV_VALID"] and capi.COV_INFLATED == defines["CM_COV_INFLATED"]
    assert defines["CM_VERSION"] == 100


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CovParams(6, 0.01)
    buf = np.zeros(4, dtype=capi.VOXEL_COV_DTYPE)
    assert L.cm_result_voxel_cov(None, C.byref(p), buf.ctypes.data, 4) == capi.BAD_ARG
    assert L.cm_result_voxel_cov(None, None, None, 0) == capi.BAD_ARG
    ptr, n = C.c_void_p(), C.c_uint64()
    assert L.cm_result_voxel_cov_device(None, C.byref(p), C.byref(ptr), C.byref(n)) == capi.BAD_ARG


def one_voxel(pts, min_points=6, eig_mult=0.01):
    pts = np.asarray(pts, dtype=np.float32)
    t, lam = vr.voxel_stats(pts, np.zeros(len(pts), np.int64), 1, min_points, eig_mult)
    return t[0], lam[0]


def test_known_answer_tetrahedron():
    """(0,0,0) (1,0,0) (0,1,0) (0,0,1): population covariance 3/16 on the diagonal, -1/16 off it; PCL's (n-1)/n makes that
    9/64 and -3/64 (the textbook n/(n-1) would give 1/4). Eigenvalues 3/64, 12/64, 12/64: not inflated. Inverse (16/3)(I + J)."""
    e, _ = one_voxel([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], min_points=3)
    assert e["count"] == 4 and np.array_equal(e["mean"], np.float32([0.25, 0.25, 0.25]))
    assert np.array_equal(e["cov"], np.float32([9, -3, -3, 9, -3, 9]) / np.float32(64))
    assert e["flags"] == capi.COV_VALID
    assert np.allclose(e["evals"], [3 / 64, 12 / 64, 12 / 64], rtol=1e-6)
    assert np.allclose(e["icov"], np.array([2, 1, 1, 2, 1, 2]) * 16 / 3, rtol=1e-5)


def test_known_answer_planar_voxel_is_inflated():
    """Six points on z = 0: C has an exact zero row, lambda_0 = 0 is raised to 0.01 lambda_2 and C rebuilt."""
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (.5, .5, 0), (.25, .75, 0)]
    e, lam = one_voxel(pts)
    assert lam[0] == 0.0
    assert e["flags"] == capi.COV_VALID | capi.COV_INFLATED
    l2 = e["evals"][2]
    assert l2 > 0 and e["evals"][0] == np.float32(np.float64(np.float32(0.01)) * lam[2])
    c = capi.sym6_to_3x3(e["cov"].astype(np.float64))
    assert abs(c[2, 2] - 0.01 * l2) < 1e-7 and abs(c[0, 2]) < 1e-7 and abs(c[1, 2]) < 1e-7
    # in-plane block untouched by the inflation (population covariance times 5/6)
    x = np.array([p[0] for p in pts])
    assert abs(c[0, 0] - x.var() * 5 / 6) < 1e-7
    assert np.allclose(capi.sym6_to_3x3(e["icov"].astype(np.float64)) @ c, np.eye(3), atol=1e-4)


def test_known_answer_identical_points_are_invalid():
    e, _ = one_voxel([(1.0, -2.0, 0.5)] * 8)
    assert e["count"] == 8 and np.array_equal(e["mean"], np.float32([1.0, -2.0, 0.5]))
    assert e["flags"] == 0 and not e["cov"].any() and not e["icov"].any() and not e["evals"].any()


def test_known_answer_below_min_points_has_count_and_mean_only():
    e, _ = one_voxel([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], min_points=6)
    assert e["count"] == 5 and np.array_equal(e["mean"], np.float32([0.4, 0.4, 0.4]))
    assert e["flags"] == 0 and not e["cov"].any() and not e["icov"].any() and not e["evals"].any()


def test_restatement_sums_are_sequential():
    """The restatement adds point after point: 1e16, 1, -1e16, 1 gives 1 in order (pairwise summation would give 2 or 0)."""
    pts = np.float32([(1e16, 0, 0), (1, 0, 0), (-1e16, 0, 0), (1, 0, 0)])
    e, _ = one_voxel(pts, min_points=3)
    assert e["mean"][0] == np.float32(((1e16 + 1.0) - 1e16 + 1.0) / 4)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def check_table(cm, res, leaf, n_cap, min_points=6, eig_mult=0.01):
    """The frame's table against the restatement; returns (valid, inflated, invalid) counts."""
    assert res.status == capi.OK
    t = cm.voxel_covariance(res.n_out, min_points, eig_mult)
    merged = cm.merged(n_cap)
    cells, counts = cm.cells(res.n_out)
    ref, lam = vr.voxel_cov(merged, cells, counts, leaf, min_points, eig_mult)
    assert np.array_equal(t["count"], ref["count"])
    assert np.array_equal(t["mean"].view(np.uint32), ref["mean"].view(np.uint32)), "means must be bit-exact"
    l2 = np.abs(lam[:, 2])
    near = (np.abs(lam[:, 0]) <= 1e-12 * l2) | (np.abs(lam[:, 1]) <= 1e-12 * l2)
    far = ~near
    assert np.array_equal(t["flags"][far], ref["flags"][far]), "flags differ away from the zero-eigenvalue boundary"
    same = t["flags"] == ref["flags"]
    big = t["count"] >= min_points
    plain = same & big & ((t["flags"] & capi.COV_INFLATED) == 0)
    assert np.array_equal(t["cov"][plain].view(np.uint32), ref["cov"][plain].view(np.uint32)), "covariance must be bit-exact"
    assert not t["cov"][~big].any() and not t["icov"][~big].any()
    ok = same & ((t["flags"] & capi.COV_VALID) != 0)
    infl = ok & ((t["flags"] & capi.COV_INFLATED) != 0)
    tol = 1e-5 * np.abs(ref["evals"][:, 2].astype(np.float64))[:, None]
    assert (np.abs(t["cov"][infl].astype(np.float64) - ref["cov"][infl]) <= tol[infl]).all()
    assert (np.abs(t["evals"][ok].astype(np.float64) - ref["evals"][ok]) <= tol[ok]).all()
    scale = np.abs(ref["icov"][ok].astype(np.float64)).max(axis=1, keepdims=True)
    assert (np.abs(t["icov"][ok].astype(np.float64) - ref["icov"][ok]) <= 1e-4 * scale).all()
    inv = ~ok & same & big
    assert not t["icov"][inv].any() and not t["evals"][inv].any()
    return int(ok.sum()), int(infl.sum()), int((big & ((t["flags"] & capi.COV_VALID) == 0)).sum())


def tilted_plane(n=20_000, seed=5, centre=(60.0, 60.0, 0.0), sigma=0.0):
    """A plane (normal ~ (0.3, -0.2, 1)) — exact up to fp32 rounding, or sigma metres thick — far from the cfg2 scene,
    plus a cluster of identical points."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.3, -0.2, 1.0]); nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [1.0, 0, 0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    uv = rng.uniform(-4, 4, (n, 2))
    xyz = np.array(centre) + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0.0, sigma, (n, 1)) * nrm
    same = np.tile([70.25, 70.25, 0.25], (12, 1))
    return np.concatenate([xyz, same]).astype(np.float32), nrm


def frame_sensors(n_per=150_000, plane=True):
    sensors, _ = synth.config2(n_per_sensor=n_per, min_pts=0)
    if plane:
        xyz, _ = tilted_plane()
        sensors.append(xyzi_cloud(xyz, np.ones(len(xyz), np.float32)))
    return sensors, sum(s.n for s in sensors)


def run_frame(cm, sensors, params):
    cm.submit_all(sensors)
    return cm.merge_voxelize(params)


COARSE = dict(leaf=(0.5,) * 3, min_points_per_voxel=0)
CROP = dict(crop_min=(-40.0, -40.0, -10.0), crop_max=(80.0, 80.0, 10.0))


def totals(acc, r):
    return tuple(a + b for a, b in zip(acc, r))


# ---- GPU: every route -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_general_route(monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert not res.path_flags & capi.PATH_BUCKET
        valid, infl, invalid = check_table(cm, res, COARSE["leaf"], n_cap)
    assert valid >= 1000 and infl >= 100 and invalid >= 1, (valid, infl, invalid)


@pytest.mark.gpu
def test_fixed_grid_route(monkeypatch):
    monkeypatch.setenv("CM_QUANT", "0")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        valid, infl, invalid = check_table(cm, res, COARSE["leaf"], n_cap)
    assert valid >= 1000 and infl >= 100 and invalid >= 1, (valid, infl, invalid)


@pytest.mark.gpu
def test_quantile_and_predicted_box_routes():
    """cfg2's moving stream at 5 cm: with a crop box the frames after the first take the quantile pass; without one they
    run in the box predicted from their predecessors."""
    n_per = 150_000
    for crop, want in ((dict(crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3), capi.PATH_QUANTILE), ({}, capi.PATH_PREDICTED)):
        flags = []
        with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for k in range(3):
                sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
                params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, **crop)
                res = run_frame(cm, sensors, params)
                check_table(cm, res, params.leaf, 4 * n_per, min_points=3)
                flags.append(res.path_flags)
        assert all(f & capi.PATH_BUCKET for f in flags), flags
        assert any(f & want for f in flags[1:]), flags


@pytest.mark.gpu
def test_predicted_box_route_coarse():
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        acc = (0, 0, 0)
        for k in range(2):
            res = run_frame(cm, sensors, MergeParams(**COARSE))
            acc = totals(acc, check_table(cm, res, COARSE["leaf"], n_cap))
        assert res.path_flags & capi.PATH_PREDICTED
    assert acc[0] >= 1000 and acc[1] >= 100 and acc[2] >= 1, acc


@pytest.mark.gpu
def test_one_metre_leaf_stays_on_the_fixed_grid():
    """Voxels of thousands of points, each summed by one lane."""
    sensors, n_cap = frame_sensors(n_per=600_000)
    leaf = (1.0,) * 3
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(leaf=leaf, min_points_per_voxel=0, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        counts = cm.cells(res.n_out)[1]
        assert counts.max() >= 1000
        valid, infl, invalid = check_table(cm, res, leaf, n_cap)
    assert valid >= 100 and invalid >= 1


# ---- GPU: pre-stages --------------------------------------------------------------------------------------------------
FRONT_SLABS = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]


@pytest.mark.gpu
def test_with_deskew():
    sensors, n_cap = frame_sensors()
    t_ref = 1_700_000_000_000_000_000
    m = capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000 * (s + 1) for s in range(5)])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ego_motion(m)
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_MOTION
        valid, infl, invalid = check_table(cm, res, COARSE["leaf"], n_cap)
    assert valid >= 1000 and infl >= 100, (valid, infl, invalid)


@pytest.mark.gpu
def test_with_ground_removal():
    sensors, n_cap = frame_sensors(plane=False)
    gp = capi.make_ground_params([FRONT_SLABS] * 4)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(gp)
        res = run_frame(cm, sensors, MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=2,
                                                 crop_min=(-30.0, -30.0, -10.0), crop_max=(30.0, 30.0, 10.0)))
        assert len(cm.ground(n_cap)) > 0
        valid, _, _ = check_table(cm, res, (0.5,) * 3, n_cap)
    assert valid >= 1000


@pytest.mark.gpu
def test_with_outlier_stage():
    sensors, n_cap = frame_sensors()
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, outlier_radius=0.15, outlier_min_neighbors=2, **CROP)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, params)
        assert len(cm.merged(n_cap)) < n_cap
        valid, infl, _ = check_table(cm, res, (0.5,) * 3, n_cap)
    assert valid >= 1000 and infl >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("mppv,min_points", [(0, 6), (2, 6), (6, 6), (6, 10)])
def test_min_points_per_voxel(monkeypatch, mppv, min_points):
    monkeypatch.setenv("CM_PATH", "classic")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=mppv))
        check_table(cm, res, (0.25,) * 3, n_cap, min_points=min_points)
        t = cm.voxel_covariance(res.n_out, min_points)
    assert t["count"].min() >= max(mppv, 1)
    low = t["count"] < min_points
    assert low.any() == (min_points > mppv) and not t["flags"][low].any() and not t["cov"][low].any()


# ---- GPU: non-interference, determinism, refusals, physics -------------------------------------------------------------
@pytest.mark.gpu
def test_requests_do_not_change_later_frames():
    """Two identical 12-frame streams on two contexts; one asks for the table after every frame."""
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
                    cm.voxel_covariance(res.n_out, min_points=3)
                cells, counts = cm.cells(res.n_out)
                out.append((res.status, res.n_out, res.path_flags, cm.result(res.n_out).tobytes(), cells.tobytes(),
                            counts.tobytes()))
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {k} differs"
    assert any(f[2] & capi.PATH_QUANTILE for f in runs[0])


@pytest.mark.gpu
def test_deterministic_and_device_copy_matches():
    try:
        hip = C.CDLL("libamdhip64.so.7")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        a = cm.voxel_covariance(res.n_out)
        b = cm.voxel_covariance(res.n_out)
        assert a.tobytes() == b.tobytes()
        ptr, n = cm.voxel_covariance_device()
        assert n == res.n_out and ptr
        d = np.zeros(n, dtype=capi.VOXEL_COV_DTYPE)
        assert hip.hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(n * 80), 2) == 0
        assert d.tobytes() == a.tobytes()
        c = cm.voxel_covariance(res.n_out, 8, 0.05)          # other parameters, then the defaults again
        assert c.tobytes() != a.tobytes()
        assert cm.voxel_covariance(res.n_out).tobytes() == a.tobytes()


def refused(cm, n=16, min_points=6, eig_mult=0.01, code=capi.BAD_ARG):
    with pytest.raises(capi.CloudMergeError) as e:
        cm.voxel_covariance(n, min_points, eig_mult)
    assert e.value.status == code and cm._lib.cm_last_error(cm._ctx)
    with pytest.raises(capi.CloudMergeError) as e:
        cm.voxel_covariance_device(min_points, eig_mult)
    if code == capi.BAD_ARG:
        assert e.value.status == code


@pytest.mark.gpu
def test_refusals():
    sensors, params = synth.config2(n_per_sensor=20_000, min_pts=0)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:                # no CM_FLAG_OCCUPANCY
        res = run_frame(cm, sensors, params)
        refused(cm, res.n_out)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        refused(cm)                                                                     # no result yet
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        refused(cm)                                                                     # frame in flight
        res = cm.wait()
        assert res.status == capi.OK
        refused(cm, res.n_out, min_points=2)
        refused(cm, res.n_out, eig_mult=-0.1)
        refused(cm, res.n_out, eig_mult=1.5)
        refused(cm, res.n_out, eig_mult=float("nan"))
        with pytest.raises(capi.CloudMergeError) as e:
            cm.voxel_covariance(res.n_out - 1)
        assert e.value.status == capi.CAPACITY
        assert len(cm.voxel_covariance(res.n_out, 3, 0.0)) == res.n_out
        assert len(cm.voxel_covariance(res.n_out, 3, 1.0)) == res.n_out
        # a grid that overflows PCL's int32 index: CM_GRID_OVERFLOW, no voxel grid
        tiny = MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)
        res = run_frame(cm, sensors, tiny)
        assert res.status == capi.GRID_OVERFLOW
        refused(cm, res.n_out)
        # an empty frame
        for s in range(4):
            cm.clear(s)
        cm.submit(0, xyzi_cloud(np.full((4, 3), np.nan, np.float32)))
        res = cm.merge_voxelize(params)
        assert res.status == capi.EMPTY_INPUT
        refused(cm)
        # a partial table (fused cloud across GPUs), then merged tables
        cm.submit_all(sensors)
        res = cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40))
        assert res.status == capi.OK
        refused(cm, res.n_out)
        ptr, n = cm.partial_device()
        res = cm.merge_tables([ptr], [n], params)
        assert res.status == capi.OK
        refused(cm, res.n_out)


@pytest.mark.gpu
def test_tilted_plane_normal_from_icov():
    """A 1 mm thick tilted plane (an exact one this far out is below the fp64 cancellation of PCL's one-pass formula:
    its lambda_0 comes out with either sign)."""
    xyz, nrm = tilted_plane(centre=(20.0, -10.0, 1.0), sigma=0.001)
    cloud = xyzi_cloud(xyz, np.ones(len(xyz), np.float32))
    leaf = (0.5,) * 3
    with capi.CloudMerger(max_points_total=cloud.n, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.submit(0, cloud)
        res = cm.merge_voxelize(MergeParams(leaf=leaf, min_points_per_voxel=0))
        t = cm.voxel_covariance(res.n_out)
    sel = ((t["flags"] & capi.COV_VALID) != 0) & (t["count"] >= 50) & (t["evals"][:, 1] > 2.0 * t["evals"][:, 0])
    assert sel.sum() >= 50
    icov = capi.sym6_to_3x3(t["icov"][sel].astype(np.float64))
    _, vec = np.linalg.eigh(icov)
    n_got = vec[:, :, 2]                                      # largest eigenvalue of the inverse: 1 / lambda_0
    ang = np.degrees(np.arccos(np.clip(np.abs(n_got @ nrm), 0, 1)))
    assert ang.max() < 1.0, ang.max()
    assert (t["flags"][sel] & capi.COV_INFLATED).all()
