"""Statistical outlier removal before the voxel grid (cm_set_statistical_outlier, include/cloudmerge.h; cm_kernels_sor.hip;
DESIGN.md §13).

The bar: the per-point mean distances d_i, the statistics and the surviving cloud bit for bit against the numpy restatement
(tests/sor_ref.py) fed with the stage's input — the frame's merged cloud with the stage off. The voxel result equals that of
the same library fed the restatement's kept points. On every route, with and without crop, with deskew, for every search
cell, and without any effect once the stage is switched off."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import sor_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")


# ---- CPU: the C-ABI surface -------------------------------------------------------------------------------------------
def test_sor_structs_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n",sizeof(cm_sor_params),'
                   'offsetof(cm_sor_params,std_mul),offsetof(cm_sor_params,search_cell),sizeof(cm_sor_stats),'
                   'offsetof(cm_sor_stats,n_removed),offsetof(cm_sor_stats,mean),offsetof(cm_sor_stats,stddev),'
                   'offsetof(cm_sor_stats,threshold),sizeof(cm_result),CM_SOR_MAX_K);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = capi.SorParams, capi.SorStats
    want = [C.sizeof(P), P.std_mul.offset, P.search_cell.offset, C.sizeof(S), S.n_removed.offset, S.mean.offset,
            S.stddev.offset, S.threshold.offset, C.sizeof(capi.Result), capi.SOR_MAX_K]
    assert got == want and got[0] == 16 and got[3] == 40


def test_sor_symbols_and_flag_in_header():
    text = open(HEADER).read()
    for name in ("cm_set_statistical_outlier", "cm_get_sor_stats", "cm_sor_distances_copy"):
        assert name in capi.SYMBOLS and re.search(r"CM_API int " + name + r"\(", text)
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(CM_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text)}
    assert defines["CM_PATH_SOR"] == capi.PATH_SOR and defines["CM_SOR_MAX_K"] == 64


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.SorParams(8, 1.0, 0.0, 0)
    s = capi.SorStats()
    n = C.c_uint64()
    assert L.cm_set_statistical_outlier(None, C.byref(p)) == capi.BAD_ARG
    assert L.cm_set_statistical_outlier(None, None) == capi.BAD_ARG
    assert L.cm_get_sor_stats(None, C.byref(s)) == capi.BAD_ARG
    assert L.cm_sor_distances_copy(None, None, 0, C.byref(n)) == capi.BAD_ARG


# ---- CPU: the exact sum (cm_sor_sum.hpp) against math.fsum -------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "cm_sor_sum.hpp"
int main() {
    unsigned long long bins[CM_SOR_BINS];
    unsigned n;
    while (std::scanf("%u", &n) == 1) {
        std::memset(bins, 0, sizeof bins);
        for (unsigned i = 0; i < n; ++i) {
            unsigned u, reps;
            if (std::scanf("%x %u", &u, &reps) != 2) return 2;
            float f;
            std::memcpy(&f, &u, 4);
            uint32_t e, m;
            cm_sor_split(f, &e, &m);
            bins[e] += static_cast<unsigned long long>(m) * reps;
        }
        const double r = cm_sor_bins_to_double(bins);
        unsigned long long b;
        std::memcpy(&b, &r, 8);
        std::printf("%016llx\n", b);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exact_sum(tmp_path_factory):
    d = tmp_path_factory.mktemp("sorsum")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(d / "drv.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        """cases: list of lists of (float32 value, repetitions). Returns the doubles."""
        lines = []
        for case in cases:
            lines.append(str(len(case)))
            for v, reps in case:
                lines.append("%08x %d" % (int(np.float32(v).view(np.uint32)), reps))
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return [np.uint64(int(h, 16)).view(np.float64) for h in out.split()]
    return run


def fsum_of(case):
    return math.fsum(float(np.float32(v)) for v, reps in case for _ in range(reps))


def test_exact_sum_is_fsum(exact_sum):
    tiny = np.float32(1.4e-45)                                   # the smallest subnormal
    cases = [
        [],
        [(0.0, 5)],
        [(tiny, 1)],
        [(tiny, 3), (np.float32(1.1754942e-38), 2)],            # subnormals up to the largest one
        [(1e-30, 1), (1e30, 1)],
        [(1e30, 1), (1e-30, 7), (3.0, 1)],
        [(3.4028235e38, 4)],                                     # beyond fp32's range, not beyond fp64's
        [(np.float32(0.1), 1 << 20)],                            # 2^20 equal terms
        [(np.float32(1.0) + np.float32(2 ** -23), 3), (np.float32(2 ** -60), 1)],
        [(np.float32(1.0), 1), (np.float32(2.0 ** -53), 1)],     # a tie: rounds to even (1.0)
        [(np.float32(1.0), 1), (np.float32(2.0 ** -53), 1), (np.float32(2.0 ** -100), 1)],   # just above the tie
        [(np.float32(1.0) + np.float32(2 ** -23), 1), (np.float32(2.0 ** -53), 1)],
    ]
    rng = np.random.default_rng(7)
    for _ in range(30):
        v = (rng.lognormal(0.0, 6.0, 50) * rng.choice([1.0, 0.0], 50, p=[0.9, 0.1])).astype(np.float32)
        cases.append([(float(x), int(r)) for x, r in zip(v, rng.integers(1, 5, 50))])
    got = exact_sum(cases)
    for case, g in zip(cases, got):
        want = fsum_of(case)
        assert np.float64(want).view(np.uint64) == np.float64(g).view(np.uint64), (case[:4], g, want)


def test_exact_sum_of_an_infinite_term_is_inf(exact_sum):
    assert exact_sum([[(np.inf, 1), (1.0, 1)]])[0] == np.inf


# ---- CPU: the restatement's known answers -----------------------------------------------------------------------------
def test_known_answer_collinear_points():
    xyz = np.float32([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (10, 0, 0)])
    d, (mean, sd, thr), keep = sr.sor(xyz, 2, 1.0)
    # neighbours: 0 -> 1, 2 (1.5); 1 -> 0, 2 (1); 2 -> 1, 3 (1); 3 -> 2, 1 (1.5); 10 -> 3, 2 (7.5)
    assert d.tolist() == [1.5, 1.0, 1.0, 1.5, 7.5]
    assert mean == 12.5 / 5
    var = (math.fsum([2.25, 1.0, 1.0, 2.25, 56.25]) - 12.5 * 12.5 / 5) / 4
    assert sd == math.sqrt(var) and thr == mean + sd
    assert keep.tolist() == [True, True, True, True, False]


def test_known_answer_duplicates_count_at_distance_zero():
    xyz = np.float32([(0, 0, 0), (0, 0, 0), (0, 0, 4)])
    d, _, _ = sr.sor(xyz, 1, 1.0)
    assert d.tolist() == [0.0, 0.0, 4.0]


def test_known_answer_degenerate_frame():
    d, (mean, sd, thr), keep = sr.sor(np.float32([(0, 0, 0), (1, 0, 0), (5, 0, 0)]), 3, 1.0)
    assert np.isnan(d).all() and math.isnan(mean) and math.isnan(sd) and thr == math.inf and keep.all()


def test_known_answer_lattice_variance_goes_negative():
    """Pairs 0.3 m apart, 1 km from each other: every d_i is the same fp32 value; Q squares it in fp32, and the formula's
    variance comes out slightly negative: stddev and threshold are NaN, and nothing is removed."""
    z = np.repeat(np.arange(8, dtype=np.float32) * np.float32(1000.0), 2)
    x = np.tile(np.float32([0.0, 0.3]), 8)
    xyz = np.stack([x, np.zeros_like(x), z], 1)
    d, (mean, sd, thr), keep = sr.sor(xyz, 1, 1.0)
    assert len(set(d.tolist())) == 1 and d[0] == np.float32(0.3)
    S = math.fsum(d.astype(np.float64).tolist())
    Q = math.fsum((d * d).astype(np.float64).tolist())
    var = (Q - S * S / 16) / 15
    assert var < 0 and mean == S / 16 and math.isnan(sd) and math.isnan(thr)
    assert keep.all()


def test_restatement_search_is_exact():
    rng = np.random.default_rng(3)
    xyz = np.concatenate([rng.normal(0, 1, (3000, 3)), rng.uniform(-60, 60, (20, 3))]).astype(np.float32)
    xyz[5] = xyz[6]
    for k in (1, 8, 30):
        got = sr.knn_d2(xyz, k, cell=0.3)
        want = sr._brute(xyz, np.arange(len(xyz)), k)
        assert np.array_equal(got, want)


def test_restatement_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(11)
    xyz = np.concatenate([rng.normal(0, 2, (20000, 3)), rng.uniform(-100, 100, (50, 3))]).astype(np.float32)
    k = 16
    d2 = sr.knn_d2(xyz, k, cell=0.5)
    dd, ii = spatial.cKDTree(xyz.astype(np.float64)).query(xyz.astype(np.float64), k + 1)
    ref = np.sort(sr._d2(xyz[:, None, :], xyz[ii[:, 1:]]), axis=1)
    # cKDTree ranks in fp64: a neighbour set may differ only among fp32 ties, whose values agree
    assert np.array_equal(d2, ref)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------
def scene(n_per=(40_000, 30_000, 25_000, 20_000), seed=1):
    """Three or four synthetic sensors: a noisy ground and walls, exact duplicates, an exact-tie lattice, a cluster and
    isolated returns 50-200 m from everything."""
    rng = np.random.default_rng(seed)
    sensors = []
    for s, n in enumerate(n_per):
        m = n - 600
        xyz = np.empty((m, 3))
        xyz[:, 0] = rng.uniform(-20, 20, m)
        xyz[:, 1] = rng.uniform(-20, 20, m)
        xyz[:, 2] = rng.normal(-1.5, 0.03, m)
        wall = rng.random(m) < 0.3
        xyz[wall, 2] = rng.uniform(-1.5, 3.0, wall.sum())
        xyz[wall, 1] = 12.0 + rng.normal(0, 0.02, wall.sum())
        dup = rng.integers(0, m, 200)
        lat = np.stack(np.meshgrid(*(np.arange(6) * 0.25,) * 3, indexing="ij"), -1).reshape(-1, 3)[:200] + (30.0 + s, 0, 0)
        far_dir = rng.normal(0, 1, (200, 3))
        far_dir /= np.linalg.norm(far_dir, axis=1, keepdims=True)
        far = far_dir * rng.uniform(50, 200, (200, 1)) + (0, 0, 0)
        far[:, 0] += np.sign(far[:, 0]) * 30.0
        xyz = np.concatenate([xyz, xyz[dup], lat, far]).astype(np.float32)
        sensors.append(xyzi_cloud(xyz, rng.uniform(0, 100, len(xyz)).astype(np.float32)))
    return sensors, sum(c.n for c in sensors)


VOX = dict(leaf=(0.4,) * 3, min_points_per_voxel=2)
CROP = dict(crop_min=(-30.0, -30.0, -5.0), crop_max=(40.0, 30.0, 5.0))


def merged_input(sensors, n_cap, params, motion=None, env=None):
    """The stage's input: the frame's merged cloud with the stage off (same library, same route switches)."""
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(sensors)) as cm:
        if motion is not None:
            cm.set_ego_motion(motion)
        cm.submit_all(sensors)
        res = cm.merge_voxelize(params)
        assert res.status in (capi.OK, capi.EMPTY_INPUT)
        return cm.merged(n_cap)


def xyz_of(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32)


def voxels_of(points_rec, params, n_cap, classic):
    """The voxel result of the library with the stage off, fed these 16-byte records as one cloud with identity pose, on the
    route the frame took (classic: the general path; else the first frame of a context with a crop box: the fixed grid) —
    a voxel of more than 17 points may be added in a different order on another route (CM_PATH_SPLIT)."""
    old = os.environ.get("CM_PATH")
    if classic:
        os.environ["CM_PATH"] = "classic"
    try:
        cm = capi.CloudMerger(max_points_total=max(n_cap, 1), max_sensors=1, flags=capi.FLAG_OCCUPANCY)
    finally:
        if classic:
            if old is None:
                del os.environ["CM_PATH"]
            else:
                os.environ["CM_PATH"] = old
    with cm:
        cloud = xyzi_cloud(xyz_of(points_rec), points_rec["intensity"])
        cm.submit_all([cloud])
        res = cm.merge_voxelize(params)
        if res.status != capi.OK:
            return res.status, None, None, None
        cells, counts = cm.cells(res.n_out)
        return res.status, cm.result(res.n_out).view(np.uint8).tobytes(), cells, counts


def run_sor(sensors, n_cap, params, k, std_mul, cell=0.0, frames=1, motion=None, flags=capi.FLAG_OCCUPANCY):
    """Frames of the stream with the stage on; returns the last frame's figures."""
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(sensors), flags=flags) as cm:
        if motion is not None:
            cm.set_ego_motion(motion)
        cm.set_statistical_outlier(k, std_mul, cell)
        out = []
        for _ in range(frames):
            cm.submit_all(sensors)
            res = cm.merge_voxelize(params)
            d = cm.sor_distances(n_cap)
            st = cm.sor_stats()
            merged = cm.merged(n_cap)
            vox = (cm.result(res.n_out).view(np.uint8).tobytes(), *cm.cells(res.n_out)) if res.status == capi.OK else None
            out.append((res, d, st, merged, vox))
        return out


def check_frame(P, got, k, std_mul, params, n_cap, ref=None):
    res, d, st, merged, vox = got
    ref = ref or sr.sor(xyz_of(P), k, std_mul, cell=0.5 if k <= 10 else 1.0)   # (cell: the restatement's speed only)
    dr, (mean, sd, thr), keep = ref
    assert d.view(np.uint32).tolist() == dr.view(np.uint32).tolist(), "d_i must be bit-exact"
    assert st.n_valid == len(P) and st.n_removed == int((~keep).sum())
    for g, w in ((st.mean, mean), (st.stddev, sd), (st.threshold, thr)):
        assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64) or (math.isnan(g) and math.isnan(w)), (g, w)
    kept = P[keep]
    assert merged.tobytes() == kept.tobytes(), "the surviving cloud differs"
    assert res.path_flags & capi.PATH_SOR
    s2, out2, cells2, counts2 = voxels_of(kept, params, n_cap, not res.path_flags & capi.PATH_BUCKET)
    assert res.status == s2
    if vox is not None:
        assert vox[0] == out2 and np.array_equal(vox[1], cells2) and np.array_equal(vox[2], counts2)
    return ref


# ---- GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8, 30, 64])
def test_distances_and_stats_bit_exact(k, monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    sensors, n_cap = scene()
    params = MergeParams(**VOX)
    P = merged_input(sensors, n_cap, params)
    check_frame(P, run_sor(sensors, n_cap, params, k, 1.0)[0], k, 1.0, params, n_cap)


@pytest.mark.gpu
@pytest.mark.parametrize("route,crop,all_data", [("classic", False, True), ("classic", True, False), ("fixed", True, True),
                                                  ("fixed", False, False), ("auto", True, False), ("auto", False, True)])
def test_end_to_end_on_every_route(route, crop, all_data, monkeypatch):
    if route == "classic":
        monkeypatch.setenv("CM_PATH", "classic")
    elif route == "fixed":
        monkeypatch.setenv("CM_QUANT", "0")
    sensors, n_cap = scene(seed=2)
    params = MergeParams(**VOX, **(CROP if crop else {}), downsample_all_data=all_data)
    P = merged_input(sensors, n_cap, params)
    frames = run_sor(sensors, n_cap, params, 10, 0.5, frames=3)
    ref = None
    for got in frames:
        ref = check_frame(P, got, 10, 0.5, params, n_cap, ref)
        # With the stage on a frame takes the general path, or the fixed-grid passes behind it when the crop box fixes the
        # grid — never the quantile or predicted-box routes (as with the radius stage): "auto" covers the same two routes.
        flags = got[0].path_flags
        assert not flags & (capi.PATH_QUANTILE | capi.PATH_PREDICTED)
        assert bool(flags & capi.PATH_BUCKET) == (crop and route != "classic")


@pytest.mark.gpu
def test_with_deskew():
    views = synth.moving_scene(n_sensors=3, rings=8, azimuths=1500)
    sensors = [xyzi_cloud(v["xyz"], v["intensity"], q_xyzw=v["q_xyzw"], t_xyz=v["t_xyz"]) for v in views]
    motion = capi.make_motion((15.0, 0.5, 0.0), (0.0, 0.0, 0.3), 1_000_000_000_000, [v["stamp_ns"] for v in views])
    n_cap = sum(s.n for s in sensors)
    params = MergeParams(**VOX)
    P = merged_input(sensors, n_cap, params, motion=motion)
    got = run_sor(sensors, n_cap, params, 8, 1.0, motion=motion)[0]
    assert got[0].path_flags & capi.PATH_MOTION
    check_frame(P, got, 8, 1.0, params, n_cap)


@pytest.mark.gpu
def test_search_cell_never_changes_the_result():
    sensors, n_cap = scene(seed=4)
    for extra in ({}, CROP):
        params = MergeParams(**VOX, **extra)
        runs = [run_sor(sensors, n_cap, params, 16, 1.0, cell=c, frames=2)[-1] for c in (0.0, 0.05, 0.7, 6.0, 1e-6)]
        base = runs[0]
        for r in runs[1:]:
            assert r[1].tobytes() == base[1].tobytes() and r[3].tobytes() == base[3].tobytes() and r[4][0] == base[4][0]
            assert (r[2].n_removed, r[2].threshold) == (base[2].n_removed, base[2].threshold)


@pytest.mark.gpu
def test_default_routes_match_the_general_path_across_a_jump(monkeypatch):
    """A stream whose third frame jumps 150 m (what hands a frame back on the predicted route without the stage): with the
    stage on no frame takes that route, and the default routes give the same bytes, distances and survivors as the general
    path. (The hand-back of a frame with the stage: test_hand_back_redoes_the_same_mask.)"""
    sensors, n_cap = scene(seed=5)
    moved, _ = scene(seed=5)
    for c in moved:
        c.data["x"] += np.float32(150.0)
    params = MergeParams(**VOX)
    outs = {}
    for route in ("auto", "classic"):
        if route == "classic":
            monkeypatch.setenv("CM_PATH", "classic")
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY) as cm:
            cm.set_statistical_outlier(8, 1.0)
            got = []
            for s in (sensors, sensors, moved):
                cm.submit_all(s)
                res = cm.merge_voxelize(params)
                assert res.status == capi.OK
                got.append((cm.result(res.n_out).tobytes(), cm.merged(n_cap).tobytes(), cm.sor_distances(n_cap).tobytes()))
            outs[route] = got
    assert outs["auto"] == outs["classic"]


_HANDBACK_CHILD = r"""
import hashlib, json
from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from tests.test_sor import scene, VOX, CROP
sensors, n_cap = scene(seed=7)
params = MergeParams(**VOX, **CROP)
h = lambda b: hashlib.sha256(b).hexdigest()
with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY) as cm:
    cm.set_statistical_outlier(12, 0.7)
    cm.submit_all(sensors)
    cm.merge_voxelize_async(capi.make_params(params))
    cm.set_statistical_outlier(3, 2.0)          # after the enqueue: neither this frame nor a redo of it may read these
    res = cm.wait()
    st = cm.sor_stats()
    cells, counts = cm.cells(res.n_out)
    print(json.dumps({"status": res.status, "flags": int(res.path_flags), "d": h(cm.sor_distances(n_cap).tobytes()),
                      "merged": h(cm.merged(n_cap).tobytes()), "vox": h(cm.result(res.n_out).tobytes()),
                      "cells": h(cells.tobytes() + counts.tobytes()),
                      "stats": [st.n_valid, st.n_removed, st.mean.hex(), st.stddev.hex(), st.threshold.hex()]}))
"""


@pytest.mark.gpu
def test_hand_back_redoes_the_same_mask():
    """A frame with the stage, a crop box and the fixed-grid passes (CM_QUANT=0) handed back inside cm_wait: the test build
    (-DCM_TEST_HOOKS) with CM_DEBUG_MISRANK=1 makes the voxel stage's last global pass swap two records, the finish notices
    and the frame is redone on the general path — the stage included, on the general sort. Distances, statistics, survivors
    and voxels equal those of CM_PATH=classic, and the parameters are those of the enqueue, not of a set call after it.
    Run in child processes: a process loads one build of the library."""
    import json
    import sys
    if not os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")):
        pytest.skip("test build missing: python -m cloud_merger_amd.build --test-hooks")

    def child(**env_extra):
        env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK", "CM_LIB_VARIANT")}
        env.update(env_extra, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", _HANDBACK_CHILD], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    plain = child(CM_LIB_VARIANT="testhooks", CM_QUANT="0")
    redone = child(CM_LIB_VARIANT="testhooks", CM_QUANT="0", CM_DEBUG_MISRANK="1")
    general = child(CM_PATH="classic")
    for r in (plain, redone, general):
        assert r["status"] == capi.OK and r["flags"] & capi.PATH_SOR
    assert plain["flags"] & capi.PATH_BUCKET and not plain["flags"] & capi.PATH_REDONE    # the route the hook breaks
    assert redone["flags"] & capi.PATH_REDONE and not redone["flags"] & capi.PATH_BUCKET  # handed back, redone in general
    assert not general["flags"] & capi.PATH_BUCKET
    for key in ("d", "merged", "stats", "cells"):
        assert redone[key] == general[key] == plain[key], key
    assert redone["vox"] == general["vox"]          # (the fixed-grid finish may add a long voxel in another order)


@pytest.mark.gpu
def test_degenerate_and_empty_frames():
    xyz = np.float32([(0, 0, 0), (1, 0, 0), (0, 1, 0), (5, 5, 5)])
    with capi.CloudMerger(max_points_total=16, max_sensors=1) as cm:
        cm.set_statistical_outlier(4, 1.0)
        cm.submit_all([xyzi_cloud(xyz)])
        res = cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0))
        assert res.status == capi.OK and res.n_merged == 4
        st = cm.sor_stats()
        assert st.n_valid == 4 and st.n_removed == 0 and st.threshold == math.inf and math.isnan(st.mean)
        assert np.isnan(cm.sor_distances(16)).all()
        cm.submit_all([xyzi_cloud(np.zeros((0, 3), np.float32))])
        res = cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0))
        assert res.status == capi.EMPTY_INPUT


@pytest.mark.gpu
def test_refusals():
    sensors, n_cap = scene(n_per=(5000, 5000), seed=6)
    L = capi.load()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2) as cm:
        for bad in (capi.SorParams(0, 1.0, 0.0, 0), capi.SorParams(65, 1.0, 0.0, 0), capi.SorParams(8, math.nan, 0.0, 0),
                    capi.SorParams(8, math.inf, 0.0, 0), capi.SorParams(8, 1.0, -1.0, 0), capi.SorParams(8, 1.0, math.inf, 0)):
            assert L.cm_set_statistical_outlier(cm._ctx, C.byref(bad)) == capi.BAD_ARG
            assert L.cm_last_error(cm._ctx)
        cm.set_statistical_outlier(8, -0.01)                     # a negative multiplier is allowed
        cm.submit_all(sensors)
        p = capi.make_params(MergeParams(**VOX, outlier_radius=0.3))
        res = capi.Result()
        assert L.cm_merge_voxelize(cm._ctx, C.byref(p), C.byref(res)) == capi.BAD_ARG
        assert b"outlier_enable" in L.cm_last_error(cm._ctx)
        p = capi.make_params(MergeParams(**VOX, **CROP))
        assert L.cm_merge_partial(cm._ctx, C.byref(p), None, C.byref(res)) == capi.BAD_ARG
        assert b"partial" in L.cm_last_error(cm._ctx)
        mn, mx, n = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint64()
        assert L.cm_local_bounds(cm._ctx, C.byref(p), mn, mx, C.byref(n)) == capi.BAD_ARG
        assert b"cm_local_bounds" in L.cm_last_error(cm._ctx)
        cm.set_ground_removal(capi.make_ground_params([[(-50.0, 100.0, 0.2)]]))
        assert L.cm_merge_voxelize(cm._ctx, C.byref(p), C.byref(res)) == capi.BAD_ARG
        assert b"ground" in L.cm_last_error(cm._ctx)
        cm.set_ground_removal(None)
        res = cm.merge_voxelize(MergeParams(**VOX))           # the refused calls lost no frame
        assert res.status == capi.OK and res.path_flags & capi.PATH_SOR


@pytest.mark.gpu
def test_switch_off_leaves_no_trace():
    frames = [synth.config2_stream(f, n_per_sensor=30_000, n_sensors=3)[0] for f in range(12)]
    params = MergeParams(**VOX)
    n_cap = max(sum(s.n for s in fr) for fr in frames)

    def stream(cm, idx):
        out = []
        for f in idx:
            cm.submit_all(frames[f])
            res = cm.merge_voxelize(params)
            out.append((res.status, res.path_flags, cm.result(res.n_out).tobytes()))
        return out
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        cm.set_statistical_outlier(8, 1.0)
        on = stream(cm, range(6))
        assert all(pf & capi.PATH_SOR for _, pf, _ in on)
        cm.set_statistical_outlier(None)
        after = stream(cm, range(6, 12))
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        fresh = stream(cm, range(6, 12))
    assert after == fresh


@pytest.mark.gpu
def test_full_size_cfg2():
    sensors, params = synth.config2(n_per_sensor=1_000_000, min_pts=0)
    n_cap = sum(s.n for s in sensors)
    k = 30
    P = merged_input(sensors, n_cap, params)
    res, d, st, merged, _ = run_sor(sensors, n_cap, params, k, 1.0)[0]
    assert res.status == capi.OK and len(d) == len(P) == st.n_valid
    xyz = xyz_of(P)
    # the queries' k nearest by brute force inside an x-slab around each, widened until the k-th lies inside it
    order = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[order, 0]
    rng = np.random.default_rng(0)
    q = rng.choice(len(xyz), 20_000, replace=False)
    want = np.empty(len(q), np.float32)
    for t, i in enumerate(q):
        half = 0.1
        while True:
            lo, hi = np.searchsorted(xs, xyz[i, 0] - half), np.searchsorted(xs, xyz[i, 0] + half, side="right")
            cand = order[lo:hi]
            cand = cand[cand != i]
            dd = sr._d2(xyz[i][None, :], xyz[cand])
            if len(dd) >= k:
                top = np.sort(np.partition(dd, k - 1)[:k])
                if top[-1] <= np.float32(half * half * 0.999):
                    break
            half *= 2.0
        s = 0.0
        for v in np.sqrt(top):
            s = s + float(v)
        want[t] = np.float32(s / k)
    assert np.array_equal(want.view(np.uint32), d[q].view(np.uint32))
    mean, sd, thr = sr.stats(d, k, 1.0)
    assert (st.mean, st.stddev, st.threshold) == (mean, sd, thr)
    keep = sr.keep_mask(d, thr)
    assert st.n_removed == int((~keep).sum()) and merged.tobytes() == P[keep].tobytes()
