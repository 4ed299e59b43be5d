"""Euclidean cluster extraction on the result: cm_result_clusters / cm_result_clusters_device (include/cloudmerge.h,
cm_kernels_cluster.hip).

The bar: labels, every field of the cluster table and the member lists EXACTLY equal to the restatement
(tests/cluster_ref.py: clusters_tree) fed with the frame's own result — the answer is a set partition, so there is no
tolerance anywhere. No test passes vacuously: before the device is looked at, the restatement's own output must hold at least
two clusters, a dropped component wherever a size filter is in play, and differ from both trivial labellings."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import cluster_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")
NONE = cr.NONE
F32 = np.float32


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_cluster_structs_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",sizeof(cm_cluster_params),'
                   'offsetof(cm_cluster_params,tolerance),offsetof(cm_cluster_params,min_cluster_size),'
                   'offsetof(cm_cluster_params,max_cluster_size),sizeof(cm_cluster),offsetof(cm_cluster,first),'
                   'offsetof(cm_cluster,n_voxels),offsetof(cm_cluster,n_points),offsetof(cm_cluster,_pad),'
                   'offsetof(cm_cluster,min),offsetof(cm_cluster,max),(size_t)(CM_CLUSTER_NONE == 0xFFFFFFFFu));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, K = capi.ClusterParams, capi.Cluster
    want = [C.sizeof(P), P.tolerance.offset, P.min_cluster_size.offset, P.max_cluster_size.offset, C.sizeof(K), K.first.offset,
            K.n_voxels.offset, K.n_points.offset, K._pad.offset, K.min.offset, K.max.offset, 1]
    assert got == want and got[0] == 16 and got[4] == 40
    d = capi.CLUSTER_DTYPE
    assert [d.fields[k][1] for k in ("first", "n_voxels", "n_points", "_pad", "min", "max")] == want[5:11]
    assert d == cr.CLUSTER_DTYPE


def test_cluster_none_mirrors_the_header():
    text = open(HEADER).read()
    m = re.search(r"#define\s+CM_CLUSTER_NONE\s+(0x[0-9a-fA-F]+)u\b", text)
    assert m and int(m.group(1), 0) == capi.CLUSTER_NONE == cr.NONE == 0xFFFFFFFF
    for name in ("cm_result_clusters", "cm_result_clusters_device"):
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.ClusterParams(0.5, 1, 100, 0)
    lab = np.zeros(4, np.uint32)
    nc, nm = C.c_uint64(), C.c_uint64()
    assert L.cm_result_clusters(None, C.byref(p), lab.ctypes.data, 4, None, 0, None, 0, C.byref(nc), C.byref(nm)) == capi.BAD_ARG
    assert L.cm_result_clusters(None, None, None, 0, None, 0, None, 0, None, None) == capi.BAD_ARG
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.cm_result_clusters_device(None, C.byref(p), C.byref(a), C.byref(b), C.byref(c), C.byref(nc), C.byref(nm)) == capi.BAD_ARG


# ---- CPU: known answers of the restatement ------------------------------------------------------------------------------------
def both(xyz, tol, lo=1, hi=NONE, counts=None):
    a = cr.clusters_brute(xyz, tol, lo, hi, counts)
    b = cr.clusters_tree(xyz, tol, lo, hi, counts)
    assert cr.same(a, b)
    return a


def line(n, step, y=0.0):
    return np.stack([np.arange(n, dtype=F32) * F32(step), np.full(n, y, F32), np.zeros(n, F32)], axis=1)


def test_chain_spaced_exactly_tol_is_singletons_and_one_cluster_just_above():
    xyz = line(8, 0.5)                                         # multiples of 0.5: every difference exact
    labels, table, indices = both(xyz, 0.5)
    assert np.array_equal(labels, np.arange(8)) and np.array_equal(table["n_voxels"], np.ones(8)) and len(indices) == 8
    labels, table, indices = both(xyz, np.nextafter(F32(0.5), F32(1)))
    assert not labels.any() and len(table) == 1 and table["n_voxels"][0] == 8 and np.array_equal(indices, np.arange(8))
    assert np.array_equal(table["min"][0], [0, 0, 0]) and np.array_equal(table["max"][0], [3.5, 0, 0])
    labels, _, _ = both(xyz, np.nextafter(F32(0.5), F32(0)))
    assert np.array_equal(labels, np.arange(8))


def test_two_blobs_joined_by_a_one_voxel_bridge():
    rng = np.random.default_rng(1)
    a = rng.uniform(0.0, 1.0, (40, 3)).astype(F32)
    b = a + F32([1.9, 0, 0])
    tol = 0.5
    assert cr.n_components(np.concatenate([a, b]), tol) == 2
    bridge = F32([[1.45, 0.5, 0.5]])
    xyz = np.concatenate([a, b, bridge])
    # the bridge voxel is within tol of both blobs? make it so: pull the nearest point of each blob next to it
    xyz[0] = [1.1, 0.5, 0.5]
    xyz[40] = [1.8, 0.5, 0.5]
    labels, table, _ = both(xyz, tol)
    assert len(table) == 1 and table["n_voxels"][0] == 81 and not labels.any()
    labels, table, _ = both(xyz[:-1], tol)
    assert len(table) == 2 and sorted(table["n_voxels"]) == [40, 40]


def test_component_above_max_size_vanishes_whole_and_numbers_close_the_gap():
    xyz = np.concatenate([line(3, 0.4, 0.0), line(5, 0.4, 10.0), line(2, 0.4, 20.0), line(4, 0.4, 30.0)])
    counts = np.arange(1, 15, dtype=np.uint32)
    labels, table, indices = both(xyz, 0.5, 1, 4, counts)
    assert np.array_equal(labels, [0, 0, 0] + [NONE] * 5 + [1, 1] + [2] * 4)
    assert np.array_equal(table["n_voxels"], [3, 2, 4]) and np.array_equal(table["first"], [0, 3, 5])
    assert np.array_equal(indices, [0, 1, 2, 8, 9, 10, 11, 12, 13])
    assert np.array_equal(table["n_points"], [1 + 2 + 3, 9 + 10, 11 + 12 + 13 + 14])
    assert np.array_equal(table["min"][1], [0, 20, 0]) and np.array_equal(table["max"][1], F32([0.4, 20, 0]))
    labels, table, _ = both(xyz, 0.5, 3, 4)                     # both ends of the filter
    assert np.array_equal(labels, [0, 0, 0] + [NONE] * 7 + [1] * 4) and not table["n_points"].any()


def test_duplicate_centroids():
    xyz = F32([[1, 2, 3], [1, 2, 3], [5, 5, 5], [1, 2, 3], [5, 5, 5], [9, 9, 9]])
    labels, table, indices = both(xyz, 1e-3)
    assert np.array_equal(labels, [0, 0, 1, 0, 1, 2]) and np.array_equal(table["n_voxels"], [3, 2, 1])
    assert np.array_equal(indices, [0, 1, 3, 2, 4, 5])
    assert np.array_equal(table["min"], table["max"])


def test_numbering_by_smallest_member_not_by_size():
    xyz = np.concatenate([line(1, 0.4, 0.0), line(6, 0.4, 10.0), line(2, 0.4, 0.0)[1:], line(3, 0.4, 20.0)])
    labels, table, indices = both(xyz, 0.5)                     # index 7 joins index 0: cluster 0 has 2, cluster 1 has 6
    assert np.array_equal(labels, [0] + [1] * 6 + [0] + [2] * 3)
    assert np.array_equal(table["n_voxels"], [2, 6, 3]) and np.array_equal(indices, [0, 7, 1, 2, 3, 4, 5, 6, 8, 9, 10])


def test_signed_zero_box():
    xyz = F32([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0]])
    _, table, _ = both(xyz, 1.0)
    assert np.signbit(table["min"][0]).tolist() == [True, True, False] and not np.signbit(table["max"][0]).any()


def adversarial_cloud(seed, n=1500):
    """Random points, points on a lattice of spacing exactly tol (1.0), duplicates, and pairs a float either side of tol."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-6, 6, (n, 3)), rng.integers(-6, 7, (n // 3, 3)).astype(np.float64)]
    base = rng.uniform(-6, 6, (60, 3)).astype(F32)
    for k, d in enumerate((np.nextafter(F32(1), F32(0)), F32(1), np.nextafter(F32(1), F32(2)))):
        parts.append(base[20 * k:20 * k + 20].astype(np.float64) + [float(d), 0, 0])
    xyz = np.concatenate(parts + [base]).astype(F32)
    return np.concatenate([xyz, xyz[:50]])[rng.permutation(len(xyz) + 50)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_two_restatements_agree(seed):
    rng = np.random.default_rng(100 + seed)
    for xyz, tol in ((rng.uniform(-5, 5, (2000, 3)).astype(F32), 0.45), (adversarial_cloud(seed), 1.0),
                     (rng.normal(0, 1, (1500, 3)).astype(F32) * F32(1e4), 1500.0)):
        counts = rng.integers(1, 50, len(xyz)).astype(np.uint32)
        full = both(xyz, tol, 1, NONE, counts)
        assert len(full[1]) >= 2 and (full[1]["n_voxels"] > 1).any() and (full[1]["n_voxels"] == 1).any()
        cut = both(xyz, tol, 2, int(full[1]["n_voxels"].max()) - 1, counts)
        assert (cut[0] == NONE).any() and len(cut[1]) >= 1 and len(cut[1]) < len(full[1])


# ---- CPU: the search grid (cluster_grid, cm_route.cpp) ------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "cm_route.hpp"
static float bits(const std::string& s) { uint32_t u = static_cast<uint32_t>(std::strtoul(s.c_str(), nullptr, 16)); float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t ubits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {           // tol mn0 mn1 mn2 mx0 mx1 mx2 (fp32 bit patterns, hex) row_cap
        std::istringstream in(line);
        std::string t[7]; uint32_t cap;
        for (auto& s : t) in >> s;
        in >> cap;
        float mn[3], mx[3];
        for (int a = 0; a < 3; ++a) { mn[a] = bits(t[1 + a]); mx[a] = bits(t[4 + a]); }
        const ClusterGrid g = cluster_grid(bits(t[0]), mn, mx, cap);
        std::printf("%08x %08x %u %u %u %u %u %u\n", ubits(g.cell), ubits(g.inv), g.dims[0], g.dims[1], g.dims[2], g.key_bits,
                    g.doublings, CM_CLUSTER_AXIS_CAP);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def grid_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("cluster_grid")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    os.path.join(CSRC, "cm_route.cpp"), str(d / "driver.cpp"), "-o", str(exe)], check=True)

    def run(tol, mn, mx, cap=1 << 22):
        h = lambda v: "%08x" % int(np.array(v, F32).view(np.uint32))
        line = " ".join([h(tol)] + [h(v) for v in mn] + [h(v) for v in mx] + [str(cap)])
        out = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()
        cell, inv = (np.array(int(v, 16), np.uint32).view(F32) for v in out[:2])
        return dict(cell=cell, inv=inv, dims=[int(v) for v in out[2:5]], key_bits=int(out[5]), doublings=int(out[6]), axis_cap=int(out[7]))
    return run


def grid_restated(tol, mn, mx, cap, axis_cap):
    """cluster_grid in numpy fp32: the first cell of tol (1 + 2^-8), doubled, whose grid fits."""
    ext = F32(mx) - F32(mn)
    cell = F32(tol) * F32(1.00390625)
    k = 0
    with np.errstate(over="ignore", invalid="ignore"):
        while np.isfinite(ext).all() and np.isfinite(cell):
            inv = F32(1) / cell
            v = ext * inv
            if (v < F32(axis_cap)).all():
                d = [int(np.floor(x)) + 1 for x in v]
                if d[1] * d[2] <= cap and d[0] * d[1] * d[2] <= 0xFFFFFFFF:
                    return cell, inv, d, k
            cell = F32(cell * F32(2))
            k += 1
    return F32(np.inf), F32(0), [1, 1, 1], None


def test_grid_cell_is_never_below_the_tolerance(grid_driver):
    rng = np.random.default_rng(7)
    for _ in range(40):
        tol = F32(10.0 ** rng.uniform(-3, 2))
        mn = rng.uniform(-100, 0, 3).astype(F32)
        mx = (mn + rng.uniform(0, 300, 3)).astype(F32)
        g = grid_driver(tol, mn, mx)
        cell, inv, dims, k = grid_restated(tol, mn, mx, 1 << 22, g["axis_cap"])
        assert g["cell"] >= tol and g["cell"] == cell and g["inv"] == inv and g["dims"] == dims and g["doublings"] == k
        assert max(dims) <= g["axis_cap"] and dims[1] * dims[2] <= 1 << 22 and dims[0] * dims[1] * dims[2] < 2 ** 32
        assert (1 << g["key_bits"]) >= dims[0] * dims[1] * dims[2]


def test_grid_doubles_for_the_axis_cap_the_row_table_and_the_key_width(grid_driver):
    z = [0, 0, 0]
    g = grid_driver(1.0, z, [100, 100, 10])                    # fits as it is
    assert g["doublings"] == 0 and g["cell"] == F32(1.00390625) and g["dims"] == [100, 100, 10]
    cap = g["axis_cap"]
    g = grid_driver(1.0, z, [8000, 10, 10])                     # 7969 cells along x: one doubling
    assert cap == 4096 and g["doublings"] == 1 and g["cell"] == F32(2.0078125) and g["dims"][0] == 3985
    g = grid_driver(1.0, z, [10, 3000, 3000])                   # 2989 x 2989 rows > 2^22: doubled to 1495 x 1495
    assert g["doublings"] == 1 and g["dims"][1] * g["dims"][2] <= 1 << 22 and g["dims"][1] == 1495
    g = grid_driver(1.0, z, [10, 3000, 3000], cap=1 << 20)      # a smaller table: doubled twice
    assert g["doublings"] == 2 and g["dims"][1] == 748
    g = grid_driver(1.0, z, [4000, 2000, 2000])                 # rows fit (1993^2 < 2^22), 3985 x 1993 x 1993 needs 34 bits
    assert g["doublings"] == 1 and g["dims"][0] * g["dims"][1] * g["dims"][2] < 2 ** 32 and g["key_bits"] <= 32
    g = grid_driver(1e-20, z, [1, 1, 1])                        # a tolerance far below the extent: many doublings, still finite
    assert g["doublings"] > 50 and np.isfinite(g["cell"]) and max(g["dims"]) <= cap
    g = grid_driver(0.5, [3, 3, 3], [3, 3, 3])                  # one centroid
    assert g["dims"] == [1, 1, 1] and g["doublings"] == 0


def test_grid_of_an_extent_that_overflows_fp32_is_one_cell(grid_driver):
    for mn, mx in (([-3e38, 0, 0], [3e38, 1, 1]), ([0, 0, -2e38], [1, 1, 2e38])):
        g = grid_driver(0.5, mn, mx)
        assert np.isinf(g["cell"]) and g["inv"] == 0 and g["dims"] == [1, 1, 1] and g["key_bits"] == 1
    g = grid_driver(0.5, [-1e38, 0, 0], [1e38, 1, 1])           # 2e38 is finite: a (huge) finite cell fits
    assert np.isfinite(g["cell"]) and g["cell"] >= 0.5 and max(g["dims"]) <= g["axis_cap"]


def test_joined_centroids_are_never_two_cells_apart(grid_driver):
    """The stencil's premise, in the kernel's own arithmetic (cell = floor((p - min) * inv), fp32): pairs the fp32 predicate
    joins — drawn at distances a hair below the tolerance, along the axes and across cell faces — differ by at most one
    cell on every axis, at the largest grids cluster_grid allows."""
    rng = np.random.default_rng(11)
    for tol, span in ((0.05, 200.0), (1.0, 4000.0), (0.37, 1500.0), (1e-3, 4.0)):
        mn = F32([-span / 3, -span / 2, -1.0])
        mx = (mn + F32([span, span * 0.2, 3.0])).astype(F32)
        g = grid_driver(tol, mn, mx)
        n = 200_000
        a = (mn + rng.uniform(0, 1, (n, 3)) * (mx - mn)).astype(F32)
        a[: n // 2, 0] = (mn[0] + np.floor((a[: n // 2, 0] - mn[0]) / g["cell"]) * g["cell"]).astype(F32)   # on x faces
        u = rng.normal(size=(n, 3)); u[: n // 4] = [1, 0, 0]; u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = F32(tol) * (1 - 10.0 ** rng.uniform(-8, -1, (n, 1)))
        b = np.clip((a.astype(np.float64) + u * r), mn, mx).astype(F32)
        ok = cr.near(a, b, cr.tol2_of(tol))
        assert ok.sum() > n // 4
        cell = lambda p: np.clip(np.floor((p - mn) * g["inv"]), 0, np.array(g["dims"], F32) - 1)
        assert (np.abs(cell(a[ok]) - cell(b[ok])) <= 1).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def hip_rt():
    try:
        return C.CDLL("libamdhip64.so.7")
    except OSError:
        return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def expected(cm, res, tol, lo=1, hi=NONE, trivial=None):
    """The restatement on the frame's own result, and the conditions that keep the comparison from being vacuous."""
    rec = cm.result(res.n_out)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    counts = cm.cells(res.n_out)[1] if cm.flags & capi.FLAG_OCCUPANCY else None
    want = cr.clusters_tree(xyz, tol, lo, hi, counts)
    labels, table, _ = want
    n = res.n_out
    one = len(table) == 1 and table["n_voxels"][0] == n
    singles = len(table) == n
    print(f"n_out {n} tol {tol} [{lo}, {hi}]: clusters {len(table)} clustered {int(table['n_voxels'].sum())} "
          f"largest {int(table['n_voxels'].max()) if len(table) else 0} dropped voxels {int((labels == NONE).sum())}")
    if trivial is None:
        assert len(table) >= 2 and not one and not singles
        assert not np.array_equal(labels, np.zeros(n, np.uint32)) and not np.array_equal(labels, np.arange(n, dtype=np.uint32))
        if lo > 1 or hi < NONE:
            assert (labels == NONE).any()
    elif trivial == "one":
        assert one
    elif trivial == "singles":
        assert singles
    elif trivial == "none":
        assert len(table) == 0 and (labels == NONE).all()
    if counts is not None and len(table):
        assert table["n_points"].astype(np.uint64).sum() == counts[labels != NONE].astype(np.uint64).sum() > 0
    else:
        assert not table["n_points"].any()
    return want


def check(cm, res, tol, lo=1, hi=NONE, trivial=None):
    assert res.status == capi.OK
    want = expected(cm, res, tol, lo, hi, trivial)
    got = cm.clusters(tol, lo, hi)
    for name, g, w in zip(("labels", "clusters", "indices"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{name}: {len(bad)} entries differ, first at {bad[:5]}: got {g[bad[:5]]} want {w[bad[:5]]}")
    # the device entry point: the same bytes
    lp, cp, ip, nc, nm = cm.clusters_device(tol, lo, hi)
    assert nc == len(want[1]) and nm == len(want[2])
    hip = hip_rt()
    for ptr, w in zip((lp, cp, ip), want):
        assert bool(ptr) == (len(w) > 0)
        if len(w):
            d = np.zeros_like(w)
            assert hip.hipMemcpy(C.c_void_p(d.ctypes.data), C.c_void_p(ptr), C.c_size_t(w.nbytes), 2) == 0
            assert d.tobytes() == w.tobytes()
    return want


def objects(seed=3, centre=(60.0, 60.0, 0.0)):
    """Forty blobs of 30 .. 3000 points on a 5 x 8 lattice of 4 m, far from the cfg2 scene: clusters of many sizes."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(40):
        c = np.array(centre) + [4.0 * (k % 5), 4.0 * (k // 5), 0.0]
        m = int(30 * 100 ** (k / 39))
        out.append(c + rng.normal(0, 0.25 + 0.01 * k, (m, 3)))
    return np.concatenate(out).astype(F32)


def frame_sensors(n_per=150_000, extra=True):
    sensors, _ = synth.config2(n_per_sensor=n_per, min_pts=0)
    if extra:
        xyz = objects()
        sensors.append(xyzi_cloud(xyz, np.ones(len(xyz), F32)))
    return sensors, sum(s.n for s in sensors)


def run_frame(cm, sensors, params):
    cm.submit_all(sensors)
    return cm.merge_voxelize(params)


COARSE = dict(leaf=(0.5,) * 3, min_points_per_voxel=0)
CROP = dict(crop_min=(-40.0, -40.0, -10.0), crop_max=(90.0, 100.0, 10.0))
OCC = pytest.mark.parametrize("flags", [0, capi.FLAG_OCCUPANCY], ids=["plain", "occupancy"])


@pytest.mark.gpu
@OCC
def test_general_route(monkeypatch, flags):
    monkeypatch.setenv("CM_PATH", "classic")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=flags) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert not res.path_flags & capi.PATH_BUCKET
        check(cm, res, 0.5)
        check(cm, res, 0.75, 3, 500)


@pytest.mark.gpu
@OCC
def test_fixed_grid_route(monkeypatch, flags):
    monkeypatch.setenv("CM_QUANT", "0")
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=flags) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        check(cm, res, 0.5)
        check(cm, res, 0.75, 3, 500)


@pytest.mark.gpu
@OCC
def test_quantile_and_predicted_box_routes(flags):
    """cfg2's moving stream at 5 cm: with a crop box the frames after the first take the quantile pass; without one they
    run in the box predicted from their predecessors."""
    n_per = 150_000
    for crop, want in ((dict(crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3), capi.PATH_QUANTILE), ({}, capi.PATH_PREDICTED)):
        seen = []
        with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=flags) as cm:
            for k in range(3):
                sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
                params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, **crop)
                res = run_frame(cm, sensors, params)
                check(cm, res, 0.1, 2, 2000)
                seen.append(res.path_flags)
        assert all(f & capi.PATH_BUCKET for f in seen), seen
        assert any(f & want for f in seen[1:]), seen


@pytest.mark.gpu
@OCC
def test_predicted_box_route_coarse(flags):
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=flags) as cm:
        for k in range(2):
            res = run_frame(cm, sensors, MergeParams(**COARSE))
            check(cm, res, 0.5, 2, 1000)
        assert res.path_flags & capi.PATH_PREDICTED


@pytest.mark.gpu
@OCC
def test_one_metre_leaf_stays_on_the_fixed_grid(flags):
    sensors, n_cap = frame_sensors(n_per=600_000)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=flags) as cm:
        res = run_frame(cm, sensors, MergeParams(leaf=(1.0,) * 3, min_points_per_voxel=0, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        check(cm, res, 0.95, 2, 5000)


# ---- GPU: behind each pre-stage -----------------------------------------------------------------------------------------
FRONT_SLABS = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]


def street(n_ground=400_000, seed=9):
    """A flat noisy ground with sixty obstacles standing on it (boxes of points, 0.3 .. 2 m) and loose points above it, one sensor at the identity:
    what the realistic chain — crop, ground removal, voxel grid, clusters — is for."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-14, 28, n_ground), rng.uniform(-28, 28, n_ground), rng.normal(-1.5, 0.02, n_ground)], axis=1)
    obs = [np.stack([rng.uniform(-14, 28, 300), rng.uniform(-28, 28, 300), rng.uniform(0.5, 3.0, 300)], axis=1)]   # loose points
    for k in range(60):
        c = np.array([rng.uniform(-13, 26), rng.uniform(-26, 26)])
        s = rng.uniform(0.3, 2.0, 3)
        m = int(400 * s.prod() ** 0.66) + 40
        obs.append(np.stack([c[0] + rng.uniform(0, s[0], m), c[1] + rng.uniform(0, s[1], m), -1.2 + rng.uniform(0, s[2], m)], axis=1))
    xyz = np.concatenate([g] + obs).astype(F32)
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.gpu
def test_behind_ground_removal():
    xyz = street()
    cloud = xyzi_cloud(xyz, np.ones(len(xyz), F32))
    gp = capi.make_ground_params([FRONT_SLABS])
    with capi.CloudMerger(max_points_total=cloud.n, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(gp)
        cm.submit(0, cloud)
        res = cm.merge_voxelize(MergeParams(leaf=(0.2,) * 3, min_points_per_voxel=1, crop_min=(-30.0, -30.0, -10.0),
                                            crop_max=(30.0, 30.0, 10.0)))
        assert len(cm.ground(cloud.n)) > 100_000
        check(cm, res, 0.4, 5, 20000)


@pytest.mark.gpu
def test_behind_the_radius_outlier_stage():
    sensors, n_cap = frame_sensors()
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, outlier_radius=0.15, outlier_min_neighbors=2, **CROP)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, params)
        assert len(cm.merged(n_cap)) < n_cap
        check(cm, res, 0.5, 2, 1000)


@pytest.mark.gpu
def test_behind_statistical_outlier_removal():
    sensors, n_cap = frame_sensors(n_per=60_000)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_statistical_outlier(8, 0.5)
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_SOR and cm.sor_stats().n_removed > 0
        check(cm, res, 0.5, 2, 1000)


@pytest.mark.gpu
def test_behind_deskew():
    sensors, n_cap = frame_sensors()
    t_ref = 1_700_000_000_000_000_000
    m = capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000 * (s + 1) for s in range(5)])
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5) as cm:
        cm.set_ego_motion(m)
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        assert res.path_flags & capi.PATH_MOTION
        check(cm, res, 0.5, 2, 1000)


# ---- GPU: tolerance against leaf ----------------------------------------------------------------------------------------
def scattered(seed=21):
    """Blobs, a sparse haze and a few lines in a 60 m box: at leaf 0.2 the tolerance sweeps from below the voxel spacing
    (singletons dominate) to far above it (a few large clusters)."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-30, 30, (3000, 3)) * [1, 1, 0.1]]
    for k in range(30):
        parts.append(rng.uniform(-28, 28, 3) * [1, 1, 0.1] + rng.normal(0, 0.1 + 0.05 * (k % 7), (200 + 40 * k, 3)))
    for k in range(6):
        t = np.linspace(0, 1, 400)[:, None]
        parts.append(rng.uniform(-28, 28, 3) * [1, 1, 0.1] * (1 - t) + rng.uniform(-28, 28, 3) * [1, 1, 0.1] * t)
    return np.concatenate(parts).astype(F32)


@pytest.mark.gpu
def test_tolerance_against_leaf():
    xyz = scattered()
    cloud = xyzi_cloud(xyz, np.ones(len(xyz), F32))
    leaf = 0.2
    with capi.CloudMerger(max_points_total=cloud.n, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.submit(0, cloud)
        res = cm.merge_voxelize(MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=0))
        for mult in (0.5, 1.0, 1.5, 3.0, 10.0):
            check(cm, res, leaf * mult)
            check(cm, res, leaf * mult, 2, 400)
        check(cm, res, 500.0, trivial="one")                      # larger than the whole cloud
        check(cm, res, 500.0, 1, res.n_out - 1, trivial="none")
        check(cm, res, 1e-4, trivial="singles")                   # smaller than any gap between two centroids
        check(cm, res, 1e-4, 2, NONE, trivial="none")             # ... zero clusters, CM_OK


# ---- GPU: adversarial geometry, every input point its own voxel ----------------------------------------------------------
def submit_as_voxels(cm, xyz, leaf, min_pts):
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


@pytest.mark.gpu
@pytest.mark.parametrize("min_pts", [0, 1])
def test_centroids_on_search_cell_faces(min_pts):
    """tolerance 1: the search cell is 1.00390625 and the grid starts at the cloud's minimum (0, 0, 0). Points on the faces
    k * cell, a quarter below them, and partners a hair inside the tolerance on the far side."""
    cell = F32(1.00390625)
    k = np.arange(0, 40, dtype=F32)
    face = np.stack(np.meshgrid(k[:20] * cell, k[:10] * cell, k[:4] * cell, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    face = face[rng.random(len(face)) < 0.35]
    below = face[::3] - F32([0.25, 0, 0])
    below = below[below[:, 0] > 0]
    far = face[1::3] + F32([np.nextafter(F32(1), F32(0)) - F32(0.375), 0.375, 0])
    diag = face[2::3] + F32([0.5, 0.5, 0.5])
    xyz = np.concatenate([F32([[0, 0, 0]]), face[1:], below, far, diag]).astype(F32)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res = submit_as_voxels(cm, xyz, 0.0625, min_pts)
        check(cm, res, 1.0)
        check(cm, res, 1.0, 2, 50)


@pytest.mark.gpu
def test_pairs_at_the_tolerance_and_the_floats_next_to_it():
    tol = F32(1.0)
    rows = []
    for j, base in enumerate((0.0, 0.5, 16.0, 1024.0, 511.99997, -256.0, 3.0000002)):
        for i, d in enumerate((np.nextafter(tol, F32(0)), tol, np.nextafter(tol, F32(2)))):
            a = F32([base, 4.0 * (3 * j + i), 0.0])
            for axis in range(3):
                b = a.copy(); b[axis] = F32(a[axis] + d)
                o = F32([0, 0, 4.0 * axis])
                rows += [a + o, b + o]
    xyz = np.unique(np.array(rows, F32), axis=0)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1) as cm:
        res = submit_as_voxels(cm, xyz, 0.25, 1)
        want = check(cm, res, float(tol))
        assert (want[1]["n_voxels"] == 2).sum() >= 3 and (want[1]["n_voxels"] == 1).sum() >= 20


def snake(n=24_000, step=0.875, row=150, pitch=3.0):
    """A one-voxel-wide serpentine: n points `step` apart, rows of `row` points `pitch` apart joined at alternating ends by
    vertical runs — one component whose smallest-index member is far, along the path, from most of its members."""
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
def test_a_snake_of_24000_voxels_is_one_cluster():
    xyz = snake()
    decoys = np.concatenate([snake(600, row=40) + F32([0, -200.0, 0]), snake(300, row=25) + F32([0, -300.0, 0])])   # separate ones
    loose = np.stack([np.arange(25) * 5.0, np.full(25, -100.0), np.zeros(25)], axis=1).astype(F32)
    loose = np.concatenate([loose, loose + F32([0.5, 0, 0])])    # 25 pairs half a metre apart
    allp = np.concatenate([xyz, decoys, loose])
    assert cr.n_components(xyz, 1.0) == 1
    with capi.CloudMerger(max_points_total=len(allp), max_sensors=1) as cm:
        res = submit_as_voxels(cm, allp, 0.25, 0)
        want = check(cm, res, 1.0)
        assert sorted(want[1]["n_voxels"])[-3:] == [300, 600, 24_000] and len(want[1]) == 28
        check(cm, res, 1.0, 2, 1000)
        assert len(check(cm, res, 0.875)[1]) == len(allp) - 25    # exactly the spacing: strict <, only the pairs join ...
        assert len(check(cm, res, float(np.nextafter(F32(0.875), F32(1))))[1]) == 28   # ... and everything just above it


@pytest.mark.gpu
def test_one_component_with_most_of_the_voxels_beside_thousands_of_singletons():
    k = np.arange(40, dtype=F32) * F32(0.5)
    block = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)              # 64000, 0.5 apart
    s = np.arange(16, dtype=F32) * F32(3.0)
    singles = np.stack(np.meshgrid(s + 30, s, s[:12], indexing="ij"), axis=-1).reshape(-1, 3)  # 3072, 3 apart
    pairs = singles[:400] + F32([0, 100.0, 0])
    pairs = np.concatenate([pairs, pairs + F32([0.5, 0, 0])])                                  # 400 pairs
    xyz = np.concatenate([singles[:1500], pairs[:300], block, singles[1500:], pairs[300:]]).astype(F32)
    assert len(block) > 0.9 * len(xyz)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res = submit_as_voxels(cm, xyz, 0.25, 1)
        want = check(cm, res, 0.625)
        assert want[1]["n_voxels"].max() == 64_000 and (want[1]["n_voxels"] == 1).sum() == 3072 and len(want[1]) == 3473
        check(cm, res, 0.625, 2, NONE)
        check(cm, res, 0.625, 1, 63_999)


# ---- GPU: full size -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_frame():
    sensors, params = synth.config2(min_pts=0)
    n_cap = sum(s.n for s in sensors)
    tol = 2 * params.leaf[0]
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        res = run_frame(cm, sensors, params)
        assert res.n_out > 1_000_000
        check(cm, res, tol)
        check(cm, res, tol, 10, 100_000)


# ---- GPU: refusals, capacity, non-interference ----------------------------------------------------------------------------
def refused(cm, tol=0.5, lo=1, hi=NONE, code=capi.BAD_ARG):
    for call in (cm.clusters, cm.clusters_device):
        with pytest.raises(capi.CloudMergeError) as e:
            call(tol, lo, hi)
        assert e.value.status == code and cm._lib.cm_last_error(cm._ctx)


@pytest.mark.gpu
def test_refusals():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:
        with pytest.raises(capi.CloudMergeError):                  # no result yet (result_device refuses first)
            cm.clusters(0.5)
        p = capi.ClusterParams(0.5, 1, NONE, 0)
        nc, nm = C.c_uint64(), C.c_uint64()
        assert cm._lib.cm_result_clusters(cm._ctx, C.byref(p), None, 0, None, 0, None, 0, C.byref(nc), C.byref(nm)) == capi.BAD_ARG
        assert cm._lib.cm_last_error(cm._ctx)
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        assert cm._lib.cm_result_clusters(cm._ctx, C.byref(p), None, 0, None, 0, None, 0, C.byref(nc), C.byref(nm)) == capi.BAD_ARG
        assert b"flight" in cm._lib.cm_last_error(cm._ctx)         # frame in flight
        res = cm.wait()
        assert res.status == capi.OK
        for tol in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
            refused(cm, tol)
        refused(cm, 0.5, 0, 10)
        refused(cm, 0.5, 5, 4)
        assert cm._lib.cm_result_clusters(cm._ctx, None, None, 0, None, 0, None, 0, C.byref(nc), C.byref(nm)) == capi.BAD_ARG
        check(cm, res, 0.5)                                        # ... and a valid call afterwards succeeds
        tiny = MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)
        res = run_frame(cm, sensors, tiny)
        assert res.status == capi.GRID_OVERFLOW                    # no voxel grid
        refused(cm)
        for s in range(4):
            cm.clear(s)
        cm.submit(0, xyzi_cloud(np.full((4, 3), np.nan, F32)))
        res = cm.merge_voxelize(params)
        assert res.status == capi.EMPTY_INPUT
        refused(cm)
        cm.submit_all(sensors)
        res = cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40))
        assert res.status == capi.OK
        refused(cm)                                                # a partial table
        ptr, n = cm.partial_device()
        res = cm.merge_tables([ptr], [n], params)
        assert res.status == capi.OK
        refused(cm)                                                # merged tables
        res = run_frame(cm, sensors, params)
        check(cm, res, 0.5)


@pytest.mark.gpu
def test_capacity():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:
        res = run_frame(cm, sensors, MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0))
        want = expected(cm, res, 0.5, 2, 1000)
        n, k, m = res.n_out, len(want[1]), len(want[2])
        p = capi.ClusterParams(0.5, 2, 1000, 0)
        lab, tab, idx = np.zeros(n, np.uint32), np.zeros(k, capi.CLUSTER_DTYPE), np.zeros(m, np.uint32)
        for caps in ((n - 1, k, m), (n, k - 1, m), (n, k, m - 1), (n, k, m), (0, k, 0), (0, 0, 0)):
            nc, nm = C.c_uint64(99), C.c_uint64(99)
            args = [a.ctypes.data if c else None for a, c in zip((lab, tab, idx), caps)]
            st = cm._lib.cm_result_clusters(cm._ctx, C.byref(p), args[0], caps[0], args[1], caps[1], args[2], caps[2],
                                            C.byref(nc), C.byref(nm))
            small = (args[0] and caps[0] < n) or (args[1] and caps[1] < k) or (args[2] and caps[2] < m)
            assert st == (capi.CAPACITY if small else capi.OK), caps
            assert (nc.value, nm.value) == (k, m), caps
            if small:
                assert cm._lib.cm_last_error(cm._ctx)
        assert lab.tobytes() == want[0].tobytes() and tab.tobytes() == want[1].tobytes() and idx.tobytes() == want[2].tobytes()


@pytest.mark.gpu
def test_requests_do_not_change_later_frames():
    """Two identical 12-frame streams on two contexts; one asks for clusters after every frame."""
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
                    labels, table, _ = cm.clusters(0.1, 2, 5000)
                    assert len(table) >= 2 and (labels == NONE).any()
                cells, counts = cm.cells(res.n_out)
                out.append((res.status, res.n_out, res.path_flags, cm.result(res.n_out).tobytes(), cells.tobytes(),
                            counts.tobytes()))
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {k} differs"
    assert any(f[2] & capi.PATH_QUANTILE for f in runs[0])


@pytest.mark.gpu
def test_deterministic_and_stage_names():
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
        res = run_frame(cm, sensors, MergeParams(**COARSE))
        frame_stages = [n for n, _ in cm.stage_times()]
        a = cm.clusters(0.5, 2, 1000)
        names = [n for n, _ in cm.stage_times()]
        assert not any(n.startswith("k_cl_") for n in frame_stages)
        for want in ("k_cl_bounds", "k_cl_keys", "k_cl_hook", "k_cl_roots", "k_cl_labels"):
            assert want in names, names
        b = cm.clusters(0.75, 1, NONE)
        assert not cr.same(a, b)
        assert cr.same(a, cm.clusters(0.5, 2, 1000))
