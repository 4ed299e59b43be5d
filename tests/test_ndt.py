"""NDT registration against the per-voxel covariance table: cm_result_ndt_align / cm_result_ndt_align_device /
cm_ndt_correspondences_copy (include/cloudmerge.h, cm_kernels_ndt.hip, cm_ndt_math.hpp).

The bar: the correspondence table (idx, n_used, the bits of score) EXACTLY equal to the restatement (tests/ndt_ref.py) fed
with the frame's own result, cells and covariance table; H, g and the score equal to the restatement's tree sum by value
(np.array_equal), n_corr equal, all of them within 2 n 2^-53 sum|t| of math.fsum; cm_exp_neg bit for bit the restatement's
and within 4 x 2^-53 relative of math.exp; on §16's corner scene the restatement's iteration count and flags, its pose
within 1e-9 per entry, and an error to the true pose of at most twice what the restatement measured on the CPU."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import ndt_ref as nd
from tests import voxel_cov_ref as vr
from tests.test_align import corner_scene, pose_error, rodrigues
from tests.test_cluster import COARSE, CROP, frame_sensors, hip_rt, run_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")
F32 = np.float32
EYE = np.eye(3, 4)
LEAF = (0.5, 0.5, 0.5)
GUESS = np.concatenate([rodrigues(np.radians([2.0, -1.0, 1.5])), np.array([[0.03], [-0.02], [0.04]])], axis=1)
# exactly representable: a quarter turn about z that maps [0, 3]^3 onto itself, and with it multiples of the leaf onto such
GUESS_Q = np.array([[0.0, -1.0, 0.0, 3.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
# What the restatement measured on the CPU on §16's corner scene through a numpy voxel grid at leaf 0.5, neighbourhood 7,
# eps 1e-6 (test_restatement_converges_on_the_corner asserts them): iterations, and the error to the true pose as
# (distance of the images of the scene's centre, Frobenius norm of the rotations' difference), rounded up; per shift, for at
# 1000 m an fp32 coordinate resolves 6e-5 m and 69 of the 171 voxels fail the table's lambda_0 >= 0.
CPU_ITERATIONS = {0.0: 8, 1000.0: 8}
CPU_ERROR = {0.0: (2.9e-4, 4.9e-5), 1000.0: (5.2e-4, 1.3e-4)}


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_ndt_structs_match_header(tmp_path):
    pf = ("outlier_ratio", "neighborhood", "max_iterations", "min_correspondences", "cov", "trans_eps", "rot_eps", "guess")
    rf = ("pose", "H", "g", "score", "gauss_d1", "gauss_d2", "pivot", "n_corr", "iterations", "flags")
    cf = ("idx", "n_used", "score")
    items = ["sizeof(cm_ndt_params)"] + [f"offsetof(cm_ndt_params,{f})" for f in pf] + ["sizeof(cm_ndt_result)"] + \
            [f"offsetof(cm_ndt_result,{f})" for f in rf] + ["sizeof(cm_ndt_corr)"] + [f"offsetof(cm_ndt_corr,{f})" for f in cf] + \
            ["(size_t)CM_NDT_MAX_ITER", "(size_t)CM_NDT_NONE", "(size_t)CM_NDT_CONVERGED", "(size_t)CM_NDT_MAX_ITER_HIT",
             "(size_t)CM_NDT_FEW", "(size_t)CM_NDT_SINGULAR"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, R, d = capi.NdtParams, capi.NdtResult, capi.NDT_CORR_DTYPE
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in pf] + [C.sizeof(R)] + [getattr(R, f).offset for f in rf] + \
           [d.itemsize] + [d.fields[f][1] for f in cf] + \
           [capi.NDT_MAX_ITER, capi.NDT_NONE, capi.NDT_CONVERGED, capi.NDT_MAX_ITER_HIT, capi.NDT_FEW, capi.NDT_SINGULAR]
    assert got == want
    # no padding anywhere: 4 x 4 + 8 bytes before the doubles, then 16 + 96
    assert got[0] == 16 + 8 + 16 + 96 == 136 and got[1:9] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert got[9] == 376 and got[20] == 16 and got[21:24] == [0, 4, 8] and got[24] == 64
    assert d == nd.CORR_DTYPE and (nd.NONE, nd.MAX_ITER) == (capi.NDT_NONE, capi.NDT_MAX_ITER)
    assert (nd.CONVERGED, nd.MAX_ITER_HIT, nd.FEW, nd.SINGULAR) == (1, 2, 4, 8) == \
           (capi.ALIGN_CONVERGED, capi.ALIGN_MAX_ITER_HIT, capi.ALIGN_FEW, capi.ALIGN_SINGULAR)


def test_symbols_are_declared():
    text = open(HEADER).read()
    for name in ("cm_result_ndt_align", "cm_result_ndt_align_device", "cm_ndt_correspondences_copy"):
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.ndt_params()
    out = capi.NdtResult()
    src = np.zeros((4, 4), F32)
    assert L.cm_result_ndt_align(None, C.byref(p), src.ctypes.data, 4, C.byref(out)) == capi.BAD_ARG
    assert L.cm_result_ndt_align_device(None, C.byref(p), None, 0, C.byref(out)) == capi.BAD_ARG
    n = C.c_uint64()
    assert L.cm_ndt_correspondences_copy(None, None, 0, C.byref(n)) == capi.BAD_ARG


# ---- CPU: cm_ndt_math.hpp -------------------------------------------------------------------------------------------------
EXP_DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "cm_ndt_math.hpp"
int main() {
    unsigned long long u;
    while (std::scanf("%llx", &u) == 1) {
        double x, y;
        std::memcpy(&x, &u, 8);
        y = cm_exp_neg(x);
        std::memcpy(&u, &y, 8);
        std::printf("%016llx\n", u);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exp_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("ndt_math")
    (d / "driver.cpp").write_text(EXP_DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, str(d / "driver.cpp"),
                    "-o", str(exe)], check=True)

    def run(x):
        x = np.ascontiguousarray(x, np.float64)
        text = "\n".join("%016x" % int(v) for v in x.view(np.uint64))
        out = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True).stdout.split()
        return np.array([int(v, 16) for v in out], np.uint64).view(np.float64)
    return run


def exp_arguments():
    rng = np.random.default_rng(5)
    below = np.nextafter(700.0, 0.0)
    # t * log2(e) at exact half-integers (as nearly as an argument can put it there): x = (k + 0.5) ln 2 and its neighbours
    half = (np.arange(0, 1009) + 0.5) * math.log(2.0)
    half = np.concatenate([half, np.nextafter(half, 0.0), np.nextafter(half, 1e9)])
    exact_half = np.array([(k + 0.5) / nd.LOG2E for k in range(0, 1009)])
    x = np.concatenate([[0.0, below, 700.0, np.nextafter(700.0, 1e9), np.nan, 1e300, np.inf, 5e-324, 1e-300, 1e-17, 2.0 ** -53],
                        half, exact_half, rng.uniform(0, 700, 60_000), rng.uniform(0, 40, 30_000), 10.0 ** rng.uniform(-12, 2.8, 8_000)])
    return x


def test_exp_neg_driver_is_the_restatement_bit_for_bit(exp_driver):
    x = exp_arguments()
    assert 95_000 <= len(x) <= 110_000
    got, want = exp_driver(x), nd.exp_neg(x)
    assert got.tobytes() == want.tobytes()
    assert got[0] == 1.0 and got[1] > 0 and got[2] == 0 and got[3] == 0 and got[4] == 0 and not np.signbit(got[2:7]).any()
    assert got[1] == math.exp(-x[1]) or abs(got[1] / math.exp(-x[1]) - 1) < 4 * 2.0 ** -53
    # the half-integer arguments took both roundings of k
    t = -x[11:11 + 3 * 1009]
    k = np.rint(t * nd.LOG2E)
    assert (k == np.floor(t * nd.LOG2E)).any() and (k == np.ceil(t * nd.LOG2E)).any()


def test_exp_neg_against_libm(exp_driver):
    """Within 4 x 2^-53 relative of math.exp: thirteen Horner steps with |rr| <= 0.3466, each adding at most about
    2^-53 (|rr| + |rr|^2 + ...) < 0.53 x 2^-53 on top of the last step's own half ulp, the reduction's error of below one
    ulp of rr in the exponent, and libm's own half ulp and a bit."""
    x = exp_arguments()
    x = x[np.isfinite(x) & (x < 700)]
    got = exp_driver(x)
    want = np.array([math.exp(-v) for v in x.tolist()])
    rel = np.abs(got - want) / want
    print(f"cm_exp_neg against math.exp over {len(x)} arguments: max relative error {rel.max() / 2.0 ** -53:.3f} x 2^-53")
    assert rel.max() <= 4 * 2.0 ** -53


def test_constants():
    d1, d2 = nd.gauss(LEAF, 0.55)
    # PCL's values at resolution 0.5 and outlier ratio 0.55, from its formulas in plain Python floats
    c1, c2 = 10 * (1 - float(F32(0.55))), float(F32(0.55)) / 0.125
    d3 = -math.log(c2)
    assert d1 == -math.log(c1 + c2) - d3 and d1 < 0 < d2
    assert d2 == -2 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def numpy_voxel_grid(pts, leaf, min_pts=1):
    """(centroids fp32, cells, counts, min_b, div_b, voxel number per point) of pcl::VoxelGrid in numpy: what a frame of one
    sensor leaves, up to the centroid's last bits (the CPU tests need a grid, not the device's)."""
    pts = np.ascontiguousarray(pts, F32)
    inv = F32(1.0) / np.asarray(leaf, F32)
    pc = np.floor(pts * inv[None, :]).astype(np.int64)
    min_b = pc.min(axis=0)
    div_b = pc.max(axis=0) - min_b + 1
    rel = pc - min_b
    key = rel[:, 0] + rel[:, 1] * div_b[0] + rel[:, 2] * div_b[0] * div_b[1]
    uk, vox, cnt = np.unique(key, return_inverse=True, return_counts=True)
    keep = cnt >= min_pts
    renum = np.cumsum(keep) - 1
    vox = np.where(keep[vox], renum[vox], -1)
    uk, cnt = uk[keep], cnt[keep]
    cells = np.stack([uk % div_b[0], (uk // div_b[0]) % div_b[1], uk // (div_b[0] * div_b[1])], axis=1) + min_b
    cen = np.zeros((len(uk), 3))
    np.add.at(cen, vox[vox >= 0], pts[vox >= 0].astype(np.float64))
    return (cen / cnt[:, None]).astype(F32), cells, cnt, min_b, div_b, vox


def cpu_corner(shift):
    tgt, src, truth = corner_scene(60_000, 5_000, shift)
    cen, cells, cnt, min_b, div_b, vox = numpy_voxel_grid(tgt.astype(F32), LEAF)
    table, _ = vr.voxel_stats(tgt.astype(F32), vox, len(cells), 6, 0.01)      # tests/voxel_cov_ref.py's table
    return cen, cells, table, min_b, div_b, src, truth


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["origin", "1000m"])
def test_restatement_converges_on_the_corner(shift):
    """§16's corner scene, 180 k target and 15 k source points, through a numpy voxel grid at leaf 0.5; the table is
    tests/voxel_cov_ref.py's. What it measures is the yardstick of the device test: CPU_ITERATIONS and CPU_ERROR."""
    cen, cells, table, min_b, div_b, src, truth = cpu_corner(shift)
    _, d2 = nd.gauss(LEAF, 0.55)
    e = nd.align(src, cen, cells, table, d2, LEAF, min_b, div_b)
    c = np.full(3, 2.0 + shift)
    dp, dr = pose_error(e["pose"], truth, c)
    H = np.zeros((6, 6))
    H[np.tril_indices(6)] = e["H"]
    ev = np.linalg.eigvalsh(H + np.tril(H, -1).T)
    print(f"shift {shift}: voxels {len(cells)} valid {int((table['flags'] & 1).sum())} iterations {e['iterations']} flags {e['flags']} "
          f"n_corr {e['n_corr']} score {e['score']:.6g} error at the centre {dp:.6g} in R {dr:.6g} eig ratio {ev[0] / ev[-1]:.3g}")
    assert len(src) == 15_000 and e["flags"] == nd.CONVERGED and e["n_corr"] > 14_000
    assert e["iterations"] == CPU_ITERATIONS[shift]
    assert dp <= CPU_ERROR[shift][0] and dr <= CPU_ERROR[shift][1] and ev[0] > 0
    if shift == 0.0:
        one = nd.align(src, cen, cells, table, d2, LEAF, min_b, div_b, neighborhood=1, max_iterations=64)
        print(f"neighbourhood 1: iterations {one['iterations']} flags {one['flags']} n_corr {one['n_corr']}")
        assert one["n_corr"] < e["n_corr"]
        assert nd.align(src, cen, cells, table, d2, LEAF, min_b, div_b, max_iterations=2)["flags"] == nd.MAX_ITER_HIT
        far = nd.align(src + F32(100), cen, cells, table, d2, LEAF, min_b, div_b)
        assert far["flags"] == nd.FEW and far["n_corr"] == 0 and far["iterations"] == 0 and np.array_equal(far["pose"], EYE)
        same = np.repeat(src[:1], 8, axis=0)
        sing = nd.align(same, cen, cells, table, d2, LEAF, min_b, div_b)
        assert sing["flags"] == nd.SINGULAR and sing["n_corr"] == 8 and sing["iterations"] == 0


def test_restatement_voxels_of_a_point():
    """Step 2 on a 3 x 2 x 2 block of cells (all occupied, all valid, unit covariance) whose grid starts at cell (-1, 0, 4)."""
    cells = np.array([[i, j, k] for k in (4, 5) for j in (0, 1) for i in (-1, 0, 1)])
    tgt = ((cells + 0.5) * 0.5).astype(F32)
    table = np.zeros(len(cells), capi.VOXEL_COV_DTYPE)
    table["mean"], table["count"], table["flags"] = tgt, 10, 1
    table["icov"] = F32([1, 0, 0, 1, 0, 1])
    min_b, div_b = np.array([-1, 0, 4]), np.array([3, 2, 2])
    idx = nd.voxel_dict(cells)
    src = F32([[0.0, 0.5, 2.5],            # exact integers in qf * inv: the upper cells (0, 1, 5)
               [-0.5, 0.0, 2.0],           # the grid's own corner cell (-1, 0, 4)
               [-0.75, 0.25, 2.25],        # one cell outside in x: used through c + e0 alone
               [1.25, 0.25, 2.25],         # one cell outside above in x: used through c - e0 alone
               [-1.25, 0.25, 2.25],        # two cells outside: nothing
               [-0.25, 0.75, 2.25],        # cell (-1, 1, 4): c - e0 would alias onto (1, 0, 4) on the linear key
               [0.75, 0.25, 2.25],         # cell (1, 0, 4): c + e0 would alias onto (-1, 1, 4)
               [np.nan, 0, 2], [0, np.inf, 2], [0.1, 0.1, -np.inf]])
    e = nd.evaluate(src, tgt, cells, table, EYE, 1.0, LEAF, min_b, div_b)
    used = [sorted(int(v) for v in row if v >= 0) for row in e["used"]]
    at = lambda *c: idx[c]
    assert e["corr"]["idx"][0] == at(0, 1, 5) and e["corr"]["idx"][1] == at(-1, 0, 4)
    assert used[1] == sorted([at(-1, 0, 4), at(0, 0, 4), at(-1, 1, 4), at(-1, 0, 5)])
    assert used[2] == [at(-1, 0, 4)] and e["corr"]["idx"][2] == nd.NONE and e["corr"]["n_used"][2] == 1
    assert used[3] == [at(1, 0, 4)] and e["corr"]["idx"][3] == nd.NONE
    assert used[4] == [] and e["corr"]["score"][4] == 0
    assert at(1, 0, 4) not in used[5] and used[5] == sorted([at(-1, 1, 4), at(0, 1, 4), at(-1, 0, 4), at(-1, 1, 5)])
    assert at(-1, 1, 4) not in used[6] and used[6] == sorted([at(1, 0, 4), at(0, 0, 4), at(1, 1, 4), at(1, 0, 5)])
    assert all(u == [] for u in used[7:]) and (e["corr"]["idx"][7:] == nd.NONE).all() and e["n_corr"] == 6
    one = nd.evaluate(src, tgt, cells, table, EYE, 1.0, LEAF, min_b, div_b, neighborhood=1)
    assert one["corr"]["n_used"].tolist() == [1, 1, 0, 0, 0, 1, 1, 0, 0, 0]
    # the terms of the point at a voxel's mean: r = 0, w = 1, H = J^T B J with B = I
    p = nd.evaluate(tgt[:1], tgt, cells, table, EYE, 1.0, LEAF, min_b, div_b, neighborhood=1)
    a = tgt[0].astype(np.float64) - p["p0"]
    J = np.concatenate([np.cross(np.eye(3), a).T, np.eye(3)], axis=1)       # columns e_v x a, then e_v
    assert p["score"] == 1.0 and not p["g"].any() and np.allclose(p["H"], (J.T @ J)[np.tril_indices(6)], rtol=1e-15, atol=0)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def result_xyz(cm, res):
    rec = cm.result(res.n_out)
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(F32)


def result_bytes(a):
    return bytes(memoryview(a))


def grid_of(res, exact=False):
    """The result's own grid (min_b / div_b). A frame computed on a predicted box keeps its keys in a wider one; the outcome
    is the same in any grid that holds every occupied cell: a point or a candidate the narrower grid turns away has no
    occupied voxel to find in the wider one, and fsub is exact on cells below 2^24. exact: the keys' grid is this one."""
    if exact:
        assert not res.path_flags & capi.PATH_PREDICTED
    return np.array(res.min_b[:], np.int64), np.array(res.div_b[:], np.int64)


def check_eval(cm, res, src, leaf, guess=EYE, neighborhood=7, cov=(6, 0.01), label=""):
    """One evaluation (max_iterations 0) against the restatement on the DEVICE's covariance table: the correspondence table
    byte for byte, the sums by value, the fsum bound."""
    src = np.ascontiguousarray(src, F32)
    tgt = result_xyz(cm, res)
    cells, _ = cm.cells(res.n_out)
    table = cm.voxel_covariance(res.n_out, *cov)
    min_b, div_b = grid_of(res)
    got = cm.ndt_align(src, guess=guess, neighborhood=neighborhood, max_iterations=0, cov_min_points=cov[0], cov_eig_mult=cov[1])
    corr = cm.ndt_correspondences(len(src))
    d1, d2 = nd.gauss(leaf, 0.55)
    assert abs(got.gauss_d2 - d2) <= 1e-14 * d2 and abs(got.gauss_d1 - d1) <= 1e-14 * abs(d1)
    want = nd.evaluate(src, tgt, cells, table, guess, got.gauss_d2, leaf, min_b, div_b, neighborhood)
    assert corr.dtype == want["corr"].dtype and corr.shape == want["corr"].shape
    for f in ("idx", "n_used", "score"):
        if corr[f].tobytes() != want["corr"][f].tobytes():
            bad = np.nonzero(corr[f] != want["corr"][f])[0]
            raise AssertionError(f"{label}{f}: {len(bad)} of {len(src)} differ, first at {bad[:5]}: got {corr[f][bad[:5]]!r} "
                                 f"want {want['corr'][f][bad[:5]]!r} source {src[bad[:5]]}")
    assert corr.tobytes() == want["corr"].tobytes()
    H, g = np.array(got.H[:]), np.array(got.g[:])
    print(f"{label}n_src {len(src)} voxels {len(tgt)} valid {int((table['flags'] & 1).sum())} n_corr {got.n_corr} pairs "
          f"{int(corr['n_used'].sum())} cut {want['cut']} score {got.score:.6g}")
    assert got.n_corr == want["n_corr"] and got.iterations == 0
    assert got.flags == (capi.NDT_FEW if want["n_corr"] < 6 else 0)
    assert np.array_equal(H, want["H"]) and np.array_equal(g, want["g"]) and got.score == want["score"]
    assert np.array_equal(got.pose_matrix(), np.asarray(guess, float).reshape(3, 4))
    assert np.array_equal(np.array(got.pivot[:]), want["p0"])
    s = np.concatenate([H, g, [got.score]])
    t = want["terms"]
    for c in range(28):
        assert abs(s[c] - math.fsum(t[:, c].tolist())) <= 2 * len(src) * 2.0 ** -53 * np.abs(t[:, c]).sum()
    return got, corr, want, table, cells


def noisy_corner(n_per=10_000, hi=3.0, sigma=0.02, seed=17):
    """Three planes over [0, hi]^2 with Gaussian noise across them, and a dozen stray points in cells of their own."""
    rng = np.random.default_rng(seed)
    out = []
    for axis in range(3):
        p = rng.uniform(0, hi, (n_per, 3))
        p[:, axis] = rng.normal(0, sigma, n_per)
        out.append(p)
    strays = np.array([[1.2 + 0.5 * (k % 3), 1.3 + 0.5 * (k // 3 % 2), 1.1 + 0.5 * (k // 6)] for k in range(12)]) + \
        rng.uniform(-0.1, 0.1, (12, 3))
    return np.concatenate(out + [strays, strays[:4] + 0.01]).astype(F32)


def small_corner_frame(cm):
    pts = noisy_corner()
    cm.submit(0, xyzi_cloud(pts, np.ones(len(pts), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=LEAF, min_points_per_voxel=1))
    assert res.status == capi.OK and 80 <= res.n_out <= 260
    return res, pts


def border_points(res, cells, table, far):
    """For each of the six sides: a point beyond the grid by 0.3 (far: 1.8) of a cell, beside a valid voxel of the border layer."""
    min_b, div_b = grid_of(res)
    out = []
    valid = (table["flags"] & 1) != 0
    for a in range(3):
        for layer, sign in ((min_b[a], -1), (min_b[a] + div_b[a] - 1, 1)):
            k = np.nonzero(valid & (cells[:, a] == layer))[0]
            assert len(k), "no valid voxel in a border layer"
            p = table["mean"][k[0]].astype(np.float64)
            edge = (layer + (1 if sign > 0 else 0)) * 0.5
            p[a] = edge + sign * (0.9 if far else 0.15)     # cells of 0.5
            out.append(p)
    return np.array(out, F32)


def eval_sources(res, cells, table, seed=23):
    """769 records: points near the planes, random points around the box, multiples of the leaf (qf * inv an exact integer),
    points outside the grid by less and by more than a cell on all six sides, NaN and inf records."""
    rng = np.random.default_rng(seed)
    near = noisy_corner(150, seed=seed)[:450] + rng.normal(0, 0.05, (450, 3)).astype(F32)
    rnd = rng.uniform(-1.2, 4.2, (200, 3))
    exact = rng.integers(-1, 8, (60, 3)) * 0.5
    exact[:, rng.integers(0, 3)] = 0.0
    just = border_points(res, cells, table, far=False)
    far = border_points(res, cells, table, far=True)
    special = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan], [3e38, 3e38, 3e38], [1e30, 0, 0]])
    parts = [near, rnd, exact, just, far, special]
    xyz = np.concatenate(parts).astype(F32)
    kind = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    fill = 769 - len(xyz)
    assert fill >= 0
    xyz = np.concatenate([xyz, rng.uniform(0, 3, (fill, 3)).astype(F32)])
    kind = np.concatenate([kind, np.full(fill, 1)])
    perm = rng.permutation(769)
    return xyz[perm], kind[perm]


@pytest.mark.gpu
@pytest.mark.parametrize("neighborhood", [1, 7])
@pytest.mark.parametrize("guess", [EYE, GUESS, GUESS_Q], ids=["identity", "small", "quarter-turn"])
def test_one_evaluation_bit_for_bit(guess, neighborhood):
    with capi.CloudMerger(max_points_total=40_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res, pts = small_corner_frame(cm)
        cells, counts = cm.cells(res.n_out)
        table = cm.voxel_covariance(res.n_out)
        assert (counts < 6).sum() >= 4 and (table["flags"][counts < 6] == 0).all() and (table["flags"] & 1).sum() >= 60
        src, kind = eval_sources(res, cells, table)
        got, corr, want, _, _ = check_eval(cm, res, src, LEAF, guess, neighborhood)
        assert got.n_corr > 300
        for n in (257, 64, 1):                                             # the partial last block, one wave, one point
            check_eval(cm, res, src[:n], LEAF, guess, neighborhood, label=f"n {n}: ")
        _, qf = nd.transform(src, guess)
        if guess is not GUESS:
            # multiples of the leaf stay such under these poses and go to the upper cell: floor of the exact integer
            rows = np.nonzero(kind == 2)[0]
            assert len(rows) == 60 and (qf[rows] * F32(2) == np.floor(qf[rows] * F32(2))).all()
            hit = rows[corr["idx"][rows] != nd.NONE]
            assert len(hit) >= 5
            assert (cells[corr["idx"][hit]] == np.floor(qf[hit] * F32(2)).astype(np.int64)).all()
        if guess is EYE:
            just, far, special = (np.nonzero(kind == k)[0] for k in (3, 4, 5))
            assert (corr["idx"][just] == nd.NONE).all() and (corr["n_used"][far] == 0).all() and (corr["n_used"][special] == 0).all()
            if neighborhood == 7:
                assert (corr["n_used"][just] >= 1).all()                   # used, and only through a neighbour
            else:
                assert (corr["n_used"][just] == 0).all()
            if neighborhood == 7:
                ptr_src = cm.result_device()[0]                            # the device entry point: the result as the source
                a = cm.ndt_align_device(ptr_src, res.n_out, max_iterations=0)
                b = cm.ndt_align(cm.result(res.n_out), max_iterations=0)
                assert result_bytes(a) == result_bytes(b) and a.n_corr > 60


@pytest.mark.gpu
def test_the_x_border_does_not_alias(monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")                               # the keys' grid is the cloud's own: its borders are occupied
    with capi.CloudMerger(max_points_total=40_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res, _ = small_corner_frame(cm)
        cells, _ = cm.cells(res.n_out)
        table = cm.voxel_covariance(res.n_out)
        min_b, div_b = grid_of(res, exact=True)
        at = nd.voxel_dict(cells)
        valid = lambda c: c in at and bool(table["flags"][at[c]] & 1)
        lo, hi = int(min_b[0]), int(min_b[0] + div_b[0] - 1)
        src, alias = [], []
        for c in cells.tolist():                                           # lower border: (0, j, k) and (div0 - 1, j - 1, k)
            if c[0] == lo and valid(tuple(c)) and valid((hi, c[1] - 1, c[2])) and c[1] > min_b[1]:
                src.append((np.array(c) + 0.5) * 0.5)
                alias.append(at[(hi, c[1] - 1, c[2])])
                break
        for c in cells.tolist():                                           # upper border: (div0 - 1, j, k) and (0, j + 1, k)
            if c[0] == hi and valid(tuple(c)) and valid((lo, c[1] + 1, c[2])) and c[1] < min_b[1] + div_b[1] - 1:
                src.append((np.array(c) + 0.5) * 0.5)
                alias.append(at[(lo, c[1] + 1, c[2])])
                break
        assert len(src) == 2, "the fixture lacks the voxels an aliased neighbour would land on"
        src = np.array(src, F32)
        got, corr, want, _, _ = check_eval(cm, res, src, LEAF)
        for i in range(2):
            assert alias[i] not in want["used"][i].tolist() and corr["idx"][i] != nd.NONE
            # with the alias the point would have one voxel more: its m is finite, so it would count
            assert corr["n_used"][i] == (want["used"][i] >= 0).sum() <= 6


@pytest.mark.gpu
def test_the_cut_off_at_700():
    with capi.CloudMerger(max_points_total=40_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res, _ = small_corner_frame(cm)
        rng = np.random.default_rng(3)
        # in the layer of cells above the plane z = 0, towards its far side: the thin voxel below is a neighbour
        src = np.stack([rng.uniform(0.6, 2.4, 200), rng.uniform(0.6, 2.4, 200), rng.uniform(0.7, 0.99, 200)], axis=1).astype(F32)
        got, corr, want, table, cells = check_eval(cm, res, src, LEAF, cov=(6, 1e-4))
        assert want["cut"] >= 100
        below = want["used"][:, 5]                                          # c - e2
        rows = np.nonzero((below >= 0) & (corr["n_used"] == 1))[0]
        assert len(rows) >= 50 and (corr["score"][rows] == 0).all() and not np.signbit(corr["score"][rows]).any()
        assert got.n_corr >= len(rows)                                      # they count, and add zeros


def voxel_corner(cm, shift):
    tgt, src, truth = corner_scene(60_000, 5_000, shift)
    cm.submit(0, xyzi_cloud(tgt.astype(F32), np.ones(len(tgt), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=LEAF, min_points_per_voxel=0))
    assert res.status == capi.OK and 150 < res.n_out < 400
    return res, src, truth


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["origin", "1000m"])
def test_convergence_on_the_corner_scene(shift):
    with capi.CloudMerger(max_points_total=180_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res, src, truth = voxel_corner(cm, shift)
        tgt = result_xyz(cm, res)
        cells, _ = cm.cells(res.n_out)
        table = cm.voxel_covariance(res.n_out)                              # the device's table
        min_b, div_b = grid_of(res)
        got = cm.ndt_align(src)
        want = nd.align(src, tgt, cells, table, got.gauss_d2, LEAF, min_b, div_b)
        pose = got.pose_matrix()
        c = np.full(3, 2.0 + shift)
        e_dev, e_ref = pose_error(pose, truth, c), pose_error(want["pose"], truth, c)
        diff = np.abs(pose - want["pose"]).max()
        print(f"shift {shift}: iterations {got.iterations} / {want['iterations']} n_corr {got.n_corr} / {want['n_corr']} score "
              f"{got.score:.9g} / {want['score']:.9g} max |pose - restatement| {diff:.3g} error to the truth at the centre "
              f"{e_dev[0]:.6g} / {e_ref[0]:.6g} in R {e_dev[1]:.3g} / {e_ref[1]:.3g}")
        assert want["flags"] == nd.CONVERGED and len(src) == 15_000
        assert got.flags == want["flags"] and got.iterations == want["iterations"] and got.n_corr == want["n_corr"]
        assert diff <= 1e-9
        assert e_dev[0] <= 2 * CPU_ERROR[shift][0] and e_dev[1] <= 2 * CPU_ERROR[shift][1]
        # the final evaluation is the restatement's at the device's own pose
        fin = nd.evaluate(src, tgt, cells, table, pose, got.gauss_d2, LEAF, min_b, div_b)
        assert cm.ndt_correspondences(len(src)).tobytes() == fin["corr"].tobytes()
        assert np.array_equal(np.array(got.H[:]), fin["H"]) and np.array_equal(np.array(got.g[:]), fin["g"]) and got.score == fin["score"]


@pytest.mark.gpu
def test_stops():
    with capi.CloudMerger(max_points_total=180_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
        res, src, truth = voxel_corner(cm, 0.0)
        tgt = result_xyz(cm, res)
        cells, _ = cm.cells(res.n_out)
        table = cm.voxel_covariance(res.n_out)
        min_b, div_b = grid_of(res)
        far = cm.ndt_align(src + F32(100), guess=GUESS)                    # a source 100 m away
        assert far.flags == capi.NDT_FEW and far.n_corr == 0 and far.iterations == 0 and np.array_equal(far.pose_matrix(), GUESS)
        assert (cm.ndt_correspondences(len(src))["n_used"] == 0).all()
        names = [n for n, _ in cm.stage_times()]
        assert len(names) == len(set(names)) and "k_ndt_eval" in names and "k_aln_sum" in names and "k_cl_bounds" in names, names
        same = np.repeat(src[:1], 8, axis=0)                               # eight copies of one point: rank 3
        want = nd.align(same, tgt, cells, table, far.gauss_d2, LEAF, min_b, div_b)
        got = cm.ndt_align(same)
        assert got.flags == want["flags"] == capi.NDT_SINGULAR and got.iterations == 0 and got.n_corr == 8
        assert np.array_equal(got.pose_matrix(), EYE)
        b = cm.ndt_align(src, max_iterations=2)
        assert b.flags == capi.NDT_MAX_ITER_HIT and b.iterations == 2
        z = cm.ndt_align(src, guess=GUESS, max_iterations=0)               # a single evaluation at the guess
        e = nd.evaluate(src, tgt, cells, table, GUESS, z.gauss_d2, LEAF, min_b, div_b)
        assert z.flags == 0 and z.iterations == 0 and np.array_equal(z.pose_matrix(), GUESS) and z.score == e["score"]
        assert cm.ndt_correspondences(len(src)).tobytes() == e["corr"].tobytes()
        none = cm.ndt_align(np.zeros((0, 4), F32))                         # no source at all
        assert none.flags == capi.NDT_FEW and none.n_corr == 0 and len(cm.ndt_correspondences(0)) == 0


@pytest.mark.gpu
def test_table_reuse_and_non_interference():
    outs = []
    for first in (0, 1, 2):
        with capi.CloudMerger(max_points_total=180_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
            res, src, _ = voxel_corner(cm, 0.0)
            # first 0: no covariance call before this one's own
            others = lambda: (cm.voxel_covariance(res.n_out).tobytes() if first else None,
                              [x.tobytes() for x in cm.clusters(0.6, 1, 100_000)], cm.normals(10).tobytes(),
                              result_bytes(cm.align(src, 0.6, max_iterations=3)))
            before = others()
            if first == 1:
                ptr, n = cm.voxel_covariance_device(6, 0.01)                # the same parameters: the call reuses the table
                assert n == res.n_out
            if first == 2:
                cm.voxel_covariance_device(3, 0.05)                         # other parameters: the call computes its own
            a = cm.ndt_align(src, max_iterations=4)
            outs.append((result_bytes(a), cm.ndt_correspondences(len(src)).tobytes()))
            if first == 2:
                b = cm.ndt_align(src, max_iterations=4, cov_min_points=3, cov_eig_mult=0.05)
                assert result_bytes(b) != result_bytes(a)
                assert result_bytes(cm.ndt_align(src, max_iterations=4)) == result_bytes(a)
            assert before == others()
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.gpu
def test_a_held_table_is_not_computed_again():
    """Under CM_FLAG_PROFILE the call's stage list has the entry "voxel_cov" iff the call computed the table itself."""
    with capi.CloudMerger(max_points_total=180_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
        res, src, _ = voxel_corner(cm, 0.0)

        def computed(**kw):
            out = cm.ndt_align(src, max_iterations=1, **kw)
            names = [n for n, _ in cm.stage_times()]
            assert "k_ndt_eval" in names
            return "voxel_cov" in names, result_bytes(out)

        first = computed()                                                 # no table yet
        assert first[0]
        assert computed() == (False, first[1])                             # its own table, held
        cm.voxel_covariance_device(6, 0.01)
        assert computed() == (False, first[1])                             # a covariance call's at the same parameters
        cm.voxel_covariance_device(3, 0.05)
        assert computed() == (True, first[1])                              # ... at others: computed again
        assert computed(cov_min_points=3, cov_eig_mult=0.05)[0]            # other parameters of the call's own
        assert computed(cov_min_points=3, cov_eig_mult=0.05)[0] is False
        voxel_corner(cm, 0.0)                                              # a new frame: nothing is held
        assert computed(cov_min_points=3, cov_eig_mult=0.05)[0]


@pytest.mark.gpu
def test_requests_do_not_change_later_frames():
    """Two identical 12-frame streams on two contexts; one registers every frame's predecessor against its table."""
    n_per = 100_000
    runs = []
    for ask in (False, True):
        out, prev = [], None
        with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for k in range(12):
                sensors, _ = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2, wide=(k == 7))
                params = MergeParams(leaf=STREAM_LEAF, min_points_per_voxel=2)
                if k % 4 == 3:
                    params = MergeParams(leaf=STREAM_LEAF, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
                res = run_frame(cm, sensors, params)
                rec = cm.result(res.n_out)
                if ask and prev is not None:
                    a = cm.ndt_align(prev, max_iterations=3, cov_min_points=3)
                    assert a.n_corr > 100 and a.iterations >= 1                # (the call did real work)
                prev = rec
                cells, counts = cm.cells(res.n_out)
                out.append((res.status, res.n_out, res.path_flags, cm.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes()))
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {k} differs"
    print("path_flags of the stream:", [f[2] for f in runs[0]])


# the stream's scene at a leaf that leaves most voxels three points or more (at its own 5 cm few have them)
STREAM_LEAF = (0.2, 0.2, 0.2)


def previous_and_current(cm, prev_sensors, prev_params, sensors, params):
    res = run_frame(cm, prev_sensors, prev_params)
    assert res.status == capi.OK
    prev = result_xyz(cm, res)
    return prev, run_frame(cm, sensors, params)


@pytest.mark.gpu
def test_general_route(monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    before, _ = frame_sensors(n_per=120_000)
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        prev, res = previous_and_current(cm, before, MergeParams(**COARSE), sensors, MergeParams(**COARSE))
        assert not res.path_flags & capi.PATH_BUCKET
        got, *_ = check_eval(cm, res, prev, COARSE["leaf"], GUESS)
        assert got.n_corr > 100


@pytest.mark.gpu
def test_fixed_grid_route(monkeypatch):
    monkeypatch.setenv("CM_QUANT", "0")
    before, _ = frame_sensors(n_per=120_000)
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        prev, res = previous_and_current(cm, before, MergeParams(**COARSE, **CROP), sensors, MergeParams(**COARSE, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        got, *_ = check_eval(cm, res, prev, COARSE["leaf"], GUESS)
        assert got.n_corr > 100


@pytest.mark.gpu
def test_quantile_route():
    n_per = 150_000
    crop = dict(crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
    seen = []
    with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        prev = None
        for k in range(3):
            sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
            res = run_frame(cm, sensors, MergeParams(leaf=params.leaf, min_points_per_voxel=2, **crop))
            seen.append(res.path_flags)
            if prev is not None and res.path_flags & capi.PATH_QUANTILE:
                # (at the stream's own 5 cm few voxels hold three points: a few dozen source points find one)
                got, *_ = check_eval(cm, res, prev[:20_000], params.leaf, EYE, cov=(3, 0.01))
                assert got.n_corr > 10
                break
            prev = result_xyz(cm, res)
    assert seen[-1] & capi.PATH_QUANTILE, seen


def refused(cm, src, code=capi.BAD_ARG, **kw):
    """Both entry points refuse; the device one is given no source (n_src 0), which alone would be accepted."""
    with pytest.raises(capi.CloudMergeError) as e:
        cm.ndt_align(src, **kw)
    assert e.value.status == code and cm._lib.cm_last_error(cm._ctx)
    with pytest.raises(capi.CloudMergeError) as e:
        cm.ndt_align_device(None, 0, **kw)
    assert e.value.status == code


@pytest.mark.gpu
def test_refusals():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
    src = np.zeros((8, 4), F32)
    nan = float("nan")
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:     # a context without CM_FLAG_OCCUPANCY
        assert run_frame(cm, sensors, params).status == capi.OK
        refused(cm, src)
        assert b"OCCUPANCY" in cm._lib.cm_last_error(cm._ctx)
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        L, ctx = cm._lib, cm._ctx
        p, out, n = cm.ndt_params(), capi.NdtResult(), C.c_uint64(7)
        call = lambda: L.cm_result_ndt_align(ctx, C.byref(p), src.ctypes.data, len(src), C.byref(out))
        assert call() == capi.BAD_ARG and L.cm_last_error(ctx)              # no result yet
        assert L.cm_ndt_correspondences_copy(ctx, None, 0, C.byref(n)) == capi.BAD_ARG and n.value == 0
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        assert call() == capi.BAD_ARG and b"flight" in L.cm_last_error(ctx)
        res = cm.wait()
        assert res.status == capi.OK
        for kw in (dict(outlier_ratio=0.0), dict(outlier_ratio=1.0), dict(outlier_ratio=-0.1), dict(outlier_ratio=1.5),
                   dict(outlier_ratio=nan), dict(outlier_ratio=float("inf")), dict(neighborhood=0), dict(neighborhood=3),
                   dict(neighborhood=27), dict(max_iterations=65), dict(min_correspondences=5), dict(trans_eps=-1e-9),
                   dict(rot_eps=-1.0), dict(trans_eps=nan), dict(rot_eps=nan), dict(guess=np.full((3, 4), np.inf)),
                   dict(guess=np.where(np.arange(12).reshape(3, 4) == 7, nan, EYE)),
                   dict(cov_min_points=2), dict(cov_eig_mult=1.5), dict(cov_eig_mult=-0.1), dict(cov_eig_mult=nan),
                   dict(cov_min_points=0, cov_eig_mult=0.5)):
            refused(cm, src, **kw)
        assert L.cm_result_ndt_align(ctx, None, src.ctypes.data, len(src), C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_ndt_align(ctx, C.byref(p), src.ctypes.data, len(src), None) == capi.BAD_ARG
        assert L.cm_result_ndt_align(ctx, C.byref(p), None, 4, C.byref(out)) == capi.BAD_ARG and b"source" in L.cm_last_error(ctx)
        assert L.cm_result_ndt_align_device(ctx, C.byref(p), None, 4, C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_ndt_align_device(ctx, C.byref(p), cm.result_device()[0], 1 << 30, C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_ndt_align(ctx, C.byref(p), None, 0, C.byref(out)) == capi.OK and out.flags == capi.NDT_FEW   # n_src 0
        dflt = cm.ndt_align(cm.result(res.n_out), max_iterations=0, cov_min_points=0, cov_eig_mult=0.0)   # {0, 0}: {6, 0.01f}
        a = cm.ndt_align(cm.result(res.n_out), max_iterations=0)            # ... and a valid call afterwards succeeds
        assert a.n_corr > 0 and result_bytes(a) == result_bytes(dflt)
        corr = np.zeros(res.n_out, capi.NDT_CORR_DTYPE)
        assert L.cm_ndt_correspondences_copy(ctx, corr.ctypes.data, res.n_out - 1, C.byref(n)) == capi.CAPACITY
        assert n.value == res.n_out and L.cm_last_error(ctx) and not corr["n_used"].any()
        assert L.cm_ndt_correspondences_copy(ctx, corr.ctypes.data, res.n_out, C.byref(n)) == capi.OK
        used = corr["idx"] != nd.NONE
        assert used.any() and (corr["idx"][used] == np.arange(res.n_out)[used]).all()
        tiny = MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)
        res = run_frame(cm, sensors, tiny)
        assert res.status == capi.GRID_OVERFLOW                            # no voxel grid
        refused(cm, src)
        assert L.cm_ndt_correspondences_copy(ctx, corr.ctypes.data, len(corr), C.byref(n)) == capi.BAD_ARG   # a merge since
        for s in range(4):
            cm.clear(s)
        cm.submit(0, xyzi_cloud(np.full((4, 3), np.nan, F32)))
        assert cm.merge_voxelize(params).status == capi.EMPTY_INPUT
        refused(cm, src)
        cm.submit_all(sensors)
        assert cm.merge_partial(params, global_min_max=(-40, -40, -40, 40, 40, 40)).status == capi.OK
        refused(cm, src)                                                   # a partial table
        ptr, cnt = cm.partial_device()
        assert cm.merge_tables([ptr], [cnt], params).status == capi.OK
        refused(cm, src)                                                   # merged tables
        res = run_frame(cm, sensors, params)
        assert cm.ndt_align(cm.result(res.n_out), max_iterations=0).n_corr > 0
        # d2 not finite and > 0: c1 = 10 (1 - p) vanishes beside c2 = p / res3, so d1 = 0 and the quotient is 0 / 0
        for s in range(4):
            cm.clear(s)
        rng = np.random.default_rng(5)
        cm.submit(0, xyzi_cloud(rng.uniform(0, 0.005, (2_000, 3)).astype(F32)))
        fine = MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)
        res = cm.merge_voxelize(fine)
        assert res.status == capi.OK and res.n_out > 0
        almost_one = float(np.nextafter(F32(1), F32(0)))
        c1, c2 = 10.0 * (1.0 - almost_one), almost_one / float(np.prod(np.asarray(fine.leaf, F32).astype(np.float64)))
        assert c1 > 0 and c1 + c2 == c2 and c1 * math.exp(-0.5) + c2 == c2
        out.score, out.flags = 12.5, 77
        p = cm.ndt_params(outlier_ratio=almost_one)
        assert call() == capi.BAD_ARG and b"d2" in L.cm_last_error(ctx)
        assert out.score == 12.5 and out.flags == 77                        # a refused call leaves the outcome as it was
        refused(cm, src, outlier_ratio=almost_one)
        assert cm.ndt_align(cm.result(res.n_out), max_iterations=0).gauss_d2 > 0    # the same frame at the default ratio
