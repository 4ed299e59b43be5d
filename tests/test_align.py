"""Point-to-plane registration against the result: cm_result_align / cm_result_align_device / cm_align_correspondences_copy
(include/cloudmerge.h, cm_kernels_align.hip, cm_align_solve.hpp).

The bar: the correspondences (idx, d2) EXACTLY equal to the restatement (tests/align_ref.py) fed with the frame's own result;
H, g and sse equal to the restatement's tree sum by value (np.array_equal) on the device's own normals table, n_corr equal,
and all of them within 2 n 2^-53 sum|t| of math.fsum; on the corner scene the restatement's iteration count and flags, its
pose within 1e-9 per entry, and an error to the true pose of at most 1.01 x the restatement's."""
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
from tests import align_ref as ar
from tests import normals_ref as nr
from tests.test_cluster import COARSE, CROP, frame_sensors, hip_rt, run_frame, submit_as_voxels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")
F32 = np.float32
EYE = np.eye(3, 4)


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_align_structs_match_header(tmp_path):
    pf = ("max_corr_dist", "max_iterations", "normals_k", "min_correspondences", "trans_eps", "rot_eps", "guess")
    rf = ("pose", "H", "g", "sse", "rms", "pivot", "n_corr", "iterations", "flags")
    items = ["sizeof(cm_align_params)"] + [f"offsetof(cm_align_params,{f})" for f in pf] + ["sizeof(cm_align_result)"] + \
            [f"offsetof(cm_align_result,{f})" for f in rf] + \
            ["sizeof(cm_align_corr)", "offsetof(cm_align_corr,idx)", "offsetof(cm_align_corr,d2)", "(size_t)CM_ALIGN_MAX_ITER",
             "(size_t)CM_ALIGN_NONE", "(size_t)CM_ALIGN_CONVERGED", "(size_t)CM_ALIGN_MAX_ITER_HIT", "(size_t)CM_ALIGN_FEW",
             "(size_t)CM_ALIGN_SINGULAR", "(size_t)CM_VERSION", "(size_t)(CM_ALIGN_PIVOT_MIN * 1e12)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%zu ",(size_t)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, R, d = capi.AlignParams, capi.AlignResult, capi.ALIGN_CORR_DTYPE
    want = [C.sizeof(P)] + [getattr(P, f).offset for f in pf] + [C.sizeof(R)] + [getattr(R, f).offset for f in rf] + \
           [d.itemsize, d.fields["idx"][1], d.fields["d2"][1], capi.ALIGN_MAX_ITER, capi.ALIGN_NONE, capi.ALIGN_CONVERGED,
            capi.ALIGN_MAX_ITER_HIT, capi.ALIGN_FEW, capi.ALIGN_SINGULAR, 100, round(capi.ALIGN_PIVOT_MIN * 1e12)]
    assert got == want and got[0] == 128 and got[8] == 368 and got[18] == 8 and got[21] == 64 and got[-1] == 1000
    assert d == ar.CORR_DTYPE and (ar.NONE, ar.MAX_ITER, ar.PIVOT_MIN) == (capi.ALIGN_NONE, capi.ALIGN_MAX_ITER, capi.ALIGN_PIVOT_MIN)
    assert (ar.CONVERGED, ar.MAX_ITER_HIT, ar.FEW, ar.SINGULAR) == (1, 2, 4, 8)


def test_symbols_are_declared():
    text = open(HEADER).read()
    for name in ("cm_result_align", "cm_result_align_device", "cm_align_correspondences_copy"):
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CloudMerger.align_params(0.5)
    out = capi.AlignResult()
    src = np.zeros((4, 4), F32)
    assert L.cm_result_align(None, C.byref(p), src.ctypes.data, 4, C.byref(out)) == capi.BAD_ARG
    assert L.cm_result_align_device(None, C.byref(p), None, 0, C.byref(out)) == capi.BAD_ARG
    n = C.c_uint64()
    assert L.cm_align_correspondences_copy(None, None, 0, C.byref(n)) == capi.BAD_ARG


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def rodrigues(rv):
    th = np.linalg.norm(rv)
    k = np.asarray(rv, float) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def corner_points(n_per, rng, shift=0.0):
    out = []
    for axis in range(3):
        p = rng.uniform(0, 4, (n_per, 3))
        p[:, axis] = 0.0
        out.append(p)
    return np.concatenate(out) + shift


def corner_scene(n_tgt_per, n_src_per, shift=0.0, seed=41):
    """(target points fp64, source fp32, true pose (3, 4)): three planes over [0, 4]^2; the source is other samples of them
    moved by the inverse of the pose: rotation vector (1.5, -2, 3) degrees about (2, 2, 2) + shift, then (0.08, -0.05, 0.06)."""
    rng = np.random.default_rng(seed)
    tgt = corner_points(n_tgt_per, rng, shift)
    smp = corner_points(n_src_per, rng, shift)
    R = rodrigues(np.radians([1.5, -2.0, 3.0]))
    c = np.full(3, 2.0 + shift)
    t = c + np.array([0.08, -0.05, 0.06]) - R @ c
    src = (smp - t) @ R                                                    # R^T (x - t), row-wise
    return tgt, src.astype(F32), np.concatenate([R, t[:, None]], axis=1)


def pose_error(T, truth, c):
    """(distance between the images of c, Frobenius norm of the difference of the rotations)."""
    T, truth = np.asarray(T).reshape(3, 4), np.asarray(truth).reshape(3, 4)
    return (float(np.linalg.norm((T[:, :3] - truth[:, :3]) @ c + T[:, 3] - truth[:, 3])),
            float(np.linalg.norm(T[:, :3] - truth[:, :3])))


def lattice():
    g = [np.arange(m, dtype=F32) for m in (12, 10, 6)]
    xyz = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3)
    return xyz[np.random.default_rng(3).permutation(len(xyz))]


R_LAT = 1.0


def lattice_sources(n_random=2000, seed=7):
    """About 3 000 points for the 12 x 10 x 6 lattice at r = 1: cell centres, face centres and edge midpoints (8-, 4- and 2-way
    ties), random points in and around the box, points beyond the bounds by less and by more than r, NaN and inf records."""
    rng = np.random.default_rng(seed)
    h = lambda m: np.arange(m - 1, dtype=F32) + F32(0.5)
    i = lambda m: np.arange(m, dtype=F32)
    grid = lambda *ax: np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    ties8, ties4, ties2 = grid(h(12), h(10), h(6)), grid(h(12), h(10), i(6)), grid(h(12), i(10), i(6))
    ties4, ties2 = ties4[::2], ties2[::3]
    rnd = rng.uniform([-1.5, -1.5, -1.5], [12.5, 10.5, 6.5], (n_random, 3)).astype(F32)
    beyond = np.array([[-0.5, 3, 2], [-0.999, 3, 2], [-1.0, 3, 2], [-1.5, 3, 2], [11.75, 9.5, 5.5], [12.5, 4, 4], [3, 9.9, 5.9],
                       [3, 4, -0.75], [3, 4, 6.5], [-0.6, -0.6, -0.5], [-0.7, -0.7, -0.7], [11.5, 9.5, 5.2], [-0.3, -0.3, 0], [11.9, 3, 3],
                       [5, -0.9, 2], [5, 5, 5.99], [40, 40, 40], [-1e6, 0, 0],
                       [1e30, 1e30, 1e30]], F32)
    special = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan, np.nan, np.nan], [3e38, 3e38, 3e38]], F32)
    xyz = np.concatenate([ties8, ties4, ties2, rnd, beyond, special]).astype(F32)
    kind = np.concatenate([np.full(len(a), k) for k, a in enumerate((ties8, ties4, ties2, rnd, beyond, special))])
    perm = rng.permutation(len(xyz))
    return xyz[perm], kind[perm]


GUESS = np.concatenate([rodrigues(np.radians([2.0, -1.0, 1.5])), np.array([[0.03], [-0.02], [0.04]])], axis=1)
# exactly representable: a quarter turn about z and a shift: maps lattice points onto lattice points, and the ties with them
GUESS_Q = np.array([[0.0, -1.0, 0.0, 9.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree():
    tgt = lattice()
    src, kind = lattice_sources()
    assert 2800 <= len(src) <= 3300
    for T in (EYE, GUESS, GUESS_Q):
        _, qf = ar.transform(src, T)
        stats = {}
        a = ar.match_brute(qf, tgt, R_LAT)
        b = ar.match_tree(qf, tgt, R_LAT)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        b = ar.match_tree(qf, tgt, R_LAT, kq=4, stats=stats)               # lists too short for the 8-way ties
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        if T is not GUESS:                                                 # (a general pose leaves no exact ties)
            assert 0 < stats["brute_rows"] < len(src)                      # both branches of the tree restatement ran
    # at identity: every cell centre matched at d2 0.75 to the smallest of its 8 corners, and so on
    idx, d2 = ar.match_brute(src, tgt, R_LAT)
    for k, want_d2, ways in ((0, 0.75, 8), (1, 0.5, 4), (2, 0.25, 2)):
        rows = np.nonzero(kind == k)[0]
        assert len(rows) > 100 and (d2[rows] == F32(want_d2)).all()
        d = nr.d2_f32(src[rows][:, None, :], tgt[None, :, :])
        tied = d == F32(want_d2)
        assert (tied.sum(axis=1) == ways).all() and (idx[rows] == tied.argmax(axis=1)).all()
    assert (idx[kind == 5] == ar.NONE).all() and (d2[kind == 5] == 0).all()
    assert (idx[kind == 4] == ar.NONE).sum() >= 6 and (idx[kind == 4] != ar.NONE).sum() >= 6


def test_the_radius_is_strict_in_the_restatement():
    tgt = F32([[0, 0, 0]])
    src = F32([[3, 4, 0], [0, -3, 4], [0, 0, 5]])
    assert (ar.match_brute(src, tgt, 5.0)[0] == ar.NONE).all()
    idx, d2 = ar.match_brute(src, tgt, np.nextafter(F32(5), F32(6)))
    assert (idx == 0).all() and (d2 == 25).all()


def small_corner():
    tgt, src, truth = corner_scene(700, 400)
    tgt = tgt.astype(F32)
    tbl, _ = nr.table(tgt, 10)
    return tgt, src, truth, tbl


def test_tree_sum_against_fsum_and_the_order_of_a_wave():
    tgt, src, _, tbl = small_corner()
    for n in (1200, 257, 769, 64, 1):
        e = ar.evaluate(src[:n], tgt, tbl, EYE, 0.4)
        q64, qf = ar.transform(src[:n], EYE)
        t, has = ar.terms(q64, tgt, tbl, e["corr"]["idx"], e["p0"])
        assert has.sum() == e["n_corr"] > 0.9 * n
        s = np.concatenate([e["H"], e["g"], [e["sse"]]])
        for k in range(28):
            exact = math.fsum(t[:, k].tolist())
            assert abs(s[k] - exact) <= 2 * n * 2.0 ** -53 * np.abs(t[:, k]).sum()
    # the order inside a wave, on integers-valued terms whose float sum depends on it
    v = np.zeros((256 * 2 + 3, 1))
    v[:, 0] = 2.0 ** 53 * (np.arange(len(v)) % 3 == 0) + 1.0
    want = 0.0
    for b in range(3):
        blk = v[256 * b: 256 * (b + 1), 0].tolist() + [0.0] * (256 - len(v[256 * b: 256 * (b + 1)]))
        waves = []
        for w in range(4):
            lane = blk[64 * w: 64 * (w + 1)]
            for s in (32, 16, 8, 4, 2, 1):
                lane = [lane[l] + lane[l + s] for l in range(s)]
            waves.append(lane[0])
        want = want + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    assert ar.tree_sum(v)[0] == want != math.fsum(v[:, 0].tolist())


def test_the_sign_of_a_normal_cancels_exactly():
    tgt, src, _, tbl = small_corner()
    flipped = tbl.copy()
    flipped["normal"][::2] = -flipped["normal"][::2]
    a, b = ar.evaluate(src, tgt, tbl, GUESS, 0.4), ar.evaluate(src, tgt, flipped, GUESS, 0.4)
    assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["g"], b["g"]) and a["sse"] == b["sse"]


def test_restatement_converges_on_the_corner():
    tgt, src, truth, tbl = small_corner()
    e = ar.align(src, tgt, tbl, 0.4, trans_eps=1e-7, rot_eps=1e-7)
    assert e["flags"] == ar.CONVERGED and 3 <= e["iterations"] <= 8 and e["n_corr"] == len(src)
    dp, dr = pose_error(e["pose"], truth, np.full(3, 2.0))
    assert dp < 5e-3 and dr < 2e-3 and e["rms"] < 0.02
    assert ar.align(src, tgt, tbl, 0.4, max_iterations=2)["flags"] == ar.MAX_ITER_HIT
    far = ar.align(src + F32(50), tgt, tbl, 0.4)
    assert far["flags"] == ar.FEW and far["n_corr"] == 0 and far["iterations"] == 0 and np.array_equal(far["pose"], EYE)


# ---- CPU: cm_align_solve.hpp ------------------------------------------------------------------------------------------------
SOLVE_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include "cm_align_solve.hpp"
static double rd() { unsigned long long u; if (std::scanf("%llx", &u) != 1) std::exit(2); double d; std::memcpy(&d, &u, 8); return d; }
static void wr(double d) { unsigned long long u; std::memcpy(&u, &d, 8); std::printf("%016llx ", u); }
int main() {
    double H[21], g[6], pose[12], p0[3], x[6] = {0, 0, 0, 0, 0, 0};
    for (double& v : H) v = rd();
    for (double& v : g) v = rd();
    for (double& v : pose) v = rd();
    for (double& v : p0) v = rd();
    const bool ok = cm_align_solve(H, g, x);
    std::printf("%d ", ok ? 1 : 0);
    if (ok) cm_align_update(pose, x, p0);
    for (double v : x) wr(v);
    for (double v : pose) wr(v);
    std::printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def solve_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("align_solve")
    (d / "driver.cpp").write_text(SOLVE_DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, str(d / "driver.cpp"),
                    "-o", str(exe)], check=True)

    def run(H, g, pose, p0):
        vals = np.concatenate([np.ravel(H), np.ravel(g), np.ravel(pose), np.ravel(p0)]).astype(np.float64)
        text = " ".join("%016x" % int(v) for v in vals.view(np.uint64))
        out = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True).stdout.split()
        f = np.array([int(v, 16) for v in out[1:]], np.uint64).view(np.float64)
        return out[0] == "1", f[:6], f[6:].reshape(3, 4)
    return run


def full(H21):
    A = np.zeros((6, 6))
    A[np.tril_indices(6)] = H21
    return A + np.tril(A, -1).T


def test_solve_against_numpy_on_the_corner(solve_driver):
    tgt, src, _, tbl = small_corner()
    e = ar.evaluate(src, tgt, tbl, GUESS, 0.4)
    ok, x, pose = solve_driver(e["H"], e["g"], GUESS, e["p0"])
    want = np.linalg.solve(full(e["H"]), -e["g"])
    assert ok and np.abs(x - want).max() <= 1e-10 * np.abs(want).max() and np.abs(want).max() > 1e-3
    mine = ar.solve(e["H"], e["g"])
    assert np.array_equal(x, mine)                                         # the restatement: the same operations
    up = ar.update(GUESS, mine, e["p0"])
    assert np.abs(pose - up).max() <= 1e-15
    # the update is a rigid motion about the pivot: p0 moves by v, R stays orthonormal
    R = pose[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    moved = pose[:, :3] @ e["p0"] + pose[:, 3] - (GUESS[:, :3] @ e["p0"] + GUESS[:, 3])
    W = rodrigues(x[:3])
    assert np.abs(moved - ((W - np.eye(3)) @ (GUESS[:, :3] @ e["p0"] + GUESS[:, 3] - e["p0"]) + x[3:])).max() < 1e-12


def test_solve_zero_gradient_is_the_identity(solve_driver):
    tgt, src, _, tbl = small_corner()
    e = ar.evaluate(src, tgt, tbl, EYE, 0.4)
    ok, x, pose = solve_driver(e["H"], np.zeros(6), EYE, e["p0"])
    assert ok and not x.any() and np.array_equal(pose, EYE)
    assert np.array_equal(ar.update(EYE, ar.solve(e["H"], np.zeros(6)), e["p0"]), EYE)


def test_solve_calls_a_plane_singular(solve_driver):
    g = np.arange(20, dtype=F32)
    tgt = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1), F32)], axis=1).astype(F32)
    tbl, _ = nr.table(tgt, 9)
    assert (tbl["flags"] == 1).all()
    src = (tgt + F32([0.1, 0.1, 0.05])).astype(F32)
    e = ar.evaluate(src, tgt, tbl, EYE, 0.5)
    assert e["n_corr"] == len(src)
    ok, x, pose = solve_driver(e["H"], e["g"], GUESS, e["p0"])
    assert not ok and np.array_equal(pose, GUESS) and ar.solve(e["H"], e["g"]) is None
    nan = e["H"].copy()
    nan[0] = np.nan
    assert not solve_driver(nan, e["g"], GUESS, e["p0"])[0] and ar.solve(nan, e["g"]) is None
    r = ar.align(src, tgt, tbl, 0.5, guess=EYE)
    assert r["flags"] == ar.SINGULAR and r["iterations"] == 0 and np.array_equal(r["pose"], EYE)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def result_xyz(cm, res):
    rec = cm.result(res.n_out)
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(F32)


def sums_of(a):
    return np.array(a.H[:]), np.array(a.g[:]), float(a.sse)


def result_bytes(a):
    return bytes(memoryview(a))


def check_eval(cm, res, src, r, guess=EYE, k=9, tree=False, label=""):
    """One evaluation (max_iterations 0) against the restatement: correspondences bit for bit, sums by value, the fsum bound."""
    src = np.ascontiguousarray(src, F32)
    tgt = result_xyz(cm, res)
    tbl = cm.normals(k) if res.n_out else np.zeros(0, capi.VOXEL_NORMAL_DTYPE)
    want = ar.evaluate(src, tgt, tbl, guess, r, tree=tree)
    got = cm.align(src, r, guess=guess, max_iterations=0, normals_k=k)
    corr = cm.align_correspondences(len(src))
    assert corr.dtype == want["corr"].dtype and corr.shape == want["corr"].shape
    for f in ("idx", "d2"):
        if corr[f].tobytes() != want["corr"][f].tobytes():
            bad = np.nonzero(corr[f].view(np.uint32) != want["corr"][f].view(np.uint32))[0]
            raise AssertionError(f"{label}{f}: {len(bad)} of {len(src)} differ, first at {bad[:5]}: got {corr[f][bad[:5]]} "
                                 f"want {want['corr'][f][bad[:5]]} source {src[bad[:5]]}")
    H, g, sse = sums_of(got)
    print(f"{label}n_src {len(src)} n_tgt {len(tgt)} matched {int((corr['idx'] != ar.NONE).sum())} n_corr {got.n_corr} sse {sse:.6g}")
    assert got.n_corr == want["n_corr"] and got.iterations == 0
    assert got.flags == (capi.ALIGN_FEW if want["n_corr"] < 6 else 0)
    assert np.array_equal(H, want["H"]) and np.array_equal(g, want["g"]) and sse == want["sse"]
    assert np.array_equal(np.array(got.pose[:]).reshape(3, 4), np.asarray(guess, float).reshape(3, 4))
    if len(tgt):
        assert np.array_equal(np.array(got.pivot[:]), want["p0"])
    assert got.rms == (math.sqrt(sse / got.n_corr) if got.n_corr else 0.0)
    q64, _ = ar.transform(src, guess)
    t, _ = ar.terms(q64, tgt, tbl, want["corr"]["idx"], want["p0"])
    s = np.concatenate([H, g, [sse]])
    for c in range(28):
        assert abs(s[c] - math.fsum(t[:, c].tolist())) <= 2 * len(src) * 2.0 ** -53 * np.abs(t[:, c]).sum()
    return got, corr, want


@pytest.mark.gpu
@pytest.mark.parametrize("guess", [EYE, GUESS, GUESS_Q], ids=["identity", "small", "quarter-turn"])
def test_exact_match_and_sums_on_a_lattice(guess):
    tgt = lattice()
    src, kind = lattice_sources()
    with capi.CloudMerger(max_points_total=len(tgt), max_sensors=1) as cm:
        res = submit_as_voxels(cm, tgt, 0.25, 0)
        got, corr, want = check_eval(cm, res, src, R_LAT, guess)
        assert got.n_corr > 1000
        if guess is not GUESS:
            # the ties are there and went to the smaller index (the quarter turn maps the lattice onto itself)
            _, qf = ar.transform(src, guess)
            xyz = result_xyz(cm, res)
            for k, want_d2, ways in ((0, 0.75, 8), (1, 0.5, 4), (2, 0.25, 2)):
                inside = ((qf >= 0) & (qf <= F32([11, 9, 5]))).all(axis=1)       # (all of its corners are lattice points)
                rows = np.nonzero((kind == k) & inside)[0]
                assert len(rows) > 50
                d = nr.d2_f32(qf[rows][:, None, :], xyz[None, :, :])
                tied = d == F32(want_d2)
                assert (corr["d2"][rows] == F32(want_d2)).all() and (tied.sum(axis=1) == ways).all()
                assert (corr["idx"][rows] == tied.argmax(axis=1)).all()
        if guess is EYE:
            assert (corr["idx"][kind == 5] == ar.NONE).all() and (corr["d2"][kind == 5] == 0).all()
            out = corr["idx"][kind == 4]
            assert (out == ar.NONE).sum() >= 6 and (out != ar.NONE).sum() >= 6
            # the partial last block, several blocks, one wave, one point
            for n in (257, 256 * 3 + 1, 64, 1):
                check_eval(cm, res, src[:n], R_LAT, guess, label=f"n {n}: ")
            ptr_src = cm.result_device()[0]                                # the device entry point: the result against itself
            a = cm.align_device(ptr_src, res.n_out, R_LAT, max_iterations=0, normals_k=9)
            b = cm.align(cm.result(res.n_out), R_LAT, max_iterations=0, normals_k=9)
            assert result_bytes(a) == result_bytes(b) and a.sse == 0 and a.n_corr > 0
            c2 = cm.align_correspondences(res.n_out)
            assert (c2["idx"] == np.arange(res.n_out)).all() and not c2["d2"].any()


@pytest.mark.gpu
def test_the_radius_is_strict_on_results_of_one_and_two_voxels():
    r_up = float(np.nextafter(F32(5), F32(6)))
    src = F32([[3, 4, 0], [0, -3, 4], [0, 0, 5], [103, 4, 0], [97, -4, 0], [50, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1e30, 0, 0]])
    for tgt in (F32([[0, 0, 0]]), F32([[0, 0, 0], [100, 0, 0]])):
        with capi.CloudMerger(max_points_total=8, max_sensors=1) as cm:
            res = submit_as_voxels(cm, tgt, 0.25, 0)
            _, corr, _ = check_eval(cm, res, src, 5.0)
            assert (corr["idx"][:6] == ar.NONE).all() and corr["idx"][6] != ar.NONE
            got, corr, _ = check_eval(cm, res, src, r_up)
            assert (corr["idx"][:3] != ar.NONE).all() and (corr["d2"][:3] == 25).all() and got.n_corr == 0
            assert ((corr["idx"][3:5] != ar.NONE).all() and (corr["d2"][3:5] == 25).all()) == (len(tgt) == 2)
            assert (corr["idx"][[5, 7, 8]] == ar.NONE).all()


@pytest.mark.gpu
def test_two_blobs_300_m_apart_with_a_small_radius():
    """r = 0.05 over 300 m: 6 000 cells along x exceed the grid's 4 096 per axis, so the cell doubles."""
    rng = np.random.default_rng(11)
    blob = lambda c: c + rng.uniform(-1, 1, (1500, 3))
    tgt = np.concatenate([blob(np.zeros(3)), blob(np.array([300.0, 20.0, -3.0]))]).astype(F32)
    _, first = np.unique(np.floor(tgt.astype(np.float64) / 0.0625).astype(np.int64), axis=0, return_index=True)
    tgt = tgt[np.sort(first)]                                              # the first point of every voxel
    src = np.concatenate([tgt[::2] + rng.normal(0, 0.02, (len(tgt[::2]), 3)), blob(np.array([300.0, 20.0, -3.0])),
                          [[150.0, 10.0, 0.0], [301.5, 20.0, -3.0], [-1.04, 0.0, 0.0]]]).astype(F32)
    with capi.CloudMerger(max_points_total=len(tgt), max_sensors=1) as cm:
        res = submit_as_voxels(cm, tgt, 0.0625, 0)
        assert res.n_out > 2900
        got, corr, _ = check_eval(cm, res, src, 0.05, k=9, tree=True)
        hit = corr["idx"] != ar.NONE
        assert 500 < hit.sum() < len(src) - 500


def voxel_corner(cm, shift, n_tgt_per=20_000, n_src_per=5_000):
    tgt, src, truth = corner_scene(n_tgt_per, n_src_per, shift)
    cm.submit(0, xyzi_cloud(tgt.astype(F32), np.ones(len(tgt), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0))
    assert res.status == capi.OK and 4000 < res.n_out < 5500
    return res, src, truth


CORNER = dict(max_iterations=30, normals_k=10, trans_eps=1e-7, rot_eps=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1000.0], ids=["origin", "1000m"])
def test_convergence_on_the_corner_scene(shift):
    with capi.CloudMerger(max_points_total=60_000, max_sensors=1) as cm:
        res, src, truth = voxel_corner(cm, shift)
        tgt, tbl = result_xyz(cm, res), cm.normals(10)
        want = ar.align(src, tgt, tbl, 0.4, trans_eps=1e-7, rot_eps=1e-7)
        got = cm.align(src, 0.4, **CORNER)
        pose = got.pose_matrix()
        c = np.full(3, 2.0 + shift)
        e_dev, e_ref = pose_error(pose, truth, c), pose_error(want["pose"], truth, c)
        diff = np.abs(pose - want["pose"]).max()
        print(f"shift {shift}: iterations {got.iterations} / {want['iterations']} n_corr {got.n_corr} / {want['n_corr']} rms "
              f"{got.rms:.6g} / {want['rms']:.6g} max |pose - restatement| {diff:.3g} error to the truth at the pivot "
              f"{e_dev[0]:.6g} / {e_ref[0]:.6g} in R {e_dev[1]:.3g} / {e_ref[1]:.3g}")
        assert want["flags"] == ar.CONVERGED and want["n_corr"] == len(src) == 15_000 and want["iterations"] <= 8
        assert got.flags == capi.ALIGN_CONVERGED and got.iterations == want["iterations"] and got.n_corr == want["n_corr"]
        assert diff <= 1e-9
        assert e_dev[0] <= 1.01 * e_ref[0] and e_dev[1] <= 1.01 * e_ref[1]
        assert e_ref[0] < 2e-3 and e_ref[1] < 5e-4 and got.rms < 0.01           # (the scene is the one meant: 0.7 mm, 1e-4, 4 mm)
        # the final evaluation is the restatement's at the device's own pose
        fin = ar.evaluate(src, tgt, tbl, pose, 0.4)
        assert cm.align_correspondences(len(src)).tobytes() == fin["corr"].tobytes()
        assert np.array_equal(np.array(got.H[:]), fin["H"]) and np.array_equal(np.array(got.g[:]), fin["g"]) and got.sse == fin["sse"]


@pytest.mark.gpu
def test_fixed_points_and_stops():
    with capi.CloudMerger(max_points_total=60_000, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        res, src, truth = voxel_corner(cm, 0.0)
        own = cm.result(res.n_out)
        a = cm.align(own, 0.4, **CORNER)                                   # the result against itself
        assert a.flags == capi.ALIGN_CONVERGED and a.iterations == 1 and a.sse == 0 and a.rms == 0
        assert np.array_equal(a.pose_matrix(), EYE) and not np.array(a.g[:]).any() and 0 < a.n_corr <= res.n_out
        names = [n for n, _ in cm.stage_times()]
        assert len(names) == len(set(names)) and len(names) <= 48
        for want in ("k_cl_bounds", "k_cl_keys", "k_cl_gather", "cl_rows", "k_aln_eval", "k_aln_sum"):
            assert want in names, names
        b = cm.align(src, 0.4, max_iterations=2, normals_k=10, trans_eps=1e-7, rot_eps=1e-7)
        assert b.flags == capi.ALIGN_MAX_ITER_HIT and b.iterations == 2
        far = cm.align(src + F32(50), 0.4, **CORNER)                       # a source far away
        assert far.flags == capi.ALIGN_FEW and far.n_corr == 0 and far.iterations == 0 and np.array_equal(far.pose_matrix(), EYE)
        assert (cm.align_correspondences(len(src))["idx"] == ar.NONE).all()
        none = cm.align(np.zeros((0, 4), F32), 0.4, **CORNER)              # no source at all
        assert none.flags == capi.ALIGN_FEW and none.n_corr == 0 and len(cm.align_correspondences(0)) == 0
    g = np.arange(20, dtype=F32)
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    plane = np.concatenate([plane, np.zeros((len(plane), 1), F32)], axis=1).astype(F32)
    with capi.CloudMerger(max_points_total=len(plane), max_sensors=1) as cm:
        res = submit_as_voxels(cm, plane, 0.25, 0)
        src = (plane + F32([0.1, 0.1, 0.05])).astype(F32)
        want = ar.align(src, result_xyz(cm, res), cm.normals(9), 0.5, guess=EYE)
        got = cm.align(src, 0.5, normals_k=9)
        assert got.flags == want["flags"] == capi.ALIGN_SINGULAR and got.iterations == 0 and got.n_corr == len(src)
        assert np.array_equal(got.pose_matrix(), EYE)
        tilt = np.concatenate([rodrigues(np.radians([0.0, 0.0, 1.0])), [[0.01], [0.0], [0.0]]], axis=1)
        got = cm.align(src, 0.5, guess=tilt, normals_k=9)
        assert got.flags & capi.ALIGN_SINGULAR and np.array_equal(got.pose_matrix(), tilt)


@pytest.mark.gpu
def test_table_reuse_and_non_interference():
    outs = []
    for first in (False, True):
        with capi.CloudMerger(max_points_total=60_000, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
            res, src, _ = voxel_corner(cm, 0.0)
            cl0 = cm.clusters(0.15, 2, 100_000)
            if first:
                kept = cm.normals(10, viewpoint=(1.0, 2.0, 30.0))
                ptr, _ = cm.normals_device(10, viewpoint=(1.0, 2.0, 30.0))
            a = cm.align(src, 0.4, **CORNER)
            outs.append((result_bytes(a), cm.align_correspondences(len(src)).tobytes()))
            if first:
                # the table the context holds is still the one turned to that viewpoint: the call did not compute its own ...
                now = np.zeros_like(kept)
                assert hip_rt().hipMemcpy(C.c_void_p(now.ctypes.data), C.c_void_p(ptr), C.c_size_t(now.nbytes), 2) == 0
                assert now.tobytes() == kept.tobytes() != cm.normals(10).tobytes()
                cm.normals(10, viewpoint=(1.0, 2.0, 30.0))
                b = cm.align(src, 0.4, **{**CORNER, "normals_k": 12})      # ... and another k makes it do so
                assert result_bytes(b) != result_bytes(a)
                assert cm.normals(12).tobytes() != kept.tobytes()
                c = cm.align(src, 0.4, **CORNER)                           # back at k = 10: recomputed, the same outcome
                assert result_bytes(c) == result_bytes(a)
            cl1 = cm.clusters(0.15, 2, 100_000)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(cl0, cl1)) and len(cl0[1]) >= 1
    assert outs[0] == outs[1]


@pytest.mark.gpu
def test_requests_do_not_change_later_frames():
    """Two identical 12-frame streams on two contexts; one aligns every frame's result to its predecessor."""
    n_per = 100_000
    runs = []
    for ask in (False, True):
        out, prev = [], None
        with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for k in range(12):
                sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2, wide=(k == 7))
                if k % 4 == 3:
                    params = MergeParams(leaf=params.leaf, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
                res = run_frame(cm, sensors, params)
                rec = cm.result(res.n_out)
                if ask and prev is not None:
                    a = cm.align(prev, 0.5, max_iterations=3)
                    assert a.n_corr > 100 and a.iterations >= 1                # (the call did real work)
                prev = rec
                cells, counts = cm.cells(res.n_out)
                out.append((res.status, res.n_out, res.path_flags, cm.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes()))
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        assert a == b, f"frame {k} differs"
    assert any(f[2] & capi.PATH_QUANTILE for f in runs[0])


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
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5) as cm:
        prev, res = previous_and_current(cm, before, MergeParams(**COARSE), sensors, MergeParams(**COARSE))
        assert not res.path_flags & capi.PATH_BUCKET
        check_eval(cm, res, prev, 1.0, GUESS, k=10, tree=True)


@pytest.mark.gpu
def test_fixed_grid_route(monkeypatch):
    monkeypatch.setenv("CM_QUANT", "0")
    before, _ = frame_sensors(n_per=120_000)
    sensors, n_cap = frame_sensors()
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=5) as cm:
        prev, res = previous_and_current(cm, before, MergeParams(**COARSE, **CROP), sensors, MergeParams(**COARSE, **CROP))
        assert res.path_flags & capi.PATH_BUCKET and not res.path_flags & capi.PATH_QUANTILE
        check_eval(cm, res, prev, 1.0, GUESS, k=10, tree=True)


@pytest.mark.gpu
def test_quantile_route():
    n_per = 150_000
    crop = dict(crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)
    seen = []
    with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4) as cm:
        prev = None
        for k in range(3):
            sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2)
            res = run_frame(cm, sensors, MergeParams(leaf=params.leaf, min_points_per_voxel=2, **crop))
            seen.append(res.path_flags)
            if prev is not None and res.path_flags & capi.PATH_QUANTILE:
                check_eval(cm, res, prev, 0.2, EYE, k=10, tree=True)
                break
            prev = result_xyz(cm, res)
    assert seen[-1] & capi.PATH_QUANTILE, seen


def refused(cm, src, code=capi.BAD_ARG, **kw):
    """Both entry points refuse; the device one is given no source (n_src 0), which alone would be accepted."""
    args = dict(max_corr_dist=0.5)
    args.update(kw)
    r = args.pop("max_corr_dist")
    with pytest.raises(capi.CloudMergeError) as e:
        cm.align(src, r, **args)
    assert e.value.status == code and cm._lib.cm_last_error(cm._ctx)
    with pytest.raises(capi.CloudMergeError) as e:
        cm.align_device(None, 0, r, **args)
    assert e.value.status == code


@pytest.mark.gpu
def test_refusals():
    sensors, _ = synth.config2(n_per_sensor=20_000, min_pts=0)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
    src = np.zeros((8, 4), F32)
    nan = float("nan")
    with capi.CloudMerger(max_points_total=80_000, max_sensors=4) as cm:
        L, ctx = cm._lib, cm._ctx
        p, out, n = cm.align_params(0.5), capi.AlignResult(), C.c_uint64(7)
        call = lambda: L.cm_result_align(ctx, C.byref(p), src.ctypes.data, len(src), C.byref(out))
        assert call() == capi.BAD_ARG and L.cm_last_error(ctx)              # no result yet
        assert L.cm_align_correspondences_copy(ctx, None, 0, C.byref(n)) == capi.BAD_ARG and n.value == 0
        cm.submit_all(sensors)
        cm.merge_voxelize_async(capi.make_params(params))
        assert call() == capi.BAD_ARG and b"flight" in L.cm_last_error(ctx)
        res = cm.wait()
        assert res.status == capi.OK
        for r in (0.0, -1.0, nan, float("inf"), 1e-30, 1e30):
            refused(cm, src, max_corr_dist=r)
        for kw in (dict(normals_k=2), dict(normals_k=65), dict(max_iterations=65), dict(min_correspondences=5), dict(trans_eps=-1e-9),
                   dict(rot_eps=-1.0), dict(trans_eps=nan), dict(rot_eps=nan), dict(guess=np.full((3, 4), np.inf)),
                   dict(guess=np.where(np.arange(12).reshape(3, 4) == 7, nan, EYE))):
            refused(cm, src, **kw)
        assert L.cm_result_align(ctx, None, src.ctypes.data, len(src), C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_align(ctx, C.byref(p), src.ctypes.data, len(src), None) == capi.BAD_ARG
        assert L.cm_result_align(ctx, C.byref(p), None, 4, C.byref(out)) == capi.BAD_ARG and b"source" in L.cm_last_error(ctx)
        assert L.cm_result_align_device(ctx, C.byref(p), None, 4, C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_align_device(ctx, C.byref(p), cm.result_device()[0], 1 << 30, C.byref(out)) == capi.BAD_ARG
        assert L.cm_result_align(ctx, C.byref(p), None, 0, C.byref(out)) == capi.OK and out.flags == capi.ALIGN_FEW   # n_src 0
        a = cm.align(cm.result(res.n_out), 0.5, max_iterations=0)           # ... and a valid call afterwards succeeds
        assert a.n_corr > 0 and a.sse == 0
        corr = np.zeros(res.n_out, capi.ALIGN_CORR_DTYPE)
        assert L.cm_align_correspondences_copy(ctx, corr.ctypes.data, res.n_out - 1, C.byref(n)) == capi.CAPACITY
        assert n.value == res.n_out and L.cm_last_error(ctx) and not corr["idx"].any()
        assert L.cm_align_correspondences_copy(ctx, corr.ctypes.data, res.n_out, C.byref(n)) == capi.OK
        assert (corr["idx"] == np.arange(res.n_out)).all()
        tiny = MergeParams(leaf=(1e-4,) * 3, min_points_per_voxel=0)
        res = run_frame(cm, sensors, tiny)
        assert res.status == capi.GRID_OVERFLOW                            # no voxel grid
        refused(cm, src)
        assert L.cm_align_correspondences_copy(ctx, corr.ctypes.data, len(corr), C.byref(n)) == capi.BAD_ARG   # a merge since
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
        assert cm.align(cm.result(res.n_out), 0.5, max_iterations=0).sse == 0
