"""The covariance table byte for byte: cm_result_voxel_cov / cm_result_voxel_cov_device against the kernel-order restatement
(tests/voxel_cov_exact.py) on designed frames (tests/cov_edge_frames.py) — the whole 80-byte entries, no voxel and no
field left out. test_voxel_cov.py keeps its eigh comparison within tolerances beside this, as the independent cross-check;
it has to look away at the zero-eigenvalue boundary, which is where these frames live.

Guards first: what the frames are built to contain is asserted without a GPU on the frames themselves, and again on the
GPU on the library's own merged cloud, cells and counts before any table is compared. The routes are not forced here (the
large-frame tests and test_edge_values cover them); path_flags is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import XYZI_DTYPE
from tests import cov_edge_frames as cf
from tests import voxel_cov_exact as vx
from tests import voxel_cov_ref as vr

LEAF = cf.LEAF
SORT_TILE = 4096                    # CM_TILE, cm_device.h
RADIX_BITS = 8                      # CM_RADIX_BITS
N_OUTS = (1, 2, 255, 256, 257, 65536, 65537)
V, I = capi.COV_VALID, capi.COV_INFLATED


@functools.lru_cache(maxsize=None)
def designed():
    return cf.designed_frame()


def as_merged(xyz):
    m = np.zeros(len(xyz), XYZI_DTYPE)
    m["x"], m["y"], m["z"], m["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0
    return m


def sort_passes(n_out):
    """8-bit passes of the pair sort: key_width(n_out) = bits of n_out - 1, at least 1 (cm_route.cpp), 8 bits a pass"""
    bits = max(1, int(n_out - 1).bit_length())
    return (bits + RADIX_BITS - 1) // RADIX_BITS


def classes(table, info):
    """voxel masks of the flag classes, from the exact table and its kernel-order eigenvalues"""
    big, l, fl = info["big"], info["lam"], table["flags"]
    neg = big & ((l[:, 0] < 0) | (l[:, 1] < 0))
    return {"below min_points": ~big & (fl == 0),
            "invalid, lambda_2 == 0": big & (l[:, 2] == 0) & (fl == 0),
            "invalid, a negative eigenvalue": neg & (fl == 0),
            "VALID": fl == V,
            "VALID|INFLATED, lambda_0 raised": (fl == (V | I)) & (info["raised"] == 1),
            "VALID|INFLATED, both raised": (fl == (V | I)) & (info["raised"] == 2),
            "INFLATED alone": fl == I,
            "valid eigenvalues, no finite inverse": info["eig_ok"] & ((fl & V) == 0)}


def families(fr, mask):
    out = {}
    for k in np.nonzero(mask)[0]:
        f = fr.probes[k]["family"]
        out[f] = out.get(f, 0) + 1
    return out


def designed_tables(min_points, eig_mult):
    fr = designed()
    return vx.voxel_cov(as_merged(fr.merged_xyz()), fr.cells(), fr.counts(), LEAF, min_points, eig_mult)


# ---- CPU: the guards ----------------------------------------------------------------------------------------------------
def test_pass_counts_of_the_lattice_sizes():
    assert [sort_passes(n) for n in N_OUTS] == [1, 1, 1, 1, 2, 2, 3]


def test_guard_every_probe_is_alone_in_its_voxel():
    fr = designed()
    fr.check_cells()
    assert len({p["cell"] for p in fr.probes}) == len(fr.probes)
    assert fr.n_points() <= 4000 and len(fr.sensors()) == 2
    # the restatement finds the frame's voxels from the merged cloud by the cell rule: its counts are the frame's
    t, _ = designed_tables(6, 0.01)
    assert np.array_equal(t["count"], fr.counts())
    # the points of a probe lie in both sensors
    assert np.array_equal(np.bincount(fr.merged_vox()), fr.counts())
    want = {"identical", "col_axis", "col_diag", "col_gen", "plane_axis", "plane_tilt", "two_points", "blob", "cube", "sym3",
            "thin1", "thin2", "minpts", "single", "wide", "wide_line"}
    assert {p["family"] for p in fr.probes} == want
    sites = {(p["family"], p["site"]) for p in fr.probes}
    assert all(("blob", s) in sites for s in cf.SITES)
    print(f"designed frame: {len(fr.probes)} voxels, {fr.n_points()} points")


def test_guard_every_flag_class_is_in_the_frame():
    fr = designed()
    t, info = designed_tables(6, 0.01)
    cl = classes(t, info)
    for name, mask in cl.items():
        print(f"(6, 0.01) {name}: {int(mask.sum())} {families(fr, mask)}")
    for name in ("below min_points", "invalid, lambda_2 == 0", "invalid, a negative eigenvalue", "VALID",
                 "VALID|INFLATED, lambda_0 raised", "VALID|INFLATED, both raised"):
        assert cl[name].sum() >= 3, name
    assert cl["INFLATED alone"].sum() == 0 and cl["valid eigenvalues, no finite inverse"].sum() == 0
    assert sum(int(m.sum()) for k, m in cl.items() if k != "valid eigenvalues, no finite inverse") == len(fr.probes)
    # without inflation: valid eigenvalues whose inverse is not finite (INFLATED alone is unreachable: voxel_cov_exact.py)
    t0, info0 = designed_tables(6, 0.0)
    cl0 = classes(t0, info0)
    print(f"(6, 0.0) valid eigenvalues, no finite inverse: {int(cl0['valid eigenvalues, no finite inverse'].sum())} "
          f"{families(fr, cl0['valid eigenvalues, no finite inverse'])}")
    assert cl0["valid eigenvalues, no finite inverse"].sum() >= 3 and not (t0["flags"] & I).any()
    # eig_mult 1 raises everything that is valid and not isotropic; min_points 20 leaves count and mean only
    t1, info1 = designed_tables(6, 1.0)
    assert ((t1["flags"] == V) == (info1["eig_ok"] & (info1["lam"][:, 0] == info1["lam"][:, 2]))).all() and (t1["flags"] == V).any()
    t20, info20 = designed_tables(20, 0.01)
    assert not info20["big"].any() and not t20["flags"].any() and not t20["cov"].any()
    # the min_points edge: the same geometry at min_points - 1, min_points, min_points + 1
    for mp in (3, 6):
        tm, _ = designed_tables(mp, 0.01)
        cnt = sorted(int(tm["count"][k]) for k, p in enumerate(fr.probes) if p["family"] == "minpts" and p["site"] == "p60")
        assert cnt == [2, 3, 4, 5, 6, 7]
        for k, p in enumerate(fr.probes):
            if p["family"] == "minpts":
                assert bool(tm["cov"][k].any()) == (tm["count"][k] >= mp)


def test_guard_the_frame_lives_where_the_eigh_comparison_looks_away():
    fr = designed()
    for mp, em in ((6, 0.01), (3, 0.01)):
        a, info = designed_tables(mp, em)
        b, lam = vr.voxel_cov(as_merged(fr.merged_xyz()), fr.cells(), fr.counts(), LEAF, mp, em)
        l2 = np.abs(lam[:, 2])
        near = info["big"] & ((np.abs(lam[:, 0]) <= 1e-12 * l2) | (np.abs(lam[:, 1]) <= 1e-12 * l2))     # check_table's rule
        differ = info["big"] & ((a["flags"] & V) != (b["flags"] & V))
        print(f"({mp}, {em}) inside check_table's excluded boundary: {int(near.sum())} {families(fr, near)}")
        print(f"({mp}, {em}) VALID differs between kernel order and eigh: {int(differ.sum())} {families(fr, differ)}")
        assert near.sum() >= 20 and differ.sum() >= 3
        # ... and away from the boundary the two restatements agree, as they do in test_voxel_cov_exact.py
        far = info["big"] & (lam[:, 0] > 1e-9 * l2)
        assert far.sum() >= 50 and np.array_equal(a["flags"][far], b["flags"][far])


def test_guard_order_sweeps_and_ties_decide_bytes():
    fr = designed()
    xyz, vox, n = fr.merged_xyz(), fr.merged_vox(), len(fr.probes)
    t, info = vx.voxel_stats(xyz, vox, n, 6, 0.01)
    rev, _ = vx.voxel_stats(xyz[::-1], vox[::-1], n, 6, 0.01)
    order = cf.rows_differ(t["cov"].copy(), rev["cov"].copy())
    d = info["diag"]
    ties = info["big"] & ((d[:, 0] == d[:, 1]) | (d[:, 1] == d[:, 2]) | (d[:, 0] == d[:, 2]))
    sweep = cf.rows_differ(t, vx.voxel_stats(xyz, vox, n, 6, 0.01, sweeps=11)[0])
    t1 = vx.voxel_stats(xyz, vox, n, 6, 1.0)[0]
    tie_rule = cf.rows_differ(t1, vx.voxel_stats(xyz, vox, n, 6, 1.0, strict=False)[0])
    print(f"cov changes when the points are summed in reverse: {int(order.sum())} {families(fr, order)}")
    print(f"two exactly equal eigenvalues after jacobi3: {int(ties.sum())} {families(fr, ties)}")
    print(f"the twelfth sweep changes the table: {int(sweep.sum())} {families(fr, sweep)}")
    print(f"the tie rule of the sort changes the table at eig_mult 1: {int(tie_rule.sum())} {families(fr, tie_rule)}")
    assert order.sum() >= 1 and ties.sum() >= 1 and sweep.sum() >= 1 and tie_rule.sum() >= 1
    assert families(fr, ties & tie_rule).get("sym3", 0) >= 1 and families(fr, ties).get("cube", 0) >= 1


def test_guard_lattices_and_long_runs():
    for n_out in (1, 2, 257):
        fr = cf.lattice_frame(n_out)
        cnt = fr.counts()
        assert len(fr.cells()) == n_out and cnt.min() >= 1 and cnt.max() <= 8 and fr.n_points() == cnt.sum()
        t, _ = vx.voxel_cov(as_merged(fr.merged_xyz()), fr.cells(), cnt, LEAF, 3, 0.01)
        assert np.array_equal(t["count"], cnt)
    fr = cf.long_run_frame(5000, 300)
    cnt = fr.counts()
    start = int(cnt[:150].sum())
    assert cnt[150] == 5000 and 0 < start % SORT_TILE and start // SORT_TILE != (start + 4999) // SORT_TILE
    assert cf.long_run_frame(10_000, 0).counts().tolist() == [10_000]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def hip_rt():
    try:
        return C.CDLL("libamdhip64.so.7")
    except OSError:
        return C.CDLL("/opt/rocm/lib/libamdhip64.so")


def run_frame(cm, fr, min_points_per_voxel=0):
    cm.submit_all(fr.sensors())
    res = cm.merge_voxelize(fr.params(min_points_per_voxel))
    assert res.status == capi.OK
    print(f"n_out {res.n_out} path_flags {res.path_flags:#x}")
    return res


def library_frame(cm, res, fr, min_points_per_voxel=0):
    """The guards again, on what the library made of the frame: its merged cloud is the frame's bit for bit and in order; its
    voxels are the frame's (those that min_points_per_voxel keeps), each with the frame's count. Returns (merged, cells,
    counts, probe): probe[k] is the frame's voxel number of result voxel k."""
    merged = cm.merged(fr.n_points())
    xyz = np.stack([merged["x"], merged["y"], merged["z"]], axis=1).astype(np.float32)
    assert xyz.shape == fr.merged_xyz().shape and np.array_equal(xyz.view(np.uint32), fr.merged_xyz().view(np.uint32))
    cells, counts = cm.cells(res.n_out)
    keep = np.nonzero(fr.counts() >= max(min_points_per_voxel, 1))[0]
    assert res.n_out == len(keep)
    want_key = vr.cell_keys(fr.cells()[keep])
    order = np.argsort(want_key)
    got_key = vr.cell_keys(cells)
    pos = np.searchsorted(want_key[order], got_key)
    assert len(np.unique(got_key)) == len(got_key) and (want_key[order][np.minimum(pos, len(keep) - 1)] == got_key).all()
    probe = keep[order[pos]]
    assert np.array_equal(counts, fr.counts()[probe])
    return merged, cells, counts, probe


def assert_same_bytes(got, want, fr, probe, label):
    d = vx.first_difference(got, want)
    if d is None:
        return
    k, field, g, w = d
    where = ""
    if k >= 0:
        p = getattr(fr, "probes", None)
        fam = f"family {p[probe[k]]['family']} at {p[probe[k]]['site']}, " if p else ""
        n_bad = int(cf.rows_differ(got, want).sum())
        where = f"{n_bad} of {len(want)} entries differ; first: voxel {k} ({fam}count {want['count'][k]}), "
    raise AssertionError(f"{label}: {where}field {field}: got {g!r} want {w!r}")


def exact(cm, res, fr, lib, min_points, eig_mult, hip):
    """Both entry points against the restatement, every byte."""
    merged, cells, counts, probe = lib
    want, info = vx.voxel_cov(merged, cells, counts, LEAF, min_points, eig_mult)
    got = cm.voxel_covariance(res.n_out, min_points, eig_mult)
    assert_same_bytes(got, want, fr, probe, f"cm_result_voxel_cov ({min_points}, {eig_mult})")
    ptr, n = cm.voxel_covariance_device(min_points, eig_mult)
    assert n == res.n_out and ptr
    dev = np.zeros(n, dtype=capi.VOXEL_COV_DTYPE)
    assert hip.hipMemcpy(C.c_void_p(dev.ctypes.data), C.c_void_p(ptr), C.c_size_t(n * 80), 2) == 0
    assert_same_bytes(dev, want, fr, probe, f"cm_result_voxel_cov_device ({min_points}, {eig_mult})")
    return want, info


def context(fr):
    return capi.CloudMerger(max_points_total=fr.n_points(), max_sensors=len(fr.sensors()), flags=capi.FLAG_OCCUPANCY)


@pytest.mark.gpu
def test_designed_frame_at_every_parameter_set():
    fr, hip = designed(), hip_rt()
    with context(fr) as cm:
        res = run_frame(cm, fr)
        lib = library_frame(cm, res, fr)
        for mp, em in cf.PARAM_SETS:
            want, info = exact(cm, res, fr, lib, mp, em, hip)
            print(f"({mp}, {em}): " + ", ".join(f"{k} {int(m.sum())}" for k, m in classes(want, info).items()))
            if (mp, em) == (6, 0.01):
                cl = classes(want, info)
                assert all(cl[k].sum() >= 3 for k in ("below min_points", "invalid, lambda_2 == 0", "invalid, a negative eigenvalue",
                                                      "VALID", "VALID|INFLATED, lambda_0 raised", "VALID|INFLATED, both raised"))


@pytest.mark.gpu
@pytest.mark.parametrize("mppv", [2, 6])
def test_designed_frame_with_dropped_voxels(mppv):
    """min_points_per_voxel drops voxels that lie between kept ones: their records leave the pair sort in pass 0 and the
    table is numbered by the kept voxels."""
    fr, hip = designed(), hip_rt()
    with context(fr) as cm:
        res = run_frame(cm, fr, mppv)
        lib = library_frame(cm, res, fr, mppv)
        dropped = fr.counts() < mppv
        key = vr.cell_keys(fr.cells())
        kept_keys = np.sort(key[~dropped])
        between = (key[dropped] > kept_keys[0]) & (key[dropped] < kept_keys[-1])
        print(f"min_points_per_voxel {mppv}: {int(dropped.sum())} voxels dropped, {int(between.sum())} between kept ones")
        assert between.sum() >= 3 and res.n_out == (~dropped).sum()
        for mp, em in ((6, 0.01), (3, 0.01)):
            exact(cm, res, fr, lib, mp, em, hip)


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", N_OUTS)
def test_every_pass_count_of_the_pair_sort(n_out):
    """The pair sort takes ceil(bits(n_out - 1) / 8) passes and k_cov_reduce reads buffer B after an odd number of them:
    one pass (odd), two (even), three (odd), and the sizes either side of each step."""
    passes = sort_passes(n_out)
    assert passes == {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65536: 2, 65537: 3}[n_out]
    fr, hip = cf.lattice_frame(n_out), hip_rt()
    assert fr.n_points() <= 300_000
    with context(fr) as cm:
        res = run_frame(cm, fr)
        assert res.n_out == n_out
        lib = library_frame(cm, res, fr)
        print(f"n_out {n_out}: {fr.n_points()} points, {passes} passes, buffer {'B' if passes & 1 else 'A'}")
        want, _ = exact(cm, res, fr, lib, 3, 0.01, hip)
        if n_out >= 255:
            assert (want["flags"] == V).sum() > n_out // 4 and (want["flags"] == 0).sum() > n_out // 8


@pytest.mark.gpu
@pytest.mark.parametrize("n_long,n_small", [(10_000, 0), (5000, 300)])
def test_runs_longer_than_a_sort_tile(n_long, n_small):
    fr, hip = cf.long_run_frame(n_long, n_small), hip_rt()
    with context(fr) as cm:
        res = run_frame(cm, fr)
        lib = library_frame(cm, res, fr)
        counts = lib[2]
        k = int(np.argmax(counts))
        start = int(counts[:k].sum())
        print(f"the run of {counts[k]} records starts at sorted record {start}")
        assert counts[k] == n_long > SORT_TILE
        if n_small:
            assert 0 < start % SORT_TILE and start // SORT_TILE != (start + n_long - 1) // SORT_TILE
        want, info = exact(cm, res, fr, lib, 6, 0.01, hip)
        assert want["flags"][k] == V and info["lam"][k, 0] > 0.1 * info["lam"][k, 2]      # generic: far from zero


@pytest.mark.gpu
def test_second_request_and_next_frame_are_exact():
    """A request, another at other parameters on the same result, then a new frame and the first parameters again: the
    cached table (cov_have, cov_min_points, cov_eig_mult: what ndt() reuses) never outlives its parameters or its frame."""
    fr, other, hip = designed(), cf.lattice_frame(257), hip_rt()
    with context(fr) as cm:
        res = run_frame(cm, fr)
        lib = library_frame(cm, res, fr)
        a, _ = exact(cm, res, fr, lib, 6, 0.01, hip)
        b, _ = exact(cm, res, fr, lib, 3, 0.05, hip)
        assert a.tobytes() != b.tobytes()
        exact(cm, res, fr, lib, 6, 0.01, hip)
        res = run_frame(cm, other)
        lib = library_frame(cm, res, other)
        exact(cm, res, other, lib, 6, 0.01, hip)
