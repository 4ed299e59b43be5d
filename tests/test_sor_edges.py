"""Statistical outlier removal at special values and grid extremes (tests/sor_edge_frames.py; cm_kernels_sor.hip).

Every probe frame is judged by the brute-force restatement (sor_ref.knn_d2_brute: every pair, no cells): d_i bits, n_valid,
n_removed, mean, stddev and threshold bit for bit, the survivors' bytes equal to the masked input, PATH_SOR, and the voxel
result equal to a stage-off run on the survivors (test_sor.check_frame). On the general route (CM_PATH=classic) without a
crop box, and where the probe has one, with the box on the general route and on the fixed-grid route (CM_QUANT=0). Search
cells of 0, 1e-6, the family's own and 1e3 m leave every byte unchanged. On the CPU: the bucketed restatement equals the
brute force on every probe, the hand derivations hold, and S and Q equal exact rational sums rounded once."""
import math
from fractions import Fraction

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from tests import sor_edge_frames as ef
from tests import sor_ref as sr
from tests.test_sor import check_frame, run_sor, xyz_of

PROBES = ef.probes()
IDS = [p.name for p in PROBES]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def reference(p):
    return sr.sor(p.xyz, p.k, p.std_mul, brute=True)


# ---- CPU: the references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [p for p in PROBES if len(p.xyz) > p.k], ids=lambda p: p.name)
def test_bucketed_search_equals_brute_force(p):
    """(frames of n <= k have no neighbours to search: their expectation is the hand derivation)"""
    want = sr.knn_d2_brute(p.xyz, p.k)
    cell = next((c for c in p.cells if c > 0), None)
    with np.errstate(over="ignore", invalid="ignore"):
        got = sr.knn_d2(p.xyz, p.k, cell)
        got_auto = sr.knn_d2(p.xyz, p.k) if len(p.xyz) <= 2000 else got
    assert bits(got) == bits(want) and bits(got_auto) == bits(want)


@pytest.mark.parametrize("p", [p for p in PROBES if p.expect_d is not None], ids=lambda p: p.name)
def test_hand_derivations(p):
    d, (mean, sd, thr), keep = reference(p)
    assert bits(d) == bits(p.expect_d)
    assert int((~keep).sum()) == p.expect_removed


def test_threshold_is_one_d_exactly():
    p = next(q for q in PROBES if q.name == "h_threshold_is_a_d")
    d, (mean, sd, thr), keep = reference(p)
    assert mean == 2.0 and thr == 2.0 and sum(d == 2.0) == 8 and keep[d == 2.0].all() and not keep[d == 3.0].any()


def test_all_equal_threshold_is_the_mean():
    p = next(q for q in PROBES if q.name == "h_all_equal")
    d, (mean, sd, thr), keep = reference(p)
    assert (mean, sd, thr) == (1.0, 0.0, 1.0) and keep.all()


def test_every_probe_input_is_finite_and_placed():
    for p in PROBES:
        assert np.isfinite(p.xyz).all(), p.name
    names = {p.name for p in PROBES}
    # the probes the margin mutations need exist (the ulp searches found their configurations)
    assert any(n.startswith("b_thin_") for n in names) and any(n.startswith("b_ring_") for n in names)
    for p in PROBES:
        if p.name.startswith(("b_thin_", "b_ring_")):
            # q (the point the search must not miss) is p's nearest, r (the decoy) the next
            d2 = sr.knn_d2_brute(p.xyz[:3], 2)
            q2 = sr._d2(p.xyz[0], p.xyz[1])
            assert d2[0, 0] == q2 and d2[0, 1] > q2, p.name


@pytest.mark.parametrize("p", [p for p in PROBES if len(p.xyz) <= 3000 and len(p.xyz) > p.k], ids=lambda p: p.name)
def test_sums_are_exact_rationals_rounded_once(p):
    d, (mean, sd, thr), _ = reference(p)
    S, Q = sr.exact_sums(d)
    n = len(d)
    fs = math.fsum(d.astype(np.float64).tolist())
    with np.errstate(over="ignore"):
        fq = math.fsum((d * d).astype(np.float32).astype(np.float64).tolist())
    if S is None:
        assert fs == math.inf and mean == math.inf
    else:
        assert float(S) == fs and mean == float(S) / n
        assert float(S) == float(Fraction(fs)) and abs(Fraction(fs) - S) <= abs(Fraction(math.nextafter(fs, math.inf)) - S)
    if Q is None:
        assert fq == math.inf
    else:
        assert float(Q) == fq


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, route):
    monkeypatch.delenv("CM_PATH", raising=False)
    monkeypatch.delenv("CM_QUANT", raising=False)
    if route == "classic":
        monkeypatch.setenv("CM_PATH", "classic")
    else:
        monkeypatch.setenv("CM_QUANT", "0")


def _params(p, crop):
    extra = dict(crop_min=crop[0], crop_max=crop[1]) if crop else {}
    return MergeParams(leaf=(p.leaf,) * 3, min_points_per_voxel=1, **extra)


def merged_input(sensors, n_cap, params):
    """The stage's input (test_sor.merged_input), for a frame whose voxel grid may overflow: CM_GRID_OVERFLOW hands the
    merged cloud on unvoxelised."""
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(sensors)) as cm:
        cm.submit_all(sensors)
        res = cm.merge_voxelize(params)
        assert res.status in (capi.OK, capi.EMPTY_INPUT, capi.GRID_OVERFLOW)
        return cm.merged(n_cap)


def _same(a, b):
    res_a, d_a, st_a, m_a, vox_a = a
    res_b, d_b, st_b, m_b, vox_b = b
    assert bits(d_a) == bits(d_b) and m_a.tobytes() == m_b.tobytes()
    assert (vox_a is None) == (vox_b is None) and (vox_a is None or vox_a[0] == vox_b[0])
    for f in ("n_valid", "n_removed", "mean", "stddev", "threshold"):
        x, y = getattr(st_a, f), getattr(st_b, f)
        assert x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)), f


@pytest.mark.gpu
@pytest.mark.parametrize("p", PROBES, ids=IDS)
def test_probe(p, monkeypatch):
    sensors = p.sensors()
    n_cap = len(p.xyz)
    ref = reference(p)
    runs = [("classic", None)] + ([("classic", p.crop), ("fixed", p.crop)] if p.crop else [])
    for route, crop in runs:
        _env(monkeypatch, route)
        params = _params(p, crop)
        P = merged_input(sensors, n_cap, params)
        if crop is None:
            # the stage's input is the raw points, bit for bit and in order
            assert bits(xyz_of(P)) == bits(p.xyz)
            r = ref
        else:
            inside = np.all((p.xyz >= np.float32(crop[0])) & (p.xyz <= np.float32(crop[1])), axis=1)
            assert bits(xyz_of(P)) == bits(p.xyz[inside])
            r = ref if inside.all() else sr.sor(xyz_of(P), p.k, p.std_mul, brute=True)
        cells = p.all_cells() if crop is None else [p.all_cells()[0]]
        first = None
        for c in cells:
            got = run_sor(sensors, n_cap, params, p.k, p.std_mul, cell=c)[0]
            if first is None:
                check_frame(P, got, p.k, p.std_mul, params, n_cap, ref=r)
                first = got
            else:
                _same(first, got)


@pytest.mark.gpu
def test_stream_crossing_k(monkeypatch):
    """One context, one stream whose point count crosses k: n = k - 1, k, k + 1, k + 5, k, 3k; every frame against the
    brute force (n <= k: d_i NaN, threshold +inf, nothing removed)."""
    _env(monkeypatch, "classic")
    rng = np.random.default_rng(12)
    for k in (16, 33):
        sizes = (k - 1, k, k + 1, k + 5, k, 3 * k)
        clouds = [rng.uniform(-2, 2, (n, 3)).astype(np.float32) for n in sizes]
        n_cap = max(sizes)
        params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=1)
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
            cm.set_statistical_outlier(k, 1.0)
            for xyz in clouds:
                probe = ef.Probe("stream", "g", xyz, k)
                cm.submit_all(probe.sensors())
                res = cm.merge_voxelize(params)
                assert res.status == capi.OK
                d, (mean, sd, thr), keep = reference(probe)
                st = cm.sor_stats()
                assert bits(cm.sor_distances(n_cap)) == bits(d) and st.n_valid == len(xyz)
                assert st.n_removed == int((~keep).sum()) and cm.merged(n_cap).tobytes() == probe.sensors()[0].data[keep].tobytes()
                if len(xyz) <= k:
                    assert math.isnan(st.mean) and st.threshold == math.inf


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["inf", "nan", "2^-70", "1e6"])
def test_auto_cell_after_an_extreme_frame(kind, monkeypatch):
    """The frame before a normal scene has a mean distance of +inf, NaN, 2^-70 or 1e6: the automatic cell that follows it
    gives the bytes of a fresh context and of an explicit search cell."""
    _env(monkeypatch, "classic")
    extreme = ef.Probe("x", "i", ef.extreme_frames()[kind], 8)
    normal = ef.Probe("n", "i", ef.local_scene(2500, seed=2), 8)
    n_cap = max(len(extreme.xyz), len(normal.xyz))
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=1)

    def frames(seq, cell=0.0):
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
            cm.set_statistical_outlier(8, 1.0, cell)
            out = []
            for pr in seq:
                cm.submit_all(pr.sensors())
                res = cm.merge_voxelize(params)
                st = cm.sor_stats()
                out.append((res.status, cm.sor_distances(n_cap).tobytes(), cm.merged(n_cap).tobytes(),
                            cm.result(res.n_out).tobytes() if res.status == capi.OK else b"",
                            (st.n_valid, st.n_removed, st.mean.hex(), st.stddev.hex(), st.threshold.hex())))
            return out
    after = frames([extreme, normal])
    d, (mean, sd, thr), keep = reference(extreme)
    assert after[0][1] == d.tobytes()
    if kind == "inf":
        assert mean == math.inf and math.isnan(thr)
    assert after[1] == frames([normal])[0] == frames([normal], 0.5)[0]
