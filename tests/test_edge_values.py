"""Special values and cell-face geometry on every voxel route (tests/edge_frames.py builds the frames).

Each frame is a seeded background plus probe voxels with expectations of their own (exact-rational quotients). Every
route runs the frame through the C-ABI and is held to the oracle (stable order) and to the probes:
  merged cloud   bit-exact, NaN payloads in intensity included (it is a copy)
  occupancy      cells, counts and order exact; min_b / div_b when the bounds do not come from the crop box
  centroids      finite: bit for bit (sign of zero included) for voxels of up to SEQ_EXACT_MAX points on the k3 finish,
                 every voxel on the k2_local finish, voxels of up to 2 points on the general path; the tolerance rules of
                 tests/util.py otherwise. Non-finite: the same class (nan / +inf / -inf) on every route and size.
The route each case asks for is asserted through path_flags. On the outlier route (family h: pairs at exactly, one ulp
below and one ulp above the radius) the probes that survive the filter are worked out by brute force in fp32 and
checked point for point in the merged cloud. The fused route (two contexts as ranks, cm_merge_partial +
cm_merge_tables) adds a voxel's partial sums per rank: its centroids are bit-exact where every order gives the same
sum (voxels of up to 2 points, subnormal and zero sums)."""
import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from oracle import oracle
from tests import edge_frames as ef
from cloud_merger_amd import fused, synth
from tests.test_voxel_cov import check_table
from tests.util import SEQ_EXACT_MAX, assert_centroids_close, same_bits, xyzi_of

pytestmark = pytest.mark.gpu

LDS_RANK, BUCKET, PREDICTED, REDONE, SPLIT, QUANTILE = 1, 2, 4, 8, 32, 64

# route -> (environment, crop box on, frames on one context, what path_flags of the last frame must show)
ROUTES = {
    "general": (dict(CM_PATH="classic"), True, 1),
    "fixed": (dict(CM_QUANT="0"), True, 2),
    "predicted": ({}, False, 2),
    "quantile": ({}, True, 2),
    "k2_local": (dict(CM_FINISH="v2"), True, 2),
    "ballot": (dict(CM_LDS_RANK="0"), True, 2),
    "outlier": ({}, True, 2),
}


def xyzi4(a):
    return np.stack([a["x"], a["y"], a["z"], a["intensity"]], axis=1)


def check_route(route, res):
    f = res.path_flags
    if route == "general":
        assert not f & BUCKET, f
        return
    if route != "ballot" and not f & LDS_RANK:
        pytest.skip("the device probe did not find lane-ordered LDS adds: no bucket path on this device")
    assert f & BUCKET and not f & REDONE, f
    if route == "fixed":
        assert not f & (PREDICTED | QUANTILE), f
    elif route == "predicted":
        assert f & PREDICTED, f
    elif route == "quantile":
        assert f & QUANTILE, f
    elif route == "k2_local":
        assert not f & SPLIT, f
    elif route == "ballot":
        assert not f & LDS_RANK, f


def background_cells(sensors, leaf):
    """the cells of the background clouds after their transforms (the oracle's transform: placement only)"""
    out = set()
    for s in sensors:
        pts = oracle.make_points(np.stack([s.data["x"], s.data["y"], s.data["z"]], axis=1))
        w = oracle.transform(pts, oracle.quat_to_matrix(s.q_xyzw, s.t_xyz))
        out |= set(map(tuple, np.unique(oracle.voxel_cells(w, leaf), axis=0).tolist()))
    return out


def probe_cells_alone(frame, params):
    """no background point shares a voxel with a probe"""
    probe = set(frame.probes.expect(params.crop_min, params.crop_max))
    assert not probe & background_cells(frame.sensors[:-frame.n_probe], params.leaf)


def compare(route, frame, params, res, got_merged, got, cells, counts):
    st, merged, out, rep = oracle.merge_voxelize(frame.sensors, params, threads=4, stable=True)
    assert res.status == st == capi.OK
    assert same_bits(got_merged, xyzi_of(merged)), "merged cloud (with NaN payloads) must be bit-exact"
    mp = frame.merged_probes(params)                               # the probe points that survive, in order, last
    want_tail = np.array([w for w, _ in mp], np.float32).reshape(-1, 4)
    assert same_bits(got_merged[len(got_merged) - len(mp):], want_tail), "probe points of the merged cloud"
    if frame.outlier(params):
        assert res.n_merged < res.n_in and res.n_merged == rep.n_merged
    assert res.n_out == rep.n_out and np.array_equal(cells, rep.cells) and np.array_equal(counts, rep.counts)
    if not res.bounds_from_crop:
        assert list(res.min_b) == list(rep.min_b) and list(res.div_b) == list(rep.div_b)
    want = xyzi_of(out)
    fin = np.isfinite(want)
    gcls = np.vectorize(ef.cls)(got)
    wcls = np.vectorize(ef.cls)(want)
    assert np.array_equal(gcls, wcls), "non-finite centroid values: same class as the oracle"
    finite_rows = fin.all(axis=1)
    if res.path_flags & BUCKET and not res.path_flags & SPLIT:
        exact = np.ones(len(counts), bool)                       # k2_local: every voxel in the oracle's order
    elif res.path_flags & BUCKET:
        exact = counts <= SEQ_EXACT_MAX
    else:
        exact = counts <= 2
    e = exact[:, None] & fin
    diff = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & e)
    assert not len(diff[0]), (f"{route}: finite centroids of short voxels must be bit-exact; first differences (voxel, "
                              f"axis, count, got, want): " + ", ".join(
                                  f"({k}, {a}, {counts[k]}, {got.view(np.uint32)[k, a]:#010x}, "
                                  f"{want.view(np.uint32)[k, a]:#010x})" for k, a in zip(*[d[:6] for d in diff])))
    loose = ~exact & finite_rows
    assert_centroids_close(got[loose], want[loose])
    # the probes: their own exact-rational expectation, for the oracle and for the device
    exp = frame.expect(params)
    where = {tuple(c): k for k, c in enumerate(rep.cells.tolist())}
    below = set(frame.probes.expect(params.crop_min, params.crop_max, frame.outlier(params))) - set(exp)
    assert not below & set(where), "probe voxels below min_points_per_voxel are not kept"
    seen = 0
    for cell, v in exp.items():
        k = where.get(cell)
        assert k is not None, (cell, v)
        assert counts[k] == v["count"], (cell, v["count"], counts[k])
        ref = v["centroid"]
        for a in range(4):
            if ef.cls(ref[a]) != "finite":
                assert ef.cls(want[k, a]) == ef.cls(got[k, a]) == ef.cls(ref[a]), (cell, a, v["family"])
            else:
                assert ef.bits_of(want[k, a]) == ef.bits_of(ref[a]), \
                    f"oracle vs exact-rational reference: probe {v['family']} cell {cell} axis {a}"
                if exact[k]:
                    assert ef.bits_of(got[k, a]) == ef.bits_of(ref[a]), \
                        (f"{route}: probe {v['family']} at cell {cell}, {v['count']} points, axis {a}: "
                         f"got {ef.bits_of(got[k, a]):#010x}, want {ef.bits_of(ref[a]):#010x}")
        seen += 1
    assert seen == len(exp)
    return rep


def run_route(route, frame, monkeypatch, params=None):
    env, crop, n_frames = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = params or frame.with_crop(crop)
    probe_cells_alone(frame, params)
    n_cap = sum(s.n for s in frame.sensors)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(frame.sensors), flags=capi.FLAG_OCCUPANCY) as cm:
        for _ in range(n_frames):
            cm.submit_all(frame.sensors)
            res = cm.merge_voxelize(params)
            assert res.status == capi.OK, capi.status_string(res.status)
            got_merged = xyzi4(cm.merged(n_cap))
            got = xyzi4(cm.result(res.n_out))
            cells, counts = cm.cells(res.n_out)
            compare(route, frame, params, res, got_merged, got, cells, counts)
        check_route(route, res)
        if frame.name.startswith("faces_"):
            check_table(cm, res, params.leaf, n_cap, min_points=3)     # k_cov_keys recomputes every point's cell
    return res


_FRAMES = {}


def frame_of(name):
    if name not in _FRAMES:
        if name == "values":
            _FRAMES[name] = ef.value_frame()
        elif name.startswith("faces_"):
            _FRAMES[name] = ef.face_frame(name[len("faces_"):])
        elif name == "outliers":
            _FRAMES[name] = ef.outlier_frame()
        else:
            _FRAMES[name] = ef.key_width_frame(int(name.split("_")[-1]))
    return _FRAMES[name]


def test_probe_transform_keeps_the_sign_of_zero():
    m = oracle.quat_to_matrix(ef.IDENT_Q, ef.PROBE_T)
    assert same_bits(m.reshape(-1), np.array([1, 0, 0, -0.0, 0, 1, 0, -0.0, 0, 0, 1, -0.0], np.float32))
    assert ef.bits_of(ef.xf_ident((-0.0, -0.0, -0.0))[0]) == 0x80000000
    assert ef.bits_of(ef.xf_ident((-0.0, 1.0, 1.0))[0]) == 0


@pytest.mark.parametrize("route", [r for r in ROUTES if r != "outlier"])
def test_special_values(route, monkeypatch):
    """families a-e (subnormal, signed-zero, non-finite and overflowing values) and crop faces at 5 cm"""
    run_route(route, frame_of("values"), monkeypatch)


@pytest.mark.parametrize("key", list(ef.FACE_LEAVES))
@pytest.mark.parametrize("route", ["general", "fixed", "predicted", "quantile", "k2_local"])
def test_cell_faces(key, route, monkeypatch):
    """family f: points on voxel faces and 1-2 ulps beside them up to 2 km out, on crop faces"""
    run_route(route, frame_of("faces_" + key), monkeypatch)


@pytest.mark.parametrize("kb", sorted(ef.KEY_WIDTHS))
def test_key_widths_first_and_last_cell(kb, monkeypatch):
    """family g: boxes of 2^kb cells, probes in the first and the last cell (fixed grid, then the frame after it)"""
    frame = frame_of(f"key_bits_{kb}")
    monkeypatch.setenv("CM_QUANT", "0")
    res = run_route("fixed", frame, monkeypatch)
    assert res.key_bits == kb


def test_outlier_pairs_at_the_radius(monkeypatch):
    """family h on the bucket path behind the outlier pre-stage: pairs whose fp32 d2 is r2 exactly (both points dropped),
    one ulp below (kept) and one ulp above (dropped), along axes and diagonals, across faces of the radius grid and
    x = 0, near the origin and 1 km out"""
    frame = frame_of("outliers")
    tags = [t for _, t in frame.merged_probes(frame.params)]
    assert 0 < tags.count("h") < sum(t == "h" for t in frame.probes.tags)
    run_route("outlier", frame, monkeypatch, params=frame.params)


def fused_exact(v, a):
    """the fused route's sum of a probe voxel's values on axis a is the same in every order"""
    vals = [float(p[a]) for p in v["pts"]]
    return v["count"] <= 2 or (all(abs(x) < ef.FLT_MIN for x in vals) and abs(sum(vals)) < ef.FLT_MIN)


def test_fused_two_ranks(monkeypatch):
    """families a-e through cm_merge_partial on two contexts (ranks: sensors dealt s % 2, so every probe voxel's points
    come from both) and cm_merge_tables: occupancy exact, non-finite classes, -0.0 sums as +0.0, exact subnormal
    quotients; the rest within the tolerance"""
    frame = frame_of("values")
    params = frame.params
    sensors = frame.sensors
    world = 2
    n_total = sum(s.n for s in sensors)
    cms, parts = [], []
    try:
        for r in range(world):
            cm = capi.CloudMerger(max_points_total=n_total, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY)
            cms.append(cm)
            for k, s in enumerate(fused.shard_sensors(len(sensors), r, world)):
                cm.set_transform(k, sensors[s].q_xyzw, sensors[s].t_xyz)
                cm.submit(k, sensors[s])
        for cm in cms:
            res = cm.merge_partial(params, None)
            assert res.status == capi.OK
            if res.path_flags & LDS_RANK:
                assert res.path_flags & BUCKET, res.path_flags
            parts.append(cm.partial_device())
        res = cms[0].merge_tables([p[0] for p in parts], [p[1] for p in parts], params)
        assert res.status == capi.OK
        got = xyzi4(cms[0].result(res.n_out))
        cells, counts = cms[0].cells(res.n_out)
    finally:
        for cm in cms:
            cm.close()
    st, _, out, rep = oracle.merge_voxelize(sensors, params, threads=4, stable=True)
    assert st == oracle.OK and res.n_out == rep.n_out
    assert np.array_equal(cells, rep.cells) and np.array_equal(counts, rep.counts)
    want = xyzi_of(out)
    assert np.array_equal(np.vectorize(ef.cls)(got), np.vectorize(ef.cls)(want)), "non-finite classes"
    fin = np.isfinite(want).all(axis=1)
    assert_centroids_close(got[fin], want[fin])
    where = {tuple(c): k for k, c in enumerate(rep.cells.tolist())}
    n_exact = 0
    for cell, v in frame.expect(params).items():
        k = where[cell]
        for a in range(4):
            ref = v["centroid"][a]
            if ef.cls(ref) != "finite":
                assert ef.cls(got[k, a]) == ef.cls(ref), (cell, a, v["family"])
            elif fused_exact(v, a):
                n_exact += 1
                assert ef.bits_of(got[k, a]) == ef.bits_of(ref), \
                    (f"fused: probe {v['family']} at cell {cell}, {v['count']} points, axis {a}: "
                     f"got {ef.bits_of(got[k, a]):#010x}, want {ef.bits_of(ref):#010x}")
    assert n_exact >= 50


def test_shared_bins_dense_frame():
    """the value probes in cfg3's dense frame (8 x 1 M points): from the third frame on one global pass over bins that
    two buckets share (sort_passes == 1, CM_PATH_QUANTILE)"""
    base, params = synth.config3_dense(n_per_sensor=1_000_000, min_pts=2)
    frame = ef.shared_bin_frame(base, params, background_cells(base, params.leaf))
    assert len(frame.expect(params)) >= 40
    sensors = frame.sensors
    n = sum(s.n for s in sensors)
    with capi.CloudMerger(max_points_total=n, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY) as cm:
        seen = []
        for _ in range(3):
            cm.submit_all(sensors)
            res = cm.merge_voxelize(params)
            assert res.status == capi.OK
            got_merged = xyzi4(cm.merged(n))
            got = xyzi4(cm.result(res.n_out))
            cells, counts = cm.cells(res.n_out)
            seen.append((res.sort_passes, res.path_flags))
            if not res.path_flags & LDS_RANK:
                pytest.skip("the device probe did not find lane-ordered LDS adds: no bucket path on this device")
        compare("shared_bins", frame, params, res, got_merged, got, cells, counts)
    assert seen[2][0] == 1 and seen[2][1] & QUANTILE and seen[2][1] & BUCKET and not seen[2][1] & REDONE, seen
