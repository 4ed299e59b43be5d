"""Every wire layout of tests/layouts.py on every route that reads the raw clouds.

The loader a kernel reads a sensor with (cm_common.hpp: XYZI16, PCL32 or the generic one at the caller's offsets) is
picked per sensor by build_frame and, on the bucket routes, per tile. Each case runs the same points in another layout
and is held to two bars:
  the oracle       oracle.merge_voxelize(..., stable=True) on the points as XYZI16 records: merged cloud bit-exact,
                   occupancy exact, centroids by the rules of tests/test_edge_values.py (bit-exact where the route adds in
                   the oracle's order, the tolerance otherwise)
  the xyzi16 run   the same route and frame sequence fed the XYZI16 records (intensity 0 for a layout without the field):
                   merged cloud, cells, counts, every centroid bit, ground cloud and planes identical. Same records in the
                   same order give the same bits on every route, long voxels included; this bar has no tolerance.
Every case asserts the path flags of the route it asked for."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from cloud_merger_amd import capi, fused, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from oracle import oracle
from tests import edge_frames as ef
from tests import layouts as wl
from tests import motion_ref as mr
from tests import test_ground as tg
from tests.test_edge_values import BUCKET, LDS_RANK, QUANTILE, REDONE, ROUTES, SPLIT, check_route, compare, xyzi4
from tests.test_motion import T_REF, V, W, plain_run
from tests.test_motion import run as motion_run
from tests.util import SEQ_EXACT_MAX, assert_centroids_close, assert_centroids_close_or_exact, same_bits, xyzi_of

pytestmark = pytest.mark.gpu

PACKED = capi.PATH_PACKED
LAYOUTS = list(wl.LAYOUTS)
CROP = dict(crop_min=(-11.0, -11.0, -2.5), crop_max=(11.0, 11.0, 2.5))
NARROW = dict(crop_min=(-2.5, -3.0, -1.0), crop_max=(3.0, 2.5, 1.0))     # keeps a few percent: packed from frame 2 on


def clustered(rng, n, half=13.0, blob_max=3000):
    """n points in the sensor frame: 45 % uniform (voxels of 1-2 points at 10 cm), the rest in Gaussian blobs of 1 to
    blob_max points and 1 to 30 cm spread (voxels of 3-17 and of hundreds of points)"""
    nu = int(n * 0.45)
    parts = [rng.uniform(-half, half, (nu, 3)) * (1.0, 1.0, 0.2)]
    left = n - nu
    while left:
        m = min(left, int(rng.integers(1, blob_max)))
        c = rng.uniform(-half * 0.8, half * 0.8, 3) * (1.0, 1.0, 0.15)
        parts.append(c + rng.normal(0.0, rng.uniform(0.01, 0.3), (m, 3)))
        left -= m
    xyz = np.concatenate(parts).astype(np.float32)
    return xyz[rng.permutation(n)]


def make_scene(seed, sizes, blob_max=3000):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        q = synth.yaw_quaternion(rng.uniform(-np.pi, np.pi))
        out.append(xyzi_cloud(clustered(rng, n, blob_max=blob_max), rng.uniform(0, 255, n).astype(np.float32), q_xyzw=q,
                              t_xyz=rng.uniform(-1, 1, 3)))
    return out


SIZES = (50_111, 97_003, 131_077)              # no multiple of 64 or of CM_TILE
_SCENE = {}


def scene():
    if "s" not in _SCENE:
        _SCENE["s"] = make_scene(71, SIZES)
    return _SCENE["s"]


def route_tag(route):
    """routes that run the same parameters share the oracle"""
    return route if route in ("predicted", "packed", "outlier", "ground") else "crop"


def route_params(route):
    p = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **({} if route == "predicted" else CROP))
    if route == "packed":
        p = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **NARROW)
    elif route == "outlier":
        p.outlier_radius, p.outlier_min_neighbors = 0.15, 1
    elif route == "ground":
        p = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **tg.ROI)
    return p


def reference_of(sensors, layouts):
    """the XYZI16 clouds a frame of these layouts must give the results of (intensity 0 where the layout has none)"""
    return [None if s is None else wl.zero_intensity(s) if lay in wl.NO_INTENSITY else s
            for s, lay in zip(sensors, layouts)]


def packed_frames(sensors, layouts, seed):
    rng = np.random.default_rng(seed)
    return [None if s is None else s if lay == "xyzi16" else wl.relayout(s, lay, rng) for s, lay in zip(sensors, layouts)]


def run_stream(frames, params, n_cap, n_slots, ground=None):
    """frames: per frame, one cloud (or None: nothing submitted) per slot, on one fresh context"""
    out = []
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=n_slots, flags=capi.FLAG_OCCUPANCY) as cm:
        if ground is not None:
            cm.set_ground_removal(ground)
        for clouds, p in zip(frames, params if isinstance(params, list) else [params] * len(frames)):
            for s, c in enumerate(clouds):
                if c is not None:
                    cm.set_transform(s, c.q_xyzw, c.t_xyz)
                    cm.submit(s, c)
            res = cm.merge_voxelize(p)
            assert res.status == capi.OK, capi.status_string(res.status)
            g = dict(res=res, flags=res.path_flags, merged=xyzi4(cm.merged(n_cap)), out=xyzi4(cm.result(res.n_out)))
            g["cells"], g["counts"] = cm.cells(res.n_out)
            if ground is not None:
                g["ground"] = xyzi4(cm.ground(n_cap))
                g["planes"] = bytes(cm.ground_planes())
            out.append(g)
    return out


def assert_same_run(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["flags"] == w["flags"], (what, k, g["flags"], w["flags"])
        assert g["res"].n_merged == w["res"].n_merged and g["res"].n_out == w["res"].n_out, (what, k)
        assert same_bits(g["merged"], w["merged"]), f"{what}, frame {k}: merged cloud differs from the xyzi16 run"
        assert np.array_equal(g["cells"], w["cells"]) and np.array_equal(g["counts"], w["counts"]), (what, k)
        assert same_bits(g["out"], w["out"]), f"{what}, frame {k}: centroids differ from the xyzi16 run"
        if "ground" in w:
            assert same_bits(g["ground"], w["ground"]) and g["planes"] == w["planes"], (what, k)


_ORACLE = {}


def oracle_of(key, sensors, params):
    if key not in _ORACLE:
        _ORACLE[key] = oracle.merge_voxelize([s for s in sensors if s is not None], params, threads=4, stable=True)
    return _ORACLE[key]


def check_oracle(g, ref, leaf):
    """the bars of tests/test_edge_values.compare, without probes; voxels of more than 1000 points within 1e-4 m of their
    exact mean (tests/util.py: the oracle's own sequential sum drifts there)"""
    st, merged, out, rep = ref
    res = g["res"]
    assert st == oracle.OK and res.n_merged == rep.n_merged and res.n_out == rep.n_out
    assert same_bits(g["merged"], xyzi_of(merged)), "merged cloud must be bit-exact"
    assert np.array_equal(g["cells"], rep.cells) and np.array_equal(g["counts"], rep.counts), "occupancy"
    if not res.bounds_from_crop:
        assert list(res.min_b) == list(rep.min_b) and list(res.div_b) == list(rep.div_b)
    want, got, counts = xyzi_of(out), g["out"], rep.counts
    if res.path_flags & BUCKET and not res.path_flags & SPLIT:
        exact = np.ones(len(counts), bool)
    elif res.path_flags & BUCKET:
        exact = counts <= SEQ_EXACT_MAX
    else:
        exact = counts <= 2
    assert same_bits(got[exact], want[exact]), "centroids of the voxels the route adds in the oracle's order"
    assert_centroids_close_or_exact(got, want, counts, rep.cells, merged, leaf, sequential=False)


def skip_without_bucket(flags):
    if not flags & LDS_RANK:
        pytest.skip("the device probe did not find lane-ordered LDS adds: no bucket path on this device")


def check_packed(runs):
    skip_without_bucket(runs[-1]["flags"])
    for k, g in enumerate(runs):
        f = g["flags"]
        assert f & BUCKET and not f & REDONE and bool(f & PACKED) == (k > 0), (k, f)


# ---- the route x layout matrix ----------------------------------------------------------------------------------------
MATRIX_ROUTES = ["general", "fixed", "predicted", "quantile", "k2_local", "ballot", "packed", "outlier", "ground"]
_XYZI_RUNS = {}


def ground_scene():
    if "g" not in _SCENE:
        rng = np.random.default_rng(72)
        out = []
        for n in (60_013, 90_001):
            xyz = np.concatenate([tg.scene(rng, n - 20_000), clustered(rng, 20_000) + (20.0, 0.0, 1.5)]).astype(np.float32)
            out.append(xyzi_cloud(xyz[rng.permutation(n)], rng.uniform(0, 255, n).astype(np.float32)))
        _SCENE["g"] = out
    return _SCENE["g"]


def test_scene_has_every_voxel_size():
    """voxels of 1, 2, 3-17 and more than 17 points, in the scene the matrix runs"""
    _, _, _, rep = oracle_of(("crop", False), scene(), route_params("fixed"))
    assert rep.n_merged < sum(SIZES)
    c = rep.counts
    assert (c == 1).any() and (c == 2).any() and ((c >= 3) & (c <= 17)).any() and (c > 17).sum() >= 20
    assert all(n % 64 for n in SIZES)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("route", MATRIX_ROUTES)
def test_route_layout(route, layout, monkeypatch):
    env, _, n_frames = ROUTES.get(route, ({}, True, 2))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = route_params(route)
    base = ground_scene() if route == "ground" else scene()
    layouts = [layout] * len(base)
    ref = reference_of(base, layouts)
    clouds = packed_frames(base, layouts, 5)
    n_cap = sum(s.n for s in base)
    gp = None
    if route == "ground":
        gp = capi.make_ground_params([tg.FRONT] * len(base), 1000, 0.3, 0.99, True, 3.0, 12345)
    key = (route, layout in wl.NO_INTENSITY)
    if key not in _XYZI_RUNS:
        _XYZI_RUNS[key] = run_stream([ref] * n_frames, params, n_cap, len(base), ground=gp)
    want = _XYZI_RUNS[key]
    got = run_stream([clouds] * n_frames, params, n_cap, len(base), ground=gp)
    if route == "packed":
        check_packed(got)
    elif route == "ground":
        skip_without_bucket(got[-1]["flags"])
        assert got[-1]["flags"] & BUCKET and not got[-1]["flags"] & REDONE
    else:
        check_route(route, got[-1]["res"])
    assert_same_run(got, want, f"{route}/{layout}")
    if route == "ground":
        check_ground(got[-1], ref, params, key[1])
    else:
        for g in got:
            check_oracle(g, oracle_of((route_tag(route), key[1]), ref, params), params.leaf)


_GROUND = {}


def check_ground(g, sensors, params, zeroed):
    """tests/test_ground.check's bars on a frame already run (zeroed: the sensors' intensity is 0)"""
    if zeroed not in _GROUND:
        _GROUND[zeroed] = tg.expected(sensors, [tg.FRONT] * len(sensors), params, tg.GP)
    want_ng, want_g, want_planes = _GROUND[zeroed]
    assert same_bits(g["merged"], xyzi_of(want_ng)), "no-ground cloud (content and order)"
    assert same_bits(g["ground"], xyzi_of(want_g)), "ground cloud (content and order)"
    planes = (capi.GroundPlane * (capi.MAX_SENSORS * capi.MAX_ZONES)).from_buffer_copy(g["planes"])
    n_found = 0
    for s, pls in enumerate(want_planes):
        for z, pl in enumerate(pls):
            got = planes[s * 8 + z]
            if pl is None:
                assert got.band_points == 0 and got.found == 0
                continue
            assert got.found == pl.found and got.inliers == pl.n_inliers and got.iterations == pl.iterations
            if pl.found:
                n_found += 1
                assert np.abs(np.array(got.plane) - np.array(pl.plane)).max() <= 1e-6
    assert n_found >= 8
    st, vox, rep = oracle.voxelgrid(want_ng, params.leaf, params.min_points_per_voxel, stable=True)
    assert st == oracle.OK and g["res"].n_out == len(vox) and g["res"].n_merged == len(want_ng)
    assert np.array_equal(g["cells"], rep.cells) and np.array_equal(g["counts"], rep.counts)
    assert_centroids_close(g["out"], xyzi_of(vox))


# ---- several layouts in one frame -------------------------------------------------------------------------------------
MIXED = ["pcl32", "velo22", None, "odd17", "xyzi16", "ouster48", "tail", "pcl32_i12"]
MIXED_SIZES = [61_001, 47_113, 0, 1, 70_039, 2_049, 38_777, 29_311]
STEP16 = ["xyzi16", "zyx_i16", "i_first16", "xyz_pad16"]
MOVE = np.array([0.037, -0.021, 0.011])


def mixed_stream():
    if "m" not in _SCENE:
        # (smaller blobs: seven sensors' blobs in one box would overfill a bucket of the local finish, and the frame
        # would be handed back. The vehicle moves a few centimetres per frame: the quantiles of one frame fit the next.)
        clouds = make_scene(80, [max(n, 1) for n in MIXED_SIZES], blob_max=1000)
        frames = []
        for f in range(4):
            frames.append([None if lay is None else dataclasses.replace(c, t_xyz=tuple(np.asarray(c.t_xyz) + f * MOVE))
                           for c, lay in zip(clouds, MIXED)])
        _SCENE["m"] = frames
    return _SCENE["m"]


@pytest.mark.parametrize("route", ["quantile", "fixed", "packed"])
def test_mixed_layouts_in_one_frame(route, monkeypatch):
    """8 slots: 6 layouts, a 1-point sensor, a 2 049-point sensor and an empty slot; a 4-frame stream"""
    if route == "fixed":
        monkeypatch.setenv("CM_QUANT", "0")
    params = route_params(route if route == "packed" else "fixed")
    frames = mixed_stream()
    refs = [reference_of(fr, MIXED) for fr in frames]
    clouds = [packed_frames(fr, MIXED, 9 + k) for k, fr in enumerate(frames)]
    n_cap = max(sum(c.n for c in fr if c is not None) for fr in frames)
    got = run_stream(clouds, params, n_cap, len(MIXED))
    want = run_stream(refs, params, n_cap, len(MIXED))
    assert_same_run(got, want, route)
    for k, g in enumerate(got):
        check_oracle(g, oracle_of(("mixed", route == "packed", k), refs[k], params), params.leaf)
    if route == "packed":
        check_packed(got)
        return
    skip_without_bucket(got[-1]["flags"])
    for k, g in enumerate(got):
        f = g["flags"]
        assert f & BUCKET and not f & REDONE, (k, f)
        assert bool(f & QUANTILE) == (route == "quantile" and k > 0), (k, f)


@pytest.mark.parametrize("route", ["quantile", "fixed"])
def test_step16_layouts_with_different_offsets(route, monkeypatch):
    """four sensors of step 16 whose fields sit at different offsets: a tile read with another sensor's offsets gives
    wrong values inside the buffer"""
    if route == "fixed":
        monkeypatch.setenv("CM_QUANT", "0")
    base = make_scene(90, (40_961, 33_333, 52_007, 4_097))
    params = route_params("fixed")
    ref = reference_of(base, STEP16)
    clouds = packed_frames(base, STEP16, 13)
    n_cap = sum(s.n for s in base)
    got = run_stream([clouds] * 2, params, n_cap, 4)
    want = run_stream([ref] * 2, params, n_cap, 4)
    assert_same_run(got, want, route)
    check_oracle(got[-1], oracle_of(("step16",), ref, params), params.leaf)
    skip_without_bucket(got[-1]["flags"])
    assert bool(got[-1]["flags"] & QUANTILE) == (route == "quantile") and not got[-1]["flags"] & REDONE


def test_layout_changes_on_one_context():
    """sensor 1 goes xyzi16 -> velo22 -> pcl32 -> odd17 -> pcl32_i12 -> xyzi16 with the same points, the others keep
    theirs (the descriptor cache and the tile table see a new layout each frame): every frame gives the bits of the same
    stream fed xyzi16 throughout, frames 2 on run the quantile route without a hand-back and give frame 2's bits. Frame 1
    (fixed-grid passes) gives them too, up to the tree order of voxels of more than 17 points (CM_PATH_SPLIT)."""
    base = scene()
    params = route_params("fixed")
    rng = np.random.default_rng(17)
    others = {0: base[0], 2: wl.relayout(base[2], "livox18", rng)}
    frames = []
    for lay in ("xyzi16", "velo22", "pcl32", "odd17", "pcl32_i12", "xyzi16"):
        frames.append([others[0], base[1] if lay == "xyzi16" else wl.relayout(base[1], lay, rng), others[2]])
    n_cap = sum(s.n for s in base)
    runs = run_stream(frames, params, n_cap, 3)
    assert_same_run(runs, run_stream([base] * len(frames), params, n_cap, 3), "layout changes")
    ref = oracle_of(("crop", False), base, params)
    for g in runs:
        check_oracle(g, ref, params.leaf)
    skip_without_bucket(runs[-1]["flags"])
    assert runs[0]["flags"] & BUCKET and not runs[0]["flags"] & (QUANTILE | REDONE), runs[0]["flags"]
    for k, g in enumerate(runs[1:], 1):
        assert g["flags"] & QUANTILE and g["flags"] & BUCKET and not g["flags"] & REDONE, (k, g["flags"])
        assert_same_run([g], [runs[1]], f"frame {k + 1}")
    small = runs[0]["counts"] <= SEQ_EXACT_MAX
    assert same_bits(runs[0]["merged"], runs[1]["merged"]) and np.array_equal(runs[0]["cells"], runs[1]["cells"])
    assert same_bits(runs[0]["out"][small], runs[1]["out"][small])


def _hip():
    try:
        return C.CDLL("libamdhip64.so.7")
    except OSError:
        return C.CDLL("/opt/rocm/lib/libamdhip64.so")


@pytest.mark.parametrize("layout", ["xyzi16", "pcl32"])
@pytest.mark.parametrize("route", ["fixed", "quantile"])
def test_device_submit_at_any_alignment(route, layout, monkeypatch):
    """XYZI16 or PCL32 bytes at byte offsets 0, 4, 8 and 1 of one hipMalloc buffer: the offset-0 sensor takes the fast
    loader, the others must fall back to the generic one; results bit-identical to the host submit"""
    if route == "fixed":
        monkeypatch.setenv("CM_QUANT", "0")
    base = make_scene(91, (30_011, 45_007, 20_483, 51_001))
    params = route_params("fixed")
    clouds = packed_frames(base, [layout] * 4, 19)
    n_cap = sum(s.n for s in base)
    want = run_stream([clouds] * 2, params, n_cap, 4)
    hip = _hip()
    offsets = [0, 4, 8, 1]
    spans = [(c.n * c.point_step + 511) // 256 * 256 for c in clouds]
    starts = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(int)
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(int(sum(spans)))) == 0
    got = []
    try:
        for s, c in enumerate(clouds):
            data = np.ascontiguousarray(c.data)
            assert starts[s] + offsets[s] + data.nbytes <= sum(spans)
            assert hip.hipMemcpy(C.c_void_p(buf.value + int(starts[s]) + offsets[s]), C.c_void_p(data.ctypes.data),
                                 C.c_size_t(data.nbytes), 1) == 0
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for _ in range(2):
                for s, c in enumerate(clouds):
                    cm.set_transform(s, c.q_xyzw, c.t_xyz)
                    cm.submit_device(s, buf.value + int(starts[s]) + offsets[s], c.n, c.point_step, c.off_x, c.off_y,
                                     c.off_z, c.off_i)
                assert cm.merge_voxelize_async(capi.make_params(params)) == capi.OK
                res = cm.wait()
                assert res.status == capi.OK
                g = dict(res=res, flags=res.path_flags, merged=xyzi4(cm.merged(n_cap)), out=xyzi4(cm.result(res.n_out)))
                g["cells"], g["counts"] = cm.cells(res.n_out)
                got.append(g)
    finally:
        hip.hipFree(buf)
    assert_same_run(got, want, f"{route}/{layout} device")
    check_oracle(got[-1], oracle_of(("device",), reference_of(base, [layout] * 4), params), params.leaf)
    skip_without_bucket(got[-1]["flags"])
    assert bool(got[-1]["flags"] & QUANTILE) == (route == "quantile") and not got[-1]["flags"] & REDONE


# ---- special values through the generic loader ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["velo22", "odd17", "pcl32_i12"])
@pytest.mark.parametrize("route", ["general", "fixed", "quantile"])
def test_special_values_in_generic_layouts(route, layout, monkeypatch):
    """the value probes (NaN payloads in intensity, signed zeros, subnormals, exact-rational centroids) read by the
    generic loader: tests/test_edge_values.compare on the unpacked frame, and the xyzi16 run's bits"""
    frame = ef.value_frame()
    env, crop, n_frames = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = frame.with_crop(crop)
    from tests.test_edge_values import probe_cells_alone
    probe_cells_alone(frame, params)
    clouds = packed_frames(frame.sensors, [layout] * len(frame.sensors), 23)
    n_cap = sum(s.n for s in frame.sensors)
    got = run_stream([clouds] * n_frames, params, n_cap, len(clouds))
    want = run_stream([frame.sensors] * n_frames, params, n_cap, len(clouds))
    assert_same_run(got, want, f"{route}/{layout}")
    for g in got:
        compare(route, frame, params, g["res"], g["merged"], g["out"], g["cells"], g["counts"])
    check_route(route, got[-1]["res"])


# ---- fused ranks and motion -------------------------------------------------------------------------------------------
def fused_run(sensors, params):
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
            parts.append(cm.partial_device())
        res = cms[0].merge_tables([p[0] for p in parts], [p[1] for p in parts], params)
        assert res.status == capi.OK
        out = xyzi4(cms[0].result(res.n_out))
        cells, counts = cms[0].cells(res.n_out)
    finally:
        for cm in cms:
            cm.close()
    return res, out, cells, counts


def test_fused_two_ranks_mixed_layouts():
    """two contexts as ranks, each with sensors of different layouts: cm_merge_partial + cm_merge_tables"""
    base = make_scene(92, (40_003, 35_017, 52_001, 27_449, 1, 9_001))
    layouts = ["velo22", "odd17", "pcl32", "tail", "xyz12", "ouster48"]
    params = route_params("fixed")
    ref = reference_of(base, layouts)
    res, out, cells, counts = fused_run(packed_frames(base, layouts, 29), params)
    r0, o0, c0, n0 = fused_run(ref, params)
    assert res.n_out == r0.n_out and same_bits(out, o0), "merged table differs from the xyzi16 ranks'"
    assert np.array_equal(cells, c0) and np.array_equal(counts, n0)
    st, _, o, rep = oracle.merge_voxelize(ref, params, threads=4, stable=True)
    assert st == oracle.OK and res.n_out == rep.n_out
    assert np.array_equal(cells, rep.cells) and np.array_equal(counts, rep.counts)
    assert_centroids_close(out, xyzi_of(o))


def test_motion_with_time_at_odd_offsets():
    """k_motion reads odd17_t (f32 seconds at byte 17 of 21) and livox18_t (u32 ns at byte 19 of 23), with velo22 and
    ouster48 beside them: the frame is the one the numpy-compensated 16-byte clouds give, bit for bit"""
    rng = np.random.default_rng(93)
    kinds = ["odd17_t", "livox18_t", "velo22", "ouster48"]
    sizes = [61_003, 44_441, 30_001, 25_013]
    raws, stamps = [], [T_REF + int(s) for s in rng.integers(-50_000_000, 50_000_001, len(kinds))]
    for kind, n in zip(kinds, sizes):
        xyz, inten = synth.ground_scene(rng, n, 14.0, -2.0, 4.0)
        ttype = wl.ALL[kind].time[1]
        tau = (np.sort(rng.uniform(0, 0.1, n)).astype(np.float32) if ttype == capi.TIME_F32_S
               else rng.integers(0, 100_000_000, n).astype(np.uint32))
        c = wl.repack(xyz, inten, kind, rng, tau=tau, q_xyzw=synth.random_quaternion(rng), t_xyz=rng.uniform(-2, 2, 3))
        raws.append((c, xyz, inten, tau, ttype))
    n_cap = sum(sizes)
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2, crop_min=(-10.0, -8.0, -1.8), crop_max=(9.0, 10.0, 2.5))
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for s, (c, *_r, ttype) in enumerate(raws):
            cm.set_transform(s, c.q_xyzw, c.t_xyz)
            cm.set_time_field(s, wl.ALL[kinds[s]].time[0], ttype)
            cm.submit(s, c)
        cm.set_ego_motion(capi.make_motion(V, W, T_REF, stamps))
        want = []
        for s, (c, xyz, inten, tau, ttype) in enumerate(raws):
            comp = mr.compensate(xyz, cm.get_matrix(s), mr.time_of(tau, ttype), mr.dt0_s(stamps[s], T_REF), V, W, inten)
            want.append(xyzi_cloud(comp[:, :3], comp[:, 3], is_dense=False))
        res, got, cells, counts, merged, _ = motion_run(cm, params, n_cap)
    assert res.status == capi.OK and res.path_flags & capi.PATH_MOTION
    p_res, p_got, p_cells, p_counts, p_merged, _ = plain_run(want, params, n_cap)
    assert same_bits(got, p_got) and same_bits(merged, p_merged), "the frame the compensated clouds give"
    assert np.array_equal(cells, p_cells) and np.array_equal(counts, p_counts)
    assert res.path_flags == p_res.path_flags | capi.PATH_MOTION
    assert 0 < res.n_merged < n_cap
