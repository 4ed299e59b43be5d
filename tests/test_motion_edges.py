"""Ego-motion compensation (k_motion, cm_kernels_motion.hip; build_frame, cm_launch.cpp) at the edges of its frame geometry,
time values, stamps and twists: the designed frames of tests/motion_edge_frames.py.

Unless a test says otherwise every GPU test makes the same two comparisons (`the_check`):
  * cm.merged() equals, bit for bit and signs of zeros included, motion_ref.compensate of every raw cloud, filtered as
    point_valid filters (finite, inside the crop box) and concatenated in (sensor, point) order; frame_stats()["n_kept"] holds
    the per-sensor counts of that filter;
  * status, n_merged, n_out, result, cells, counts and merged cloud equal those of a context that never set motion and was
    fed the numpy-compensated 16-byte clouds with identity transforms; path_flags are equal up to PATH_MOTION.
The unmarked tests at the top assert on the restatement alone what the frames are designed to hold."""
import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import motion_edge_frames as ef
from tests import motion_ref as mr
from tests.test_motion import plain_run, run, setup_and_submit, xyzi4
from tests.util import assert_centroids_close, same_bits

F = np.float32
T_REF, V, W = ef.T_REF, ef.V, ef.W
PARAMS = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)
PARAMS_2 = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=2)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- CPU: what the designed frames hold -----------------------------------------------------------------------------------
def test_sizes_straddle_the_workgroup_and_the_tile():
    assert ef.SIZES == [1, 2, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145]
    assert len(ef.TWISTS) == 16 and len({t[0] for t in ef.TWISTS}) == 16


def test_u32_times_round_to_nearest_even_over_the_unsigned_range():
    t = {u: float(np.asarray([u], np.uint32).astype(F)[0]) for u in ef.U32_NS}
    assert t[2 ** 24 + 1] == 2 ** 24 and t[2 ** 24 + 3] == 2 ** 24 + 4 and t[2 ** 24 - 1] == 2 ** 24 - 1          # ties to even
    assert t[2 ** 31 - 1] == 2 ** 31 and t[2 ** 31 + 129] == 2 ** 31 + 256
    assert t[2 ** 32 - 257] == t[2 ** 32 - 129] == 2 ** 32 - 256 and t[2 ** 32 - 128] == t[2 ** 32 - 1] == 2 ** 32        # the tie at -128: to even
    signed = np.asarray(ef.U32_NS, np.uint32).view(np.int32).astype(F)
    assert (signed != np.asarray(ef.U32_NS, np.uint32).astype(F)).sum() == 7          # a conversion through int shows on seven values
    clouds, stamps = ef.u32_frame()
    for c, st in zip(clouds, stamps):
        out = c.compensated(ef.IDENT_M, st, T_REF, V, W)
        assert np.linalg.norm(c.xyz, axis=1).max() <= 50.0
        assert np.isfinite(out).all() and 90.0 < np.abs(out[:, :3]).max() < 110.0     # (the largest coordinate is about 106)
        tau = mr.time_of(c.tau_raw, c.time[1])
        assert (tau >= 0).all() and tau.max() == F(2 ** 32) * F(1e-9)


def test_f32_times_leave_exactly_the_overflowing_ones_non_finite():
    clouds, stamps = ef.f32_frame()
    n = len(ef.F32_S)
    want = np.array([any(np.array_equal(F(v), F(b), equal_nan=True) for b in ef.F32_NON_FINITE) for v in ef.F32_S])
    assert want.sum() == 7
    for c, st in zip(clouds, stamps):
        out = c.compensated(ef.IDENT_M, st, T_REF, V, W)
        bad = ~np.isfinite(out[:, :3]).all(axis=1)
        assert np.array_equal(bad, np.tile(want, ef.REPEATS)), (c.kind, np.flatnonzero(bad[:n] != want))
        dt = mr.dt0_s(st, T_REF) + c.tau_raw[:n]
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(~np.isfinite(dt * dt), want)                          # dt * dt is what overflows; 1e19 squares to 1e38
        assert np.abs(out[10::n, :3]).max() > 1e38                                     # ... and its points land finite, near FLT_MAX


def test_cancelling_time_gives_the_transformed_point():
    assert mr.dt0_s(ef.CANCEL_STAMP, T_REF) == F(-0.03) and F(-0.03) + F(0.03) == 0
    clouds, stamps = ef.cancel_frame()
    for c, st in zip(clouds, stamps):
        m = ef.matrix_of(c.q, c.t)
        out = c.compensated(m, st, T_REF, V, W)
        assert same_bits(out[:, :3], np.stack(mr.transform(c.xyz, m), 1))


def test_dt0_wraps_modulo_2_64_and_rounds_twice():
    assert mr.dt0_s(ef.INT64_MIN + 5, ef.INT64_MAX) == F(6e-9)
    assert mr.dt0_s(ef.INT64_MAX, ef.INT64_MIN) == F(-1e-9)
    assert mr.dt0_s(T_REF - 50_000_000, T_REF) == F(-0.05) and mr.dt0_s(T_REF, T_REF) == 0
    # the large differences: int64 -> double rounds 2^53 + 1 to 2^53 (a tie, to even), then the product, then fp32
    assert mr.dt0_s(T_REF + 2 ** 53 + 1, T_REF) == F(float(2 ** 53) * 1e-9) and mr.dt0_s(T_REF - 2 ** 53 - 1, T_REF) == F(float(-2 ** 53) * 1e-9)
    assert mr.dt0_s(T_REF + 2 ** 24 + 1, T_REF) == F(16777217e-9) and mr.dt0_s(T_REF + 3_600_000_000_000, T_REF) == F(3600.0)
    assert [float(mr.dt0_s(T_REF + d, T_REF)) for d in (1, -1)] == [float(F(1e-9)), float(F(-1e-9))]
    clouds, stamps = ef.stamp_frame()
    far = [np.abs(c.compensated(ef.matrix_of(c.q, c.t), st, T_REF, V, W)[:, :3]).max() for c, st in zip(clouds, stamps)]
    assert max(far[:5]) < 100.0 and min(far[5:]) > 5e4 and np.isfinite(far).all()      # the crop box drops the last four clouds


def test_unused_stamp_entries_would_move_a_point_by_metres():
    st = ef.hole_stamps(T_REF, ef.HOLE_SLOTS)
    for s in range(16):
        d = abs(float(mr.dt0_s(st[s], T_REF))) * V[0]
        assert (d < 1.0) if s in ef.HOLE_SLOTS else (d > 7.0)
        if s < 4:                                      # entry j of the descriptor (j = 0..3) is not its slot's: stamp_ns[j] shows
            assert st[s] != st[ef.HOLE_SLOTS[s]]


def test_denormal_frame_changes_when_denormals_are_flushed():
    (c,), (st,) = ef.denormal_frame()
    v, w = ef.DENORMAL_V, ef.DENORMAL_W
    out = c.compensated(ef.IDENT_M, st, T_REF, v, w)
    assert np.allclose(out[0, :3].astype(np.float64), [1.0010021e-36, 2.9999899e-37, 9.9999833e-37], rtol=2e-7, atol=0)
    cr = np.stack(mr.cross(tuple(F(a) for a in w), tuple(c.xyz[:, a] for a in range(3))), 1)
    assert (np.abs(cr[cr != 0]) < ef.FLT_MIN).all() and (cr != 0).any(axis=1).all()    # w x q: denormal in every point
    # the same arithmetic with every denormal intermediate flushed to zero: c, e and k vanish, only dt v is left
    flushed = c.xyz.copy()
    flushed[:, 0] = c.xyz[:, 0] + F(ef.DENORMAL_TAU) * F(v[0])
    assert (bits(out[:, :3]) != bits(flushed)).any(axis=1).all()


@pytest.mark.parametrize("v,w,n,span", [(V, (0.02, 0.01, 0.3), 200_000, 0.1)] + [(v, w, 20_000, ef.LARGE_SPAN) for v, w in ef.LARGE_TWISTS])
def test_restatement_within_the_series_remainder(v, w, n, span):
    """The restatement against exp(dt xi) q in float64, at the envelope of test_restatement_within_2mm_of_the_exponential and
    at each large twist of the twist tests, with a bound derived from the series instead of a millimetre figure.

    Truncation. With phi = w dt, K = [phi]x and theta = |w| |dt|:
        exp(dt xi) q = sum_n K^n q / n!  +  dt sum_n K^n v / (n + 1)!                  (Rodrigues and the V matrix as series)
    and the kernel keeps q + K q + K^2 q / 2 + dt v + dt K v / 2 = q + dt (c + v) + h (e + k). What it drops is
        sum_{n>=3} K^n q / n!  +  dt sum_{n>=2} K^n v / (n + 1)!,   |K^n x| <= theta^n |x|,
    and dt theta^n / (n + 1)! = (1 / |w|) theta^(n+1) / (n + 1)!, so both sums are bounded by the third-order remainder
        E3(theta) = sum_{m>=3} theta^m / m!   of the exponential series:   |dropped| <= (|q| + |v| / |w|) E3(theta).

    Rounding, per component and to first order in u = 2^-24, with the magnitudes bounded by C = 2 max|w| max|q|,
    E = 2 max|w| C, Kk = 2 max|w| max|v|, S1 = C + max|v|, S2 = E + Kk (q itself is exact: identity transform):
        c: two products and a difference        2u C          e: the same on a c that is 2u off      4u E        k: 2u Kk
        c + v: 2u C + u S1 <= 3u S1             dt = dt0 + tau: u |dt|                 dt (c + v): (3 + 1 + 1) u |dt| S1
        e + k: 4u E + 2u Kk + u S2 <= 5u S2     h = 0.5 (dt dt): (2 + 1) u h           h (e + k):  (5 + 3 + 1) u h S2
        the inner sum: u (|dt| S1 + h S2)       the outer sum: u (max|q| + |dt| S1 + h S2)
    in all u (max|q| + 7 |dt| S1 + 11 h S2) <= 19 u L with L the largest of the three terms max|q|, |dt| S1, h S2. The test
    allows 20 u L per component (the twentieth for the terms of second order in u), sqrt(3) times that for the distance."""
    rng = np.random.default_rng(17)
    d = rng.standard_normal((n, 3))
    xyz = (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(1, 50, n)[:, None]).astype(F)
    v32, w32 = np.asarray(v, F), np.asarray(w, F)
    dt0 = mr.dt0_s(T_REF - 30_000_000, T_REF)
    tau = rng.uniform(0, span, n).astype(F)
    got = mr.compensate(xyz, ef.IDENT_M, tau, dt0, v32, w32)[:, :3].astype(np.float64)
    dt = np.float64(dt0) + tau.astype(np.float64)
    R, t = synth.se3_exp(v32.astype(np.float64), w32.astype(np.float64), dt)
    q = xyz.astype(np.float64)
    exact = np.einsum("nij,nj->ni", R, q) + t
    wn, vn = np.linalg.norm(w32.astype(np.float64)), np.linalg.norm(v32.astype(np.float64))
    theta, term, e3 = wn * np.abs(dt), np.ones(n), np.zeros(n)
    for m in range(1, 80):                                     # E3 as a sum of positive terms: no cancellation at small theta
        term = term * theta / m
        if m >= 3:
            e3 += term
    truncation = (np.linalg.norm(q, axis=1) + vn / wn) * e3
    u = 2.0 ** -24
    wm, vm, qm = np.abs(w32).max().astype(np.float64), np.abs(v32).max().astype(np.float64), np.abs(q).max(axis=1)
    C = 2 * wm * qm
    S1, S2 = C + vm, 2 * wm * C + 2 * wm * vm
    L = np.maximum(qm, np.maximum(np.abs(dt) * S1, 0.5 * dt * dt * S2))
    bound = truncation + np.sqrt(3.0) * 20 * u * L
    err = np.linalg.norm(got - exact, axis=1)
    worst = np.argmax(err / bound)
    print(f"|w| {wn:.3g} |v| {vn:.3g}: theta up to {theta.max():.3g}, worst err / bound {err[worst] / bound[worst]:.3g} at theta {theta[worst]:.3g} "
          f"(err {err[worst]:.3g} m, truncation {truncation[worst]:.3g} m, rounding {bound[worst] - truncation[worst]:.3g} m)")
    assert (err <= bound).all()
    small = theta < 0.02                                       # where the series has converged the bound is a tight one
    assert small.sum() >= 50 and bound[small].max() < 2e-3


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------
def feed(cm, clouds, stamps, t_ref, v, w, slots=None):
    """Transforms, time fields, clouds and the twist. slots: the sensor slot of every cloud (None: 0, 1, ...), stamps by slot."""
    if slots is None:
        return setup_and_submit(cm, clouds, stamps, t_ref, v, w)
    for s, r in zip(slots, clouds):
        cm.set_transform(s, r.q, r.t)
        cm.set_time_field(s, *r.time)
        cm.submit(s, r.cloud)
    cm.set_ego_motion(capi.make_motion(v, w, t_ref, stamps))


def restated(cm, clouds, stamps, t_ref, v, w, slots=None):
    """motion_ref.compensate of every cloud, with the matrix the context holds: a list of (n, 4) arrays."""
    slots = range(len(clouds)) if slots is None else slots
    return [r.compensated(cm.get_matrix(s), stamps[s], t_ref, v, w) for s, r in zip(slots, clouds)]


def as_clouds(want4):
    return [xyzi_cloud(c[:, :3], c[:, 3], is_dense=False) for c in want4]


def outputs(cm, params, n_cap):
    res, got, cells, counts, merged, _ = run(cm, params, n_cap)
    return dict(res=res, got=got, cells=cells, counts=counts, merged=merged, kept=cm.frame_stats()["n_kept"])


def plain_outputs(sensors, params, n_cap):
    res, got, cells, counts, merged, _ = plain_run(sensors, params, n_cap)
    return dict(res=res, got=got, cells=cells, counts=counts, merged=merged)


def assert_merged_is(out, want4, params):
    keep = [mr.valid(c, params.crop_min, params.crop_max) for c in want4]
    exp = np.concatenate([c[k] for c, k in zip(want4, keep)])
    got = out["merged"]
    assert got.shape == exp.shape, (got.shape, exp.shape, out["kept"], [int(k.sum()) for k in keep])
    if not same_bits(got, exp):
        bad = np.flatnonzero((bits(got) != bits(exp)).any(axis=1))
        raise AssertionError(f"{len(bad)} of {len(exp)} merged points differ, first at {bad[0]}: got {got[bad[0]]} want {exp[bad[0]]}")
    # (cm_get_frame_stats counts n_kept for frames with a voxel grid only: zeros with any other status)
    assert out["kept"] == [int(k.sum()) if out["res"].status == capi.OK else 0 for k in keep] and out["res"].n_merged == len(exp)
    return keep


def assert_same_frame(a, b, exact_result=True):
    ra, rb = a["res"], b["res"]
    assert ra.status == rb.status, (capi.status_string(ra.status), capi.status_string(rb.status))
    assert (ra.n_merged, ra.n_out) == (rb.n_merged, rb.n_out)
    assert same_bits(a["merged"], b["merged"])
    assert (a["cells"] is None) == (b["cells"] is None)
    if a["cells"] is not None:
        assert np.array_equal(a["cells"], b["cells"]) and np.array_equal(a["counts"], b["counts"])
    if exact_result:
        assert same_bits(a["got"], b["got"])
        assert ra.path_flags & ~capi.PATH_MOTION == rb.path_flags & ~capi.PATH_MOTION
    else:
        assert_centroids_close(a["got"], b["got"])


def the_check(clouds, stamps, t_ref=T_REF, v=V, w=W, params=PARAMS, slots=None, max_sensors=None):
    """Both comparisons on a fresh context. Returns (outputs, restated clouds, their point_valid masks)."""
    n_cap = max(1, sum(r.cloud.n for r in clouds))
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=max_sensors or len(clouds), flags=capi.FLAG_OCCUPANCY) as cm:
        feed(cm, clouds, stamps, t_ref, v, w, slots)
        want4 = restated(cm, clouds, stamps, t_ref, v, w, slots)
        out = outputs(cm, params, n_cap)
    assert bool(out["res"].path_flags & capi.PATH_MOTION) == any(r.cloud.n for r in clouds)
    keep = assert_merged_is(out, want4, params)
    assert_same_frame(out, plain_outputs(as_clouds(want4), params, n_cap))
    return out, want4, keep


# ---- GPU 1: frame geometry ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", ef.SIZES)
def test_cloud_sizes_around_the_workgroup(n):
    clouds, stamps = ef.mixed3(n)
    out, want4, _ = the_check(clouds, stamps, params=PARAMS_2 if n % 2 else PARAMS)
    assert out["res"].status == capi.OK and out["res"].n_merged == 300 + n + 4100
    # the neighbour's first records and the cloud's own last ones, named on their own
    assert same_bits(out["merged"][300 + n:300 + n + 8], want4[2][:8]) and same_bits(out["merged"][300 + n - 1], want4[1][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", ef.EMPTY_PATTERNS, ids=lambda s: "-".join(map(str, s)))
def test_empty_clouds_in_front_between_and_behind(sizes):
    clouds, stamps = ef.sized(sizes)
    out, _, _ = the_check(clouds, stamps, max_sensors=5)
    assert out["res"].status == capi.OK and out["res"].n_merged == sum(sizes) and out["kept"] == list(sizes)


@pytest.mark.gpu
def test_every_cloud_empty():
    clouds, stamps = ef.sized(ef.ALL_EMPTY)
    with capi.CloudMerger(max_points_total=16, max_sensors=5, flags=capi.FLAG_OCCUPANCY) as cm:
        feed(cm, clouds, stamps, T_REF, V, W)
        out = outputs(cm, PARAMS, 16)
    p = plain_outputs([r.cloud for r in clouds], PARAMS, 16)
    assert out["res"].status == p["res"].status == capi.EMPTY_INPUT
    assert_same_frame(out, p)
    assert out["res"].n_merged == 0 and len(out["merged"]) == 0 and out["kept"] == [0] * 5


@pytest.mark.gpu
def test_slots_with_holes_and_a_stale_second_frame():
    first, second = ef.holes()
    slots = list(ef.HOLE_SLOTS)
    n_cap = sum(r.cloud.n for r in first.values()) + 77 * len(second)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=16, flags=capi.FLAG_OCCUPANCY) as cm, \
            capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as plain:
        clouds = [first[s] for s in slots]
        stamps = ef.hole_stamps(T_REF, slots)
        feed(cm, clouds, stamps, T_REF, V, W, slots)
        want4 = restated(cm, clouds, stamps, T_REF, V, W, slots)
        out = outputs(cm, PARAMS, n_cap)
        assert out["res"].status == capi.OK and out["res"].path_flags & capi.PATH_MOTION and cm.frame_stats()["sensor"] == slots
        assert_merged_is(out, want4, PARAMS)
        plain.submit_all(as_clouds(want4))
        assert_same_frame(out, outputs(plain, PARAMS, n_cap))
        # the next tick: slots 4 and 15 deliver, 1 and 9 ride along stale with the stamps of their own headers
        t_ref = T_REF + 100_000_000
        stamps2 = ef.hole_stamps(t_ref, ef.HOLE_FRESH)
        for s in (1, 9):
            stamps2[s] = stamps[s]
        assert len(set(stamps2)) == 16
        clouds2 = [second.get(s, first[s]) for s in slots]
        for s in ef.HOLE_FRESH:
            cm.submit(s, second[s].cloud)
        cm.set_ego_motion(capi.make_motion(ef.V2, ef.W2, t_ref, stamps2))
        params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, required_sensor_mask=sum(1 << s for s in ef.HOLE_FRESH))
        want4 = restated(cm, clouds2, stamps2, t_ref, ef.V2, ef.W2, slots)
        out = outputs(cm, params, n_cap)
        assert out["res"].status == capi.OK and out["res"].path_flags & capi.PATH_MOTION
        assert cm.frame_stats()["fresh"] == [0, 1, 0, 1] and cm.frame_stats()["sensor"] == slots
        assert_merged_is(out, want4, params)
        plain.submit_all(as_clouds(want4))
        assert_same_frame(out, outputs(plain, PARAMS, n_cap))


@pytest.mark.gpu
def test_sixteen_sensors():
    clouds, stamps = ef.sized([130] * 16, seed=4)
    assert len(set(stamps)) == 16
    out, _, _ = the_check(clouds, stamps, max_sensors=16)
    assert out["res"].status == capi.OK and out["kept"] == [130] * 16


# ---- GPU 2: time values ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_u32_times_over_the_unsigned_range():
    clouds, stamps = ef.u32_frame()
    out, want4, keep = the_check(clouds, stamps)
    assert out["res"].status == capi.OK and all(k.all() for k in keep) and out["kept"] == [len(ef.U32_NS) * ef.REPEATS] * 2


@pytest.mark.gpu
@pytest.mark.parametrize("leaf,crop", [(0.5, None), (0.5, 1000.0), (1e36, None)], ids=["grid_overflows", "crop_box", "huge_leaf"])
def test_f32_times_signed_denormal_huge_and_non_finite(leaf, crop):
    """The finite 1e19 s points lie near FLT_MAX. At a 0.5 m leaf without a crop box no grid holds them: whatever status the plain
    context returns for the restated clouds is the status asked for. A crop box of 1 km makes the frame an ordinary one, with
    the far points dropped on both sides; a leaf of 1e36 m makes a grid of a few hundred cells that holds every finite point,
    so that n_kept counts exactly the values the restatement leaves finite."""
    clouds, stamps = ef.f32_frame()
    params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=0, crop_min=(-crop,) * 3 if crop else None, crop_max=(crop,) * 3 if crop else None)
    out, want4, keep = the_check(clouds, stamps, params=params)
    finite = len(ef.F32_S) - len(ef.F32_NON_FINITE)
    assert out["res"].n_merged == sum(int(k.sum()) for k in keep)
    if crop:
        assert out["res"].status == capi.OK and all(0 < k.sum() < finite * ef.REPEATS for k in keep)
    else:
        assert all(k.sum() == finite * ef.REPEATS for k in keep)
        if leaf == 1e36:
            assert out["res"].status == capi.OK and out["kept"] == [finite * ef.REPEATS] * 3


@pytest.mark.gpu
def test_a_time_that_cancels_the_stamp_leaves_the_transformed_point():
    clouds, stamps = ef.cancel_frame()
    n_cap = sum(r.cloud.n for r in clouds)
    out, want4, _ = the_check(clouds, stamps)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2) as cm:       # the transformed raw points, from the library itself
        for s, r in enumerate(clouds):
            cm.set_transform(s, r.q, r.t)
            cm.submit(s, r.cloud)
        assert cm.merge_voxelize(PARAMS).status == capi.OK
        assert same_bits(out["merged"], xyzi4(cm.merged(n_cap)))
        q = np.concatenate([np.stack(mr.transform(r.xyz, cm.get_matrix(s)), 1) for s, r in enumerate(clouds)])
    assert same_bits(out["merged"][:, :3], q)


@pytest.mark.gpu
def test_stamp_differences_from_a_nanosecond_to_months():
    clouds, stamps = ef.stamp_frame()
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, crop_min=ef.STAMP_CROP[0], crop_max=ef.STAMP_CROP[1])
    out, _, keep = the_check(clouds, stamps, params=params)
    assert out["res"].status == capi.OK and out["kept"] == [200] * 5 + [0] * 4


@pytest.mark.gpu
def test_stamp_difference_wraps_modulo_2_64():
    clouds, stamps = ef.wrap_frame()
    out, _, keep = the_check(clouds, stamps, t_ref=ef.WRAP_T_REF)
    assert out["res"].status == capi.OK and all(k.all() for k in keep)


# ---- GPU 3: twists --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,v,w,span", ef.TWISTS, ids=[t[0] for t in ef.TWISTS])
def test_twists(name, v, w, span):
    clouds, stamps = ef.mixed3(3000, seed=20, n0=3000, n2=3000, span=span, zeros=True)
    out, want4, keep = the_check(clouds, stamps, v=v, w=w)
    assert out["res"].status == capi.OK and all(k.all() for k in keep)
    if name in ("zero", "minus_zero_twist"):
        # every term is a zero: the output is q wherever q is not itself a zero (-0.0 + 0.0 is +0.0), on the device as in numpy
        n_cap = sum(r.cloud.n for r in clouds)
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
            for s, r in enumerate(clouds):
                cm.set_transform(s, r.q, r.t)
                cm.submit(s, r.cloud)
            assert cm.merge_voxelize(PARAMS).status == capi.OK
            q = xyzi4(cm.merged(n_cap))
        same = bits(out["merged"]) == bits(q)
        assert same[q != 0].all() and (out["merged"] == q).all() and same.all(axis=1).sum() >= n_cap - 6
    else:
        moved = np.concatenate([np.stack(mr.transform(r.xyz, ef.matrix_of(r.q, r.t)), 1) for r in clouds])
        assert (np.abs(out["merged"][:, :3] - moved).max(axis=1) > 1e-3).mean() > 0.8


@pytest.mark.gpu
def test_denormal_products_are_not_flushed():
    clouds, stamps = ef.denormal_frame()
    out, want4, keep = the_check(clouds, stamps, v=ef.DENORMAL_V, w=ef.DENORMAL_W)
    assert out["res"].status == capi.OK and keep[0].all() and (bits(out["merged"][:, :3]) != bits(clouds[0].xyz)).any(axis=1).all()


# ---- GPU 4: the fast layouts with a time field ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_fast_layouts_with_a_time_field():
    """PCL32 with f32 seconds at byte 20 and u32 nanoseconds at byte 28 of its padding; XYZI16 whose intensity bytes are also
    read as the time, u32 and f32. (The clouds are 16-byte aligned device copies, so build_frame picks the fast loaders.)"""
    clouds, stamps = ef.fast_frame()
    for r, kind in zip(clouds, ef.FAST_KINDS):
        lay = ef.wl.layout(kind)
        assert lay.fast in ("PCL32", "XYZI16") and r.time == lay.time and r.cloud.point_step == lay.step and r.cloud.off_i == lay.off[3]
    assert same_bits(clouds[2].inten, clouds[2].tau_raw.view(F)) and same_bits(clouds[3].inten, clouds[3].tau_raw)
    out, want4, keep = the_check(clouds, stamps, params=PARAMS_2)
    assert out["res"].status == capi.OK and out["res"].path_flags & capi.PATH_MOTION and all(k.all() for k in keep)
    assert same_bits(np.concatenate([c[:, 3] for c in want4]), out["merged"][:, 3])


# ---- GPU 5: sequences on one context ----------------------------------------------------------------------------------------
def sequence():
    """(clouds, stamps, t_ref, twist or None, sensors to clear first) of the frames A, B, C and D."""
    a, sa = ef.seq_frame([8000] * 4, 30)
    b, sb = ef.seq_frame([1, ef.WG + 1], 31)
    d, sd = ef.seq_frame([8000] * 4, 32)
    return [(a, sa, T_REF, (V, W), ()), (b, sb, T_REF + 100_000_000, (ef.V2, ef.W2), (2, 3)), (a, sa, T_REF + 200_000_000, None, ()),
            (d, sd, T_REF + 300_000_000, (V, W), ())]


def submit_frame(cm, clouds, stamps, t_ref, twist, clear):
    for s in clear:
        cm.clear(s)
    if twist is None:
        cm.set_ego_motion(None)
        for s, r in enumerate(clouds):
            cm.set_transform(s, r.q, r.t)
            cm.submit(s, r.cloud)
        return None
    feed(cm, clouds, stamps, t_ref, *twist)
    return restated(cm, clouds, stamps, t_ref, *twist)


@pytest.mark.gpu
def test_shrinking_frames_motion_off_and_on_again():
    """A: 4 x 8000 points; B: two sensors of 1 and 2049 points, another twist, the other two slots cleared; C: A's clouds with
    motion off; D: motion on again at A's sizes. Every frame against the restatement, against a plain context with the same
    history (everything, bit for bit) and against the same frame on a fresh context (there the route may differ with the
    history: a result on another route is held to the centroid tolerance, everything else to equality)."""
    n_cap = 32_000
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm, \
            capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as plain:
        for k, (clouds, stamps, t_ref, twist, clear) in enumerate(sequence()):
            want4 = submit_frame(cm, clouds, stamps, t_ref, twist, clear)
            out = outputs(cm, PARAMS_2, n_cap)
            assert out["res"].status == capi.OK and bool(out["res"].path_flags & capi.PATH_MOTION) == (twist is not None), k
            for s in clear:
                plain.clear(s)
            if twist is not None:
                assert_merged_is(out, want4, PARAMS_2)
                plain.submit_all(as_clouds(want4))
            else:
                plain.submit_all([r.cloud for r in clouds])
            assert_same_frame(out, outputs(plain, PARAMS_2, n_cap))
            with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(clouds), flags=capi.FLAG_OCCUPANCY) as fresh:
                submit_frame(fresh, clouds, stamps, t_ref, twist, ())
                alone = outputs(fresh, PARAMS_2, n_cap)
            same_route = out["res"].path_flags == alone["res"].path_flags
            assert_same_frame(out, alone, exact_result=same_route)
            assert out["kept"] == alone["kept"]


@pytest.mark.gpu
def test_async_submit_with_motion():
    clouds, stamps, t_ref, (v, w), _ = sequence()[0]
    n_cap = 32_000
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        feed(cm, clouds, stamps, t_ref, v, w)
        want4 = restated(cm, clouds, stamps, t_ref, v, w)
        sync = outputs(cm, PARAMS_2, n_cap)
    holders = []
    try:
        for r in clouds:
            raw = np.ascontiguousarray(r.cloud.data).view(np.uint8).reshape(-1)
            h = capi.pinned_array(raw.nbytes)
            h.array[:] = raw
            holders.append(h)
        with capi.CloudMerger(max_points_total=n_cap, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
            for s, r in enumerate(clouds):
                cm.set_transform(s, r.q, r.t)
                cm.set_time_field(s, *r.time)
                assert cm.submit_async(s, r.cloud, host_ptr=holders[s].ptr.value) == capi.OK
            cm.set_ego_motion(capi.make_motion(v, w, t_ref, stamps))
            assert cm.merge_voxelize_async(capi.make_params(PARAMS_2)) == capi.OK
            res = cm.wait()
            cells, counts = cm.cells(res.n_out)
            got = dict(res=res, got=xyzi4(cm.result(res.n_out)), cells=cells, counts=counts, merged=xyzi4(cm.merged(n_cap)),
                       kept=cm.frame_stats()["n_kept"])
    finally:
        for h in holders:
            h.free()
    assert res.status == capi.OK and res.path_flags == sync["res"].path_flags and res.path_flags & capi.PATH_MOTION
    assert_merged_is(got, want4, PARAMS_2)
    assert_same_frame(got, sync)


@pytest.mark.gpu
def test_grid_overflow_fallback_sees_compensated_points():
    clouds, stamps = ef.mixed3(3000, seed=40)
    params = MergeParams(leaf=ef.OVERFLOW_LEAF, min_points_per_voxel=0)
    out, want4, keep = the_check(clouds, stamps, params=params)
    assert out["res"].status == capi.GRID_OVERFLOW and out["res"].path_flags & capi.PATH_MOTION
    assert out["res"].n_out == out["res"].n_merged == 300 + 3000 + 4100
    assert same_bits(out["got"], np.concatenate(want4))                      # the fallback result is the merged, compensated input
