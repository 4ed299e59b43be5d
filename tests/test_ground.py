"""Zone-wise ground removal before the fuse: the HIP stage (through the C-ABI) against
the oracle's restatement of removeGround's RANSAC plane (oracle.ground_split / orc_ransac_plane), same sample
generator on both sides. Plane coefficients within 1e-6; found, inliers, iterations and band size of every slab equal;
no-ground and ground clouds bit-exact in content and order; the voxel grid of the no-ground cloud with the usual bars.
(expected / check also take tests/ground_ref.py's restatement as the definition: tests/test_ground_edges.py.)"""
import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from oracle import oracle
from tests.util import assert_centroids_close, same_bits, xyzi_of

pytestmark = pytest.mark.gpu

ROI = dict(crop_min=(-15.0, -5.0, -0.5), crop_max=(60.0, 5.0, 3.0))
# proceedFront's five slabs (Parameter.h:45-55): front, mid2, mid, vehicle, rear — (x_min, x_length, z_max_ground)
FRONT = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]
GP = dict(max_iterations=1000, threshold=0.3, probability=0.99, optimize=True, z_keep_max=3.0, seed=12345)


def scene(rng, n, tilt=0.01, ground_sigma=0.03, obj_frac=0.25, obj_z=(0.6, 2.9)):
    """Tilted noisy ground + boxes above it (obj_z: their height range), vehicle frame."""
    ng = int(n * (1 - obj_frac))
    gx, gy = rng.uniform(-15, 60, ng), rng.uniform(-5, 5, ng)
    g = np.stack([gx, gy, -0.05 + tilt * gx + 0.02 * gy + ground_sigma * rng.standard_normal(ng)], 1)
    no = n - ng
    o = np.stack([rng.uniform(-15, 60, no), rng.uniform(-5, 5, no), rng.uniform(*obj_z, no)], 1)
    xyz = np.concatenate([g, o]).astype(np.float32)
    return xyz[rng.permutation(n)]


def expected(sensors, zones, params, gp, split=oracle.ground_split):
    """split: the definition of the stage for one sensor — the oracle's, or tests/ground_ref.py's restatement of it.
    Each plane it returns carries band_points, the size of its slab's band."""
    no_ground, ground, planes = [], [], []
    for s, c in enumerate(sensors):
        pts = oracle.make_points(np.stack([c.data["x"], c.data["y"], c.data["z"]], 1), c.data["intensity"])
        tp = oracle.transform(pts, oracle.quat_to_matrix(c.q_xyzw, c.t_xyz))
        if params.crop_min is not None:
            cp = oracle.crop(tp, params.crop_min, params.crop_max)
        else:                                                        # non-finite points vanish, crop box or not
            cp = tp[np.isfinite(tp["x"]) & np.isfinite(tp["y"]) & np.isfinite(tp["z"])]
        keep, gr, pl = split(cp, zones[s], s, gp)
        no_ground.append(cp[keep]); ground.append(cp[gr]); planes.append(pl)
    return np.concatenate(no_ground), np.concatenate(ground), planes


def run(sensors, zones, params, gp, cm=None):
    n_total = sum(c.n for c in sensors)
    own = cm is None
    if own:
        cm = capi.CloudMerger(max_points_total=n_total, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY)
    try:
        cm.set_ground_removal(capi.make_ground_params(zones, gp["max_iterations"], gp["threshold"], gp["probability"],
                                                      gp["optimize"], gp["z_keep_max"], gp["seed"],
                                                      gp.get("outlier_radius", 0.0), gp.get("outlier_min_neighbors", 1)))
        cm.submit_all(sensors)
        res = cm.merge_voxelize(params)
        out = cm.result(res.n_out)
        cells, counts = cm.cells(res.n_out) if res.status == capi.OK else (None, None)
        merged = cm.merged(n_total)
        ground = cm.ground(n_total)
        planes = cm.ground_planes()
        return dict(res=res, out=out, cells=cells, counts=counts, merged=merged, ground=ground, planes=planes)
    finally:
        if own:
            cm.close()


def a4(a):
    return np.stack([a["x"], a["y"], a["z"], a["intensity"]], 1)


def check(sensors, zones, params, gp=GP, split=oracle.ground_split, centroids_close=assert_centroids_close, exact_planes=False):
    """exact_planes: hold the planes to bit-equality instead of 1e-6 (always possible with optimize off)."""
    want_ng, want_g, want_planes = expected(sensors, zones, params, gp, split)
    g = run(sensors, zones, params, gp)
    g["plane_diff"] = max([np.abs(np.array(g["planes"][s * 8 + k].plane) - np.array(pl.plane)).max()
                           for s, pls in enumerate(want_planes) for k, pl in enumerate(pls) if pl is not None and pl.found],
                          default=0.0)
    print(f"ground planes: largest difference from the definition {g['plane_diff']:.3e}")
    assert same_bits(a4(g["merged"]), xyzi_of(want_ng)), "no-ground cloud (content and order)"
    assert same_bits(a4(g["ground"]), xyzi_of(want_g)), "ground cloud (content and order)"
    for s, pls in enumerate(want_planes):
        for k, pl in enumerate(pls):
            got = g["planes"][s * 8 + k]
            if pl is None:
                assert got.band_points == 0 and got.found == 0
                continue
            assert got.found == pl.found and got.inliers == pl.n_inliers and got.iterations == pl.iterations, (s, k)
            assert got.band_points == pl.band_points, (s, k)
            if pl.found:
                assert np.abs(np.array(got.plane) - np.array(pl.plane)).max() <= 1e-6
                if exact_planes:
                    assert same_bits(np.array(got.plane, np.float32), np.array(pl.plane, np.float32)), (s, k, list(got.plane), pl.plane)
    for s in range(capi.MAX_SENSORS):                                # no record of a slab or sensor the frame does not have
        for k in range(len(want_planes[s]) if s < len(want_planes) else 0, capi.MAX_ZONES):
            got = g["planes"][s * capi.MAX_ZONES + k]
            assert got.band_points == 0 and got.found == 0 and got.inliers == 0, (s, k)
    st, vox, rep = oracle.voxelgrid(want_ng, params.leaf, params.min_points_per_voxel, stable=True)
    assert g["res"].status == st and g["res"].n_out == len(vox) and g["res"].n_merged == len(want_ng)
    if st == oracle.OK:
        assert np.array_equal(g["cells"], rep.cells) and np.array_equal(g["counts"], rep.counts)
        centroids_close(a4(g["out"]), xyzi_of(vox))
    return g, want_planes


def test_front_sensor_five_slabs():
    rng = np.random.default_rng(21)
    sensors = [xyzi_cloud(scene(rng, 120_000), rng.uniform(0, 255, 120_000))]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    g, planes = check(sensors, [FRONT], params)
    for pl in planes[0]:                      # the fitted planes are the scene's ground: z = -0.05 + 0.01 x + 0.02 y
        n = np.array(pl.plane[:3]) * np.sign(pl.plane[2])
        assert pl.found and abs(n[0] / n[2] + 0.01) < 2e-3 and abs(n[1] / n[2] + 0.02) < 5e-3
    assert 0 < len(g["ground"]) < 120_000 and len(g["ground"]) + len(g["merged"]) <= 120_000
    if g["res"].path_flags & 1:             # (the bucket path needs the lane-ordered LDS ranking the device probe looks for)
        assert g["res"].path_flags & 2      # with the ROI fixing the grid the voxel stage runs on the bucket path (CM_PATH_BUCKET)


def test_four_sensors_with_poses_keep_all_slab_and_gaps():
    rng = np.random.default_rng(22)
    sensors = []
    for s in range(4):
        xyz = scene(rng, 60_000)
        q = synth.yaw_quaternion(0.02 * (s - 1.5))
        t = np.array([0.3 * s, -0.2 * s, 0.05 * s])
        # put the scene into the sensor frame so that the transform brings it back (roughly) to the vehicle frame
        from scipy.spatial.transform import Rotation as R
        rot = R.from_quat(q).as_matrix()
        local = ((xyz.astype(np.float64) - t) @ rot).astype(np.float32)
        sensors.append(xyzi_cloud(local, rng.uniform(0, 255, len(local)), q_xyzw=q, t_xyz=t))
    zones = [FRONT,
             [(20.0, 40.0, 1.0), (-15.0, 35.0, -1.0)],             # top-middle: one plane slab, one slab kept whole (:436-444)
             [(34.0, 26.0, 1.5), (24.0, 10.0, 1.2), (14.0, 10.0, 0.8), (4.0, 10.0, 0.5)],   # Livox (:475-497): nothing behind x = 4
             [(30.0, 30.0, 2.0), (4.0, 26.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]]   # proceedRear
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    check(sensors, zones, params)


def test_sample_planes_without_refit_are_bit_exact():
    """optimize_coefficients off: the reported plane is the best sample's own fp32 plane (cross product, square
    root, divisions — PCL's operation order), so it must equal the oracle's bit for bit, slab after slab."""
    rng = np.random.default_rng(31)
    sensors = [xyzi_cloud(scene(rng, 30_000, tilt=0.013 * (s + 1), ground_sigma=0.04), rng.uniform(0, 255, 30_000)) for s in range(6)]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    n_planes = 0
    for it, iters in enumerate((1, 3, 25)):
        gp = dict(GP, optimize=False, max_iterations=iters, threshold=0.05, seed=99 + it)
        g, planes = check(sensors, [FRONT] * 6, params, gp)
        for s, pls in enumerate(planes):
            for k, pl in enumerate(pls):
                if pl is not None and pl.found:
                    n_planes += 1
                    got = np.array(g["planes"][s * 8 + k].plane, np.float32)
                    assert same_bits(got, np.array(pl.plane, np.float32)), (iters, s, k, got, pl.plane)
    assert n_planes >= 60


# 90 % of the points are clutter inside every slab's band (z from -0.45 to 0.25, the ground at about -0.05 + 0.01 x):
# with a 1.5 cm threshold few samples are all ground, the stopping rule asks for thousands of hypotheses and every slab
# runs to max_iterations. kg_ransac scores hypotheses 32 and later itself (kg_score0 only the first 32).
def clutter_scene(seed, n_sensors=2, n=70_001):
    rng = np.random.default_rng(seed)
    return [xyzi_cloud(scene(rng, n, obj_frac=0.9, obj_z=(-0.45, 0.25)), rng.uniform(0, 255, n)) for _ in range(n_sensors)]


def test_cluttered_bands_run_past_the_first_round():
    sensors = clutter_scene(37)
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    gp = dict(GP, threshold=0.015, max_iterations=1000)
    g, planes = check(sensors, [FRONT] * len(sensors), params, gp)
    iters = [pl.iterations for pls in planes for pl in pls if pl is not None and pl.found]
    assert sum(it > 32 for it in iters) >= 2, iters
    assert len(g["ground"]) > 0


def test_cluttered_sample_planes_without_refit_are_bit_exact():
    sensors = clutter_scene(38)
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    gp = dict(GP, optimize=False, threshold=0.02, max_iterations=150, seed=7)
    g, planes = check(sensors, [FRONT] * len(sensors), params, gp)
    n_long = 0
    for s, pls in enumerate(planes):
        for k, pl in enumerate(pls):
            assert pl is not None and pl.found
            n_long += pl.iterations > 32
            got = np.array(g["planes"][s * 8 + k].plane, np.float32)
            assert same_bits(got, np.array(pl.plane, np.float32)), (s, k, got, pl.plane)
    assert n_long >= 2


def test_empty_frame_after_a_ground_frame_reports_no_planes():
    rng = np.random.default_rng(33)
    full = [xyzi_cloud(scene(rng, 20_000), rng.uniform(0, 255, 20_000))]
    empty = [xyzi_cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    with capi.CloudMerger(max_points_total=20_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        g = run(full, [FRONT], params, GP, cm=cm)
        assert any(p.found for p in g["planes"])
        g = run(empty, [FRONT], params, GP, cm=cm)
        assert g["res"].status == capi.EMPTY_INPUT and len(g["ground"]) == 0 and len(g["merged"]) == 0
        assert not any(p.found or p.band_points or p.inliers for p in g["planes"])


def test_slab_tables_follow_the_sensor_number_when_a_slot_is_empty():
    """Sensor 0 has not delivered anything (the live node's optional top-middle Velodyne at start-up): sensors 1 and
    2 must still be cut by THEIR slab tables, and their planes reported under their own numbers."""
    rng = np.random.default_rng(35)
    clouds = {1: xyzi_cloud(scene(rng, 40_000), rng.uniform(0, 255, 40_000)),
              2: xyzi_cloud(scene(rng, 30_000, tilt=-0.02), rng.uniform(0, 255, 30_000))}
    zones = [[(20.0, 40.0, 1.0)], FRONT, [(34.0, 26.0, 1.5), (4.0, 30.0, 0.5)]]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    want_ng, want_g, want_planes = [], [], {}
    for slot, c in clouds.items():
        pts = oracle.make_points(np.stack([c.data["x"], c.data["y"], c.data["z"]], 1), c.data["intensity"])
        cp = oracle.crop(oracle.transform(pts, oracle.quat_to_matrix(c.q_xyzw, c.t_xyz)), params.crop_min, params.crop_max)
        keep, gr, pl = oracle.ground_split(cp, zones[slot], slot, GP)
        want_ng.append(cp[keep]); want_g.append(cp[gr]); want_planes[slot] = pl
    with capi.CloudMerger(max_points_total=70_000, max_sensors=3, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params(zones, GP["max_iterations"], GP["threshold"], GP["probability"],
                                                      GP["optimize"], GP["z_keep_max"], GP["seed"]))
        for slot, c in clouds.items():
            cm.set_transform(slot, c.q_xyzw, c.t_xyz)
            cm.submit(slot, c)
        res = cm.merge_voxelize(params)
        assert res.status == capi.OK and res.n_sensors == 2
        assert same_bits(a4(cm.merged(70_000)), xyzi_of(np.concatenate(want_ng)))
        assert same_bits(a4(cm.ground(70_000)), xyzi_of(np.concatenate(want_g)))
        planes = cm.ground_planes()
    assert not any(planes[k].band_points for k in range(8))          # sensor 0: nothing
    for slot, pls in want_planes.items():
        for k, pl in enumerate(pls):
            got = planes[slot * 8 + k]
            assert pl is not None and got.found == pl.found and got.inliers == pl.n_inliers
            assert np.abs(np.array(got.plane) - np.array(pl.plane)).max() <= 1e-6


def test_band_outlier_filter_per_slab():
    """removeGround's outlierRemoval(:119): of a slab's band points that are not ground, those without a neighbour
    within 0.15 m (in the same slab's set) go. Sparse clutter in the band makes many of them lonely; two points
    that are close to each other but sit in different slabs do not save each other."""
    rng = np.random.default_rng(25)
    ground = scene(rng, 60_000, obj_frac=0.0)
    clutter = np.stack([rng.uniform(-15, 60, 6_000), rng.uniform(-5, 5, 6_000), rng.uniform(0.45, 2.4, 6_000)], 1)
    pair = np.array([[18.95, 0.0, 1.0], [19.05, 0.0, 1.0]])           # 10 cm apart, slab border at x = 19 between them
    xyz = np.concatenate([ground, clutter, pair]).astype(np.float32)
    sensors = [xyzi_cloud(xyz, rng.uniform(0, 255, len(xyz)))]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    gp = dict(GP, outlier_radius=0.15, outlier_min_neighbors=1)
    g, _ = check(sensors, [FRONT], params, gp)
    g0, _ = check(sensors, [FRONT], params, GP)
    assert len(g["merged"]) < len(g0["merged"]) and len(g["ground"]) == len(g0["ground"])
    got = a4(g["merged"])
    assert not ((np.abs(got[:, 0] - 18.95) < 1e-4) & (got[:, 2] == 1.0)).any()      # the pair: each alone in its slab
    assert not ((np.abs(got[:, 0] - 19.05) < 1e-4) & (got[:, 2] == 1.0)).any()


def test_degenerate_bands():
    """Empty band, two-point band (no model: nothing is ground), and a band of exactly collinear points (every
    sample is skipped: no plane either)."""
    rng = np.random.default_rng(23)
    above = np.stack([rng.uniform(0, 10, 500), rng.uniform(-2, 2, 500), rng.uniform(1.0, 2.0, 500)], 1)
    two = np.array([[12.0, 0.0, 0.0], [13.0, 1.0, 0.1]])
    line = np.stack([np.linspace(21.0, 29.0, 64), np.zeros(64), np.zeros(64)], 1)
    xyz = np.concatenate([above, two, line]).astype(np.float32)
    sensors = [xyzi_cloud(xyz, np.arange(len(xyz), dtype=np.float32))]
    zones = [[(0.0, 10.0, 0.5), (10.0, 10.0, 0.5), (20.0, 10.0, 0.5)]]
    params = MergeParams(leaf=(0.2,) * 3, min_points_per_voxel=0, **ROI)
    g, planes = check(sensors, zones, params)
    assert [p.found for p in planes[0]] == [0, 0, 0]
    assert len(g["ground"]) == 0 and len(g["merged"]) == len(xyz)


def test_general_path_gives_the_same(monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    rng = np.random.default_rng(26)
    sensors = [xyzi_cloud(scene(rng, 50_000), rng.uniform(0, 255, 50_000))]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    g, _ = check(sensors, [FRONT], params, dict(GP, outlier_radius=0.15))
    assert g["res"].path_flags & 2 == 0


def test_off_and_repeatable():
    rng = np.random.default_rng(24)
    sensors = [xyzi_cloud(scene(rng, 40_000), rng.uniform(0, 255, 40_000))]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    with capi.CloudMerger(max_points_total=40_000, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        a = run(sensors, [FRONT], params, GP, cm=cm)
        b = run(sensors, [FRONT], params, GP, cm=cm)
        assert same_bits(a4(a["out"]), a4(b["out"])) and same_bits(a4(a["ground"]), a4(b["ground"]))
        cm.set_ground_removal(None)
        cm.submit_all(sensors)
        res = cm.merge_voxelize(params)
        st, _, _, rep = oracle.merge_voxelize(sensors, params, stable=True)
        assert res.n_out == rep.n_out and res.n_merged == rep.n_merged
        with pytest.raises(capi.CloudMergeError):
            cm.ground(10)


def test_argument_checks():
    sensors, params = synth.config2(n_per_sensor=1000)
    with capi.CloudMerger(max_points_total=4000, max_sensors=4) as cm:
        g = capi.make_ground_params([FRONT])
        g.max_iterations = 0
        with pytest.raises(capi.CloudMergeError):
            cm.set_ground_removal(g)
        g = capi.make_ground_params([FRONT])
        g.outlier_radius = -1.0
        with pytest.raises(capi.CloudMergeError):
            cm.set_ground_removal(g)
        cm.set_ground_removal(capi.make_ground_params([FRONT]))
        params.outlier_radius = 0.15
        cm.submit_all(sensors)
        with pytest.raises(capi.CloudMergeError) as e:
            cm.merge_voxelize(params)
        assert e.value.status == capi.BAD_ARG
