"""The ground stage (cm_kernels_ground.hip and the band radius filter behind it) on tests/ground_edge_frames.py's
frames, through the C-ABI, on the route the library picks (the bucket path where a crop box fixes the grid) and with
CM_PATH=classic. Expectations come from tests/ground_ref.py, which tests/test_ground_ref.py ties to the oracle on the
CPU: no-ground and ground clouds bit-exact in content and order; found, inliers, iterations and band_points of every
slab equal; planes bit for bit, refit on or off (both sides add in the same fixed order: DESIGN.md §10); the voxel
grid of the no-ground cloud with tests/test_ground.py's bars; nothing reported for slabs and sensors a frame does not
have. Then the state a context carries from one frame to the next."""
import dataclasses

import numpy as np
import pytest

from cloud_merger_amd import capi
from oracle import oracle
from tests import ground_edge_frames as gf
from tests import ground_ref as gr
from tests import test_ground as tg
from tests.util import assert_centroids_close, same_bits

pytestmark = pytest.mark.gpu

FRAMES = {f.name: f for f in gf.all_frames()}
_REF = {}


def ref_split(points, zones, sensor, gp):
    """ground_ref.ground_split, computed once per (cloud, table, numbers): the routes and the context tests share it"""
    key = (points.tobytes(), repr(zones), sensor, repr(sorted(gp.items())))
    if key not in _REF:
        _REF[key] = gr.ground_split(points, zones, sensor, gp)
    return _REF[key]


def centroids_close_by_class(got, want):
    """assert_centroids_close where the expected intensity is finite; NaN for NaN and the same infinity elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    fin = np.isfinite(want[:, 3])
    assert_centroids_close(got[fin], want[fin])
    assert np.abs(got[~fin, :3] - want[~fin, :3]).max(initial=0.0) <= 1e-4
    assert np.array_equal(np.isnan(got[~fin, 3]), np.isnan(want[~fin, 3]))
    inf = ~fin & np.isinf(want[:, 3])
    assert np.array_equal(got[inf, 3], want[inf, 3])


def check_frame(f, **kw):
    special = f.name.startswith("special_values")
    return tg.check(f.sensors, f.zones, f.params, f.gp, split=ref_split, exact_planes=True,
                    centroids_close=centroids_close_by_class if special else assert_centroids_close, **kw)


@pytest.mark.parametrize("route", ["default", "classic"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_edge_frame(name, route, monkeypatch):
    if route == "classic":
        monkeypatch.setenv("CM_PATH", "classic")
    f = FRAMES[name]
    g, planes = check_frame(f)
    if route == "classic" or f.params.crop_min is None:
        assert g["res"].path_flags & 2 == 0
    print(f"{name} / {route}: path_flags {g['res'].path_flags:#x}")   # (which route the library picked: tests/test_route_policy.py)
    if name == "all_ground":                 # the voxel grid's answer for an empty cloud, and every point in the ground cloud
        st, vox, _ = oracle.voxelgrid(oracle.make_points(np.zeros((0, 3), np.float32)), f.params.leaf, 0, stable=True)
        assert g["res"].status == st == oracle.EMPTY_INPUT and g["res"].n_out == 0 and g["res"].n_merged == 0
        assert len(g["ground"]) == f.n_points and len(g["merged"]) == 0
    if name == "no_band":
        assert len(g["ground"]) == 0 and 0 < len(g["merged"]) < f.n_points
        assert not any(p.band_points or p.found or p.iterations for p in g["planes"])
    if name == "no_zones_sensor":
        assert not any(g["planes"][k].band_points for k in range(8)) and g["res"].n_sensors == 2
    if name == "filter":
        g0, _ = tg.check(f.sensors, f.zones, f.params, dict(f.gp, outlier_radius=0.0), split=ref_split, exact_planes=True)
        lonely = 2 * len(f.lattice) + len(f.pair) + 2 * len(f.shared)
        assert len(g0["merged"]) - len(g["merged"]) >= lonely and same_bits(tg.a4(g0["ground"]), tg.a4(g["ground"]))


def same_run(a, b):
    assert (a["res"].status, a["res"].n_out, a["res"].n_merged) == (b["res"].status, b["res"].n_out, b["res"].n_merged)
    assert same_bits(tg.a4(a["merged"]), tg.a4(b["merged"])), "no-ground cloud"
    assert same_bits(tg.a4(a["ground"]), tg.a4(b["ground"])), "ground cloud"
    for k, (p, q) in enumerate(zip(a["planes"], b["planes"])):
        assert bytes(p) == bytes(q), ("plane record", k, list(p.plane), list(q.plane), p.band_points, q.band_points,
                                      p.inliers, q.inliers, p.iterations, q.iterations, p.found, q.found)
    # the voxel stage behind: the same voxels; centroids within the suite's bar (a context's later frames may add a
    # voxel's points in another fixed order than its first frame: tests/util.py)
    if a["res"].status == capi.OK:
        assert np.array_equal(a["cells"], b["cells"]) and np.array_equal(a["counts"], b["counts"])
    centroids_close_by_class(tg.a4(a["out"]), tg.a4(b["out"]))
    return True


@pytest.mark.parametrize("route", ["default", "classic"])
def test_special_points_that_vanish_change_nothing(route, monkeypatch):
    if route == "classic":
        monkeypatch.setenv("CM_PATH", "classic")
    a, b = gf.special_values_frame(True), gf.special_values_frame(False)
    assert a.n_points - b.n_points == a.n_vanishing == 18
    assert same_run(tg.run(a.sensors, a.zones, a.params, a.gp), tg.run(b.sensors, b.zones, b.params, b.gp))


# ---- what a context carries from frame to frame ---------------------------------------------------------------------------
def frame_on(cm, f):
    return tg.run(f.sensors, f.zones, f.params, f.gp, cm=cm)


def collect(cm, f):
    """one frame without touching the ground settings"""
    n = f.n_points
    cm.submit_all(f.sensors)
    res = cm.merge_voxelize(f.params)
    cells, counts = cm.cells(res.n_out) if res.status == capi.OK else (None, None)
    return dict(res=res, out=cm.result(res.n_out), cells=cells, counts=counts, merged=cm.merged(n), ground=cm.ground(n),
                planes=cm.ground_planes())


def ground_params(f, zones=None, **over):
    gp = dict(f.gp, **over)
    return capi.make_ground_params(zones if zones is not None else f.zones, gp["max_iterations"], gp["threshold"],
                                   gp["probability"], gp["optimize"], gp["z_keep_max"], gp["seed"],
                                   gp.get("outlier_radius", 0.0), gp.get("outlier_min_neighbors", 1))


def test_sixteen_sensors_then_two_leaves_no_plane_record_behind():
    big, small = FRAMES["small_bands_it33"], gf.ordinary_frame()
    fresh = tg.run(small.sensors, small.zones, small.params, small.gp)
    with capi.CloudMerger(max_points_total=max(big.n_points, small.n_points), max_sensors=16, flags=capi.FLAG_OCCUPANCY) as cm:
        first = frame_on(cm, big)
        assert first["planes"][127].found and sum(p.band_points > 0 for p in first["planes"]) >= 20
        # sensors 2 .. 15 deliver nothing new and have no slab table any more: their stale clouds ride along and vanish
        only_two = dataclasses.replace(small.params, required_sensor_mask=0b11)
        again = tg.run(small.sensors, small.zones, only_two, small.gp, cm=cm)
        assert again["res"].n_sensors == 16
    assert same_run(again, fresh)
    assert not any(bytes(again["planes"][k]) != bytes(capi.GroundPlane()) for k in range(16, 128))
    assert all(again["planes"][k].found for k in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12))


def test_all_ground_frame_then_an_ordinary_one():
    empty, f = FRAMES["all_ground"], gf.ordinary_frame()
    fresh = tg.run(f.sensors, f.zones, f.params, f.gp)
    with capi.CloudMerger(max_points_total=f.n_points, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        first = frame_on(cm, empty)
        assert first["res"].status == capi.EMPTY_INPUT and len(first["ground"]) == empty.n_points
        assert same_run(frame_on(cm, f), fresh)


def test_new_tables_then_a_new_seed_between_two_frames():
    f = FRAMES["small_bands_it33"]
    other = [[(x0 + 0.25, ln, zm) for x0, ln, zm in z[::-1]] for z in f.zones]
    seeded = gf.GroundFrame("seeded", f.sensors, f.zones, f.params, dict(f.gp, seed=777), f.purpose)
    fresh = tg.run(seeded.sensors, seeded.zones, seeded.params, seeded.gp)
    with capi.CloudMerger(max_points_total=f.n_points, max_sensors=16, flags=capi.FLAG_OCCUPANCY) as cm:
        first = frame_on(cm, f)
        cm.set_ground_removal(ground_params(f, zones=other))
        cm.set_ground_removal(ground_params(f, seed=777))
        second = collect(cm, f)
        assert same_run(second, fresh)
        assert bytes(second["planes"]) != bytes(first["planes"])                       # the seed matters on this frame
        cm.set_ground_removal(ground_params(f, zones=other))                           # and the other tables alone
        third = collect(cm, f)
    moved = gf.GroundFrame("moved", f.sensors, other, f.params, f.gp, f.purpose)
    assert same_run(third, tg.run(moved.sensors, moved.zones, moved.params, moved.gp))
    tg.check(moved.sensors, moved.zones, moved.params, moved.gp, split=ref_split, exact_planes=True)


def test_stage_off_and_on_again():
    f = gf.ordinary_frame()
    with capi.CloudMerger(max_points_total=f.n_points, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        first = frame_on(cm, f)
        cm.set_ground_removal(None)
        cm.submit_all(f.sensors)
        res = cm.merge_voxelize(f.params)
        st, _, _, rep = oracle.merge_voxelize(f.sensors, f.params, stable=True)
        assert res.status == st and res.n_out == rep.n_out and res.n_merged == rep.n_merged > first["res"].n_merged
        with pytest.raises(capi.CloudMergeError):
            cm.ground(10)
        assert same_run(frame_on(cm, f), first)
