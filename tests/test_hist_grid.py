"""k4_hist as a grid-stride kernel (cm_kernels_v4.hip): a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...
in half-tiles, the launch holds what is resident at once (G workgroups: not part of the C-ABI; 3 or 2 workgroups per CU of
a 256-CU device give 768 or 512). Through the C-ABI against the CPU oracle, on the quantile route.

A frame only takes that route as the second or later frame of its context, on the same grid, when the fixed grid would
need two or more passes (cm_route.cpp): every case submits a first frame, then checks the second, and asserts
CM_PATH_QUANTILE and not CM_PATH_REDONE on the checked frame — a frame that silently ran the fixed-grid passes proves
nothing here. Bars as in tests/test_quantile.py: merged cloud and occupancy bit-exact, centroids bit-exact for voxels of up
to 17 points and within 1e-4 m beyond."""
import numpy as np
import pytest

from cloud_merger_amd import capi, synth
from cloud_merger_amd.types import MergeParams, SensorCloud, xyzi_cloud
from tests.test_layouts import (CROP, check_oracle, oracle_of, packed_frames, reference_of, run_stream, scene,
                                skip_without_bucket)
from tests.test_quantile import BUCKET, QUANTILE, REDONE, frame_against_oracle, needs_lds_rank
from tests.util import same_bits

pytestmark = pytest.mark.gpu

TILE = 4096                                   # CM_TILE


def cloud_of(seed, n, q=None, t=None):
    """n points of cfg2's scene statistics (70 % noisy ground plane, 30 % clutter, 28 m x 28 m x 6 m) in cfg2's pose s"""
    rng = np.random.default_rng(seed)
    xyz, inten = synth.ground_scene(rng, n, 14.0, -2.0, 4.0)
    return xyzi_cloud(xyz, inten, q_xyzw=synth.random_quaternion(rng) if q is None else q,
                      t_xyz=rng.uniform(-2, 2, 3) if t is None else t)


def sensors_of_tiles(n_tiles, seed):
    """four sensors with n_tiles padded tiles between them: sensor 0 ends on a tile of ONE point, sensor 1 on a tile of
    CM_TILE - 1 points, sensor 2 on a full tile, sensor 3 takes the rest and ends somewhere inside a tile"""
    per = n_tiles // 4
    tiles = [per, per, per, n_tiles - 3 * per]
    sizes = [(tiles[0] - 1) * TILE + 1, (tiles[1] - 1) * TILE + TILE - 1, tiles[2] * TILE, (tiles[3] - 1) * TILE + 1234]
    assert sum((n + TILE - 1) // TILE for n in sizes) == n_tiles
    return [cloud_of(seed + s, n) for s, n in enumerate(sizes)]


def second_frame(sensors, params, n_frames=2):
    """the same frame n_frames times on one context (its own quantiles: no bucket can overflow); the last one checked"""
    n = sum(s.n for s in sensors)
    with capi.CloudMerger(max_points_total=n, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY) as cm:
        for k in range(n_frames):
            if k < n_frames - 1:
                cm.submit_all(sensors)
                res = cm.merge_voxelize(params)
                assert res.status == capi.OK
                needs_lds_rank(res)
            else:
                res, rep = frame_against_oracle(cm, sensors, params, n)
    f = res.path_flags
    assert f & BUCKET and f & QUANTILE and not f & REDONE, f
    assert res.sort_passes == 1
    return res, rep


# The launch is min(n_tiles, G) workgroups. Sizes that straddle both plausible G (512, 768): a few tiles less, one more (the
# first workgroup alone takes a second tile), a few more; 1 600: two to four tiles per workgroup and no multiple of either G.
@pytest.mark.parametrize("n_tiles", [500, 513, 520, 760, 769, 780, 1600])
def test_tile_counts_around_the_resident_grid(n_tiles):
    """2 M to 6.5 M points at 5 cm, no crop box (the predicted box): ragged last tiles of 1, CM_TILE - 1 and 1234 points.
    (From 5.3 M records on the frame has more than 2048 buckets: k4_hist<12>, two buckets to a bin.)"""
    sensors = sensors_of_tiles(n_tiles, 4000 + n_tiles)
    # (shared bins: the first fixed-grid frame may itself be redone with a pass more — the third frame is the one to check)
    res, rep = second_frame(sensors, MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2), n_frames=3 if n_tiles > 1299 else 2)
    assert res.n_in == sum(s.n for s in sensors)


@pytest.mark.parametrize("n_points", [3, 100, TILE, TILE + 1, 2 * TILE])
def test_smallest_frames_that_take_the_route(n_points):
    """The fixed grid needs two passes for any index of more than 22 bits (cm_route.cpp bucket_passes: 14 bits are left to
    the local finish), whatever the number of points: at 5 cm in this scene's box even a frame of one tile, down to a
    few points, goes the quantile way from its second frame on. One and two workgroups; a last tile of one point."""
    rng = np.random.default_rng(11)
    # (two far corners keep the box — and with it the index width — of the full scene)
    xyz, inten = synth.ground_scene(rng, n_points, 14.0, -2.0, 4.0)
    xyz[0], xyz[1] = (-14.0, -14.0, -2.0), (14.0, 14.0, 4.0)
    sensors = [xyzi_cloud(xyz, inten)]
    res, rep = second_frame(sensors, MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=0))
    assert (res.n_in + TILE - 1) // TILE <= 2


def test_empty_sensor_between_two_others():
    """slot 1 holds a cloud of 0 points: its tile range is empty, the tiles behind it belong to slot 2"""
    a, b = cloud_of(21, 3 * TILE + 17), cloud_of(22, 2 * TILE + 4095)
    empty = SensorCloud(data=np.zeros(0, dtype=a.data.dtype), n=0, q_xyzw=a.q_xyzw, t_xyz=a.t_xyz)
    # (a crop box that keeps most points: one that drops more than half sends the frame to the packed fixed-grid passes)
    for params in (MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=0),
                   MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=0, crop_min=(-21.0, -22.0, -23.0), crop_max=(22.0, 21.0, 20.0))):
        res, rep = second_frame([a, empty, b], params)
        assert res.n_in == a.n + b.n


@pytest.mark.parametrize("crop", [False, True], ids=["predicted_box", "crop_box"])
@pytest.mark.parametrize("layout", ["xyzi16", "pcl32", "velo22"])
def test_wire_layouts_with_and_without_crop(layout, crop):
    """the two aligned loaders (twelve bytes per point, a half-tile ahead) and the generic one (fetched where it is used),
    on sensors whose sizes are no multiple of 64: the bits of the XYZI16 run, and the oracle"""
    base = scene()
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **(CROP if crop else {}))
    layouts = [layout] * len(base)
    ref = reference_of(base, layouts)
    n_cap = sum(s.n for s in base)
    got = run_stream([packed_frames(base, layouts, 5)] * 2, params, n_cap, len(base))
    want = run_stream([ref] * 2, params, n_cap, len(base))
    skip_without_bucket(got[-1]["flags"])
    for g, w in zip(got, want):
        assert g["flags"] == w["flags"]
        assert same_bits(g["merged"], w["merged"]) and same_bits(g["out"], w["out"])
        assert np.array_equal(g["cells"], w["cells"]) and np.array_equal(g["counts"], w["counts"])
    f = got[-1]["flags"]
    assert f & BUCKET and f & QUANTILE and not f & REDONE, f
    check_oracle(got[-1], oracle_of(("hist_grid", crop), ref, params), params.leaf)


def test_frame_that_leaves_its_predicted_box_is_handed_back_and_redone():
    """Frame 2 reaches 30 % further out than the box predicted from frames 0 and 1: k4_hist reports it (with the exact
    bounds folded from its per-tile records), the frame is redone with the fixed-grid passes — same result as the oracle."""
    n_per = 150_000
    with capi.CloudMerger(max_points_total=4 * n_per, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        flags = []
        for k, wide in enumerate((False, False, True, False, False)):
            sensors, params = synth.config2_stream(k, n_per_sensor=n_per, min_pts=2, wide=wide)
            res, rep = frame_against_oracle(cm, sensors, params, 4 * n_per)
            needs_lds_rank(res)
            flags.append(res.path_flags)
        assert flags[1] & QUANTILE and not flags[1] & REDONE, flags
        assert flags[2] & REDONE and not flags[2] & QUANTILE, flags
        assert any(f & QUANTILE and not f & REDONE for f in flags[3:]), flags


def test_smallest_frame_over_shared_bins():
    """More than 2048 buckets (two to a bin, k4_hist<12>) from 2048 x 2600 records on (cm_device.h cm_quant_buckets): four
    sensors of 1 331 201 points, every point valid — the smallest frame of equal sensors beyond it; 1 304 tiles."""
    n_per = (2048 * 2600) // 4 + 1
    sensors, params = synth.config2(n_per_sensor=n_per, min_pts=2)
    res, rep = second_frame(sensors, params, n_frames=3)
    assert rep.n_merged == 4 * n_per > 2048 * 2600
