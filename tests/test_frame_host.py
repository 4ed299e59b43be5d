"""tests/frame_host.py against the oracle: the fused cloud it makes of a frame equals the oracle's merged cloud bit for bit on
every layout of tests/layouts.py. This is what makes frame_host an input for the by-product tests that is independent of the
kernels (tests/test_byproduct_layouts.py). No GPU and no library.

The scene: three sensors with their own rotations and translations, points within 12 m, and by hand NaN and infinite
coordinates, a NaN intensity with a payload, signed zeros and points outside the crop box. With a crop box the oracle drops
what is not finite, as every kernel's point_valid does; without one it passes such points on to the voxel grid (PCL's
concatenation keeps them), so that run has finite points only."""
import numpy as np
import pytest

from cloud_merger_amd.types import MergeParams
from oracle import oracle
from tests import frame_host as fh
from tests import layouts as wl
from tests.util import xyzi_of

F32 = np.float32
POSES = [((0.0, 0.0, 0.0, 1.0), (1.5, -0.25, 0.5)),
         ((0.0, 0.0, 0.38268343236508978, 0.92387953251128674), (-2.0, 3.0, 0.25)),              # 45 degrees about z
         ((0.18257418583505536, 0.36514837167011072, 0.54772255750516607, 0.73029674334022143), (0.5, 4.0, -0.75))]
COUNTS = [700, 1, 533]
CROP = dict(crop_min=(-9.0, -10.0, -3.0), crop_max=(10.0, 9.0, 4.0))
NAN_PAYLOAD = 0x7FC12345


def scene(special):
    """Per sensor (xyz, intensity) in its own frame."""
    rng = np.random.default_rng(17)
    out = []
    for s, n in enumerate(COUNTS):
        xyz = rng.uniform(-12.0, 12.0, (n, 3)).astype(F32)
        inten = rng.uniform(0.0, 255.0, n).astype(F32)
        if special and n > 20:
            xyz[3, 0] = np.nan
            xyz[5, 1] = np.inf
            xyz[7, 2] = -np.inf
            xyz[9] = (-0.0, -0.0, -0.0)
            xyz[11] = (0.0, -0.0, 0.0)
            xyz[13] = (40.0, 0.0, 0.0)                                    # outside the crop box whatever the pose
            inten[15] = np.uint32(NAN_PAYLOAD).view(F32)
            inten[17] = -0.0
        out.append((xyz, inten))
    return out


def clouds_in(layout, parts, seed=0):
    rng = np.random.default_rng(seed + sum(map(ord, layout)))
    return [wl.repack(xyz, inten, layout, rng, q_xyzw=q, t_xyz=t) for (xyz, inten), (q, t) in zip(parts, POSES)]


def oracle_merged(clouds, params):
    st, merged, _, rep = oracle.merge_voxelize(clouds, params, threads=1, stable=True)
    assert st == oracle.OK and rep.n_merged == len(merged)
    return xyzi_of(merged)


def test_the_matrix_is_the_oracles():
    for q, t in POSES + [((0.5, -0.5, 0.5, 0.5), (1e-3, -0.0, 12345.678))]:
        assert fh.matrix_of(q, t).tobytes() == oracle.quat_to_matrix(q, t).tobytes()


@pytest.mark.parametrize("layout", list(wl.ALL))
@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
def test_the_fused_cloud_is_the_oracles(layout, crop):
    parts = scene(special=crop)
    params = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, **(CROP if crop else {}))
    clouds = clouds_in(layout, parts)
    fr = fh.fuse(clouds, params.crop_min, params.crop_max)
    want = oracle_merged(clouds, params)
    assert fr.A.dtype == F32 and fr.A.shape == want.shape and fr.A.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert fr.n_in == sum(COUNTS) and len(fr.sensor) == len(fr.index) == len(fr.A)
    assert fr.translations.tobytes() == np.array([t for _, t in POSES], F32).tobytes()
    # rows are in (sensor, point) order, and each is its sensor's point at its index
    assert (np.diff(fr.sensor) >= 0).all() and all((np.diff(fr.index[fr.sensor == s]) > 0).all() for s in range(3))
    if layout in wl.NO_INTENSITY:
        assert not fr.A[:, 3].view(np.uint32).any(), "a layout without the field gives intensity +0"
    else:
        # the same bytes XYZI16 gives, and the intensity's bits come through
        base = fh.fuse(clouds_in("xyzi16", parts, seed=1), params.crop_min, params.crop_max)
        assert base.A.view(np.uint32).tobytes() == fr.A.view(np.uint32).tobytes()
        k = np.flatnonzero((fr.sensor == 0) & (fr.index == 15))
        if crop and len(k):
            assert fr.A[k[0], 3].view(np.uint32) == NAN_PAYLOAD
    if crop:
        # the hand-placed points: dropped where not finite or outside the box, kept with their zeros' signs otherwise
        for s in (0, 2):
            kept = set(fr.index[fr.sensor == s].tolist())
            assert not kept & {3, 5, 7, 13}
        assert 0 < len(fr.A) < fr.n_in - 8
        assert fh.bounds(fr)[2] == len(fr.A)
        mn, mx, _ = fh.bounds(fr)
        assert (mn >= F32(CROP["crop_min"])).all() and (mx <= F32(CROP["crop_max"])).all()
    else:
        assert len(fr.A) == fr.n_in


def test_an_empty_frame():
    fr = fh.fuse(clouds_in("odd17", [(np.zeros((0, 3), F32), np.zeros(0, F32))] * 3))
    assert fr.A.shape == (0, 4) and fr.n_in == 0 and fh.bounds(fr)[2] == 0 and np.isinf(fh.bounds(fr)[0]).all()
