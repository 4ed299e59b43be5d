"""Frames for tests/test_quantile_edges.py: clouds whose kept records fall into the quantile buckets of the previous frame
in exactly the numbers a case asks for. The generator is driven by tests/quantile_model.py's splitters; whether a frame
really has the populations is established from the oracle's merged cloud, not here.

Geometry: leaf 0.0625 m (exact in fp32), crop box +-32, +-32, +-8 m: 1025 x 1025 x 257 cells, a 29-bit index. Identity
poses. A voxel is named by its number u among the 1024 x 1024 x 256 cells that lie wholly inside the box, x fastest and
z slowest, so the order of u is the order of the device's index (and of the model's keys). Points sit at the centre of their
cell plus a seeded jitter of at most a quarter leaf — no point is near a face (faces are tests/test_edge_values.py's
business) — with seeded intensities: fp32 sums of a handful of them depend on the order they are added in, so the
bit-exact rule for voxels of up to 17 points bites on the stability of every pass. CORNER names the box's very last cell
(its largest index), which only points ON the box's max corner reach."""
from dataclasses import dataclass

import numpy as np

from cloud_merger_amd.types import MergeParams, SensorCloud, XYZI_DTYPE
from tests import quantile_model as qm

LEAF = 0.0625
CROP_MIN, CROP_MAX = (-32.0, -32.0, -8.0), (32.0, 32.0, 8.0)
NX, NY, NZ = 1024, 1024, 256
LO = np.array([-512, -512, -128], dtype=np.int64)
U_END = NX * NY * NZ
CORNER = U_END                                   # pseudo-number of cell (512, 512, 128)
BOX_DIV = (1025, 1025, 257)                      # cells of the crop box per axis (floor(max / leaf) - floor(min / leaf) + 1)
KEY_BITS = 29                                    # width of 1025 * 1025 * 257 - 1
FIXED_LOW_BITS = KEY_BITS - 16                   # the fixed-grid route sorts 2 x 8 high bits globally, the finish the rest
FINISH_TILE, FINISH_CAP = 2048, 4032             # records per finish tile of the fixed-grid route / what it holds with a tail


def params(min_pts=0, crop=True):
    return MergeParams(leaf=(LEAF,) * 3, min_points_per_voxel=min_pts, crop_min=CROP_MIN if crop else None,
                       crop_max=CROP_MAX if crop else None)


def cells_of_u(u):
    u = np.asarray(u, dtype=np.int64).reshape(-1)
    c = np.stack([u % NX, (u // NX) % NY, u // (NX * NY)], axis=1) + LO
    c[u == CORNER] = (512, 512, 128)
    return c


def u_of_key(key):
    """Model key -> voxel number; `no bucket` and the corner cell -> U_END (beyond every interior cell)."""
    if key >= qm.NO_BUCKET:
        return U_END
    c = qm.cells_of_keys([key])[0] - LO
    if c[0] >= NX or c[1] >= NY or c[2] >= NZ:
        assert tuple(c) == (NX, NY, NZ), "a splitter on the box's rim that is not its corner"
        return U_END
    return int((c[2] * NY + c[1]) * NX + c[0])


def bucket_ranges(spl):
    """[lo, hi) in voxel numbers of every bucket: the voxel AT lo is the splitter, hi - 1 the last key below the next one."""
    us = [0] + [u_of_key(int(s)) for s in spl[1:]] + [U_END]
    return [(us[t], us[t + 1]) for t in range(len(spl))]


def small(pop, rng, longest=3):
    """Voxel lengths of 1..longest records that add up to pop."""
    out = []
    while pop > 0:
        k = int(min(pop, rng.integers(1, longest + 1)))
        out.append(k)
        pop -= k
    return out


def place(lo, hi, m):
    """m distinct voxel numbers in [lo, hi): the first AT lo, the last AT hi - 1, the rest spread evenly between them — and,
    where there is room, off x = -512, so that the cell in front of a voxel that becomes a splitter lies inside the box."""
    assert hi - lo >= m, f"{m} voxels do not fit [{lo}, {hi})"
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    if m == 1:
        return np.array([lo], dtype=np.int64)
    pos = lo + (np.arange(m, dtype=np.int64) * (hi - 1 - lo)) // (m - 1)
    if (hi - 1 - lo) // (m - 1) >= 3:
        inner = (pos % NX == 0) & (pos != lo) & (pos != hi - 1)
        pos[inner] += 1
    return pos


def design(spl, want, rng, ordinary=1800):
    """Voxels (numbers, lengths) of a frame with the wanted records per bucket under the splitters spl.
    want: {bucket: population or list of voxel lengths in key order}; a bucket that is not named gets `ordinary` records in
    small voxels (0 where two equal splitters leave it no room). Every bucket that holds two voxels or more has one AT its
    splitter and one at the last key below the next splitter; a bucket of one voxel has it at the splitter."""
    us, ls = [], []
    for t, (lo, hi) in enumerate(bucket_ranges(spl)):
        spec = want.get(t, ordinary)
        if hi <= lo:
            assert (spec == ordinary and t not in want) or spec in (0, []), f"bucket {t} has no room"
            continue
        if not isinstance(spec, (list, tuple)):
            spec = small(min(spec, 3 * (hi - lo)) if t not in want else spec, rng)
            if len(spec) > hi - lo:                 # (a narrow bucket: fewer, longer voxels)
                pop, room = sum(spec), hi - lo
                spec = [pop // room + (1 if i < pop % room else 0) for i in range(room)]
        us.append(place(lo, hi, len(spec)))
        ls.append(np.asarray(spec, dtype=np.int64))
    return np.concatenate(us), np.concatenate(ls)


def spread(lengths, lo=1, hi=U_END):
    """Voxels of these lengths spread evenly over [lo, hi)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    return place(lo, hi, len(lengths)), lengths


@dataclass
class Frame:
    sensors: list
    params: MergeParams
    n_in: int
    n_kept: int                      # the generator's intent (the tests take the truth from the oracle)
    crop: bool = True
    note: str = ""


def clouds(u, lengths, seed, kept_per_sensor=None, junk=0.0, min_pts=0, crop=True, note=""):
    """The voxels as sensor clouds. A global seeded shuffle deals the records of every voxel across the sensors and across
    the 4096-slot tiles of a sensor. kept_per_sensor: kept records per sensor (None: two sensors, half each; a 0 leaves a
    sensor without points). junk: this many NaN / out-of-box points per kept record (fewer than half of the points, so the
    crop does not make the frame a packed one), shuffled in."""
    assert 0.0 <= junk < 1.0
    rng = np.random.default_rng(seed)
    u = np.asarray(u, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert len(np.unique(u)) == len(u), "voxel numbers must be distinct"
    n = int(lengths.sum())
    of = np.repeat(np.arange(len(u)), lengths)
    cells = cells_of_u(u)[of].astype(np.float64)
    xyz = (cells + 0.5 + rng.uniform(-0.25, 0.25, size=(n, 3))) * LEAF
    on_corner = (u == CORNER)[of]
    xyz[on_corner] = CROP_MAX
    pts = np.zeros(n, dtype=XYZI_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0].astype(np.float32), xyz[:, 1].astype(np.float32), xyz[:, 2].astype(np.float32)
    pts["intensity"] = rng.uniform(0.0, 255.0, size=n).astype(np.float32)
    pts = pts[rng.permutation(n)]
    if kept_per_sensor is None:
        kept_per_sensor = [n - n // 2, n // 2]
    assert sum(kept_per_sensor) == n, (sum(kept_per_sensor), n)
    sensors, at = [], 0
    for k in kept_per_sensor:
        part = pts[at:at + k]
        at += k
        nj = int(junk * k)
        if nj:
            bad = np.zeros(nj, dtype=XYZI_DTYPE)
            for f in ("x", "y", "z"):
                bad[f] = rng.uniform(-7.0, 7.0, size=nj).astype(np.float32)
            bad["intensity"] = rng.uniform(0.0, 255.0, size=nj).astype(np.float32)
            which = rng.integers(0, 6, size=nj)
            bad["x"][which == 0] = np.nan
            bad["y"][which == 1] = np.nan
            bad["z"][which == 2] = np.nan
            bad["x"][which == 3] = np.float32(32.03125)        # half a cell beyond the box
            bad["y"][which == 4] = np.float32(-40.0)
            bad["z"][which == 5] = np.float32(8.5)
            part = np.concatenate([part, bad])[rng.permutation(k + nj)]
        sensors.append(SensorCloud(data=np.ascontiguousarray(part), n=len(part), is_dense=nj == 0))
    n_in = sum(s.n for s in sensors)
    return Frame(sensors=sensors, params=params(min_pts, crop), n_in=n_in, n_kept=n, crop=crop, note=note)


def box_keys(cells):
    """The device's index of absolute cells in the crop box's grid."""
    c = np.asarray(cells, dtype=np.int64) - LO
    return (c[:, 2] * BOX_DIV[1] + c[:, 1]) * BOX_DIV[0] + c[:, 0]


def fixed_grid_fits(cells):
    """Whether the fixed-grid route (two global 8-bit passes, then a finish over tiles of 2048 sorted records whose last
    bucket may run on to 4032) takes the frame without handing it back itself: every bucket of 2^13 neighbouring indices
    must end within 4032 records of the start of the tile it begins in. A frame that fails this ends on the general path,
    which leaves no splitters."""
    k = np.sort(box_keys(cells)) >> FIXED_LOW_BITS
    start = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    count = np.diff(np.r_[start, len(k)])
    return bool(((start % FINISH_TILE) + count <= FINISH_CAP).all())
