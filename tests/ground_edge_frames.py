"""Frames for the zone-wise ground stage (cm_kernels_ground.hip) at the places typical scenes never reach: points on
(and one fp32 step beside) every slab and band limit, zone keys up to 127, bands of 0 .. 16 385 points in every mix
inside one 1024-point run of the sorted band, loops that end on the spare hypotheses, points at exactly the distance
threshold, frames without any band point / without any no-ground point, special values, a scene 1 km out, and the band
radius filter at exactly the radius.

Every builder returns a GroundFrame: sensors (cloud_merger_amd.types.SensorCloud), one slab table per sensor, the
MergeParams, the RANSAC numbers (gp, as tests/test_ground.py passes them) and what the frame is for. Expectations
come from tests/ground_ref.py; tests/test_ground_ref.py asserts on the restatement alone that each frame still holds
what it was built for."""
import numpy as np

from cloud_merger_amd.types import MergeParams, xyzi_cloud

F = np.float32
ROI = dict(crop_min=(-15.0, -5.0, -0.5), crop_max=(60.0, 5.0, 3.0))
GP = dict(max_iterations=1000, threshold=0.3, probability=0.99, optimize=True, z_keep_max=3.0, seed=12345)
YAW_PI = (0.0, 0.0, 1.0, 0.0)              # rotation matrix diag(-1, -1, 1) exactly


class GroundFrame:
    def __init__(self, name, sensors, zones, params, gp, purpose, **extra):
        self.name, self.sensors, self.zones, self.params, self.gp, self.purpose = name, sensors, zones, params, gp, purpose
        self.__dict__.update(extra)

    @property
    def n_points(self):
        return sum(c.n for c in self.sensors)

    def __repr__(self):
        return self.name


def step(v, k):
    """the fp32 value k steps above (k > 0) or below v"""
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf) if k > 0 else F(-np.inf))
    return F(v)


def ground_patch(rng, n, x_lo, x_hi, y=(-2.0, 2.0), tilt=0.01, sigma=0.02, z0=0.0):
    x = rng.uniform(x_lo, x_hi, n)
    return np.stack([x, rng.uniform(*y, n), z0 + tilt * (x - x_lo) + sigma * rng.standard_normal(n)], 1).astype(np.float32)


# ---- border_frame -----------------------------------------------------------------------------------------------------
X08 = float(F(F(0.1) + F(0.7)))           # slab 0's upper limit, an fp32 sum that is no binary fraction: slab 1 starts there
BORDER_ZONES = [(0.1, 0.7, 0.3),          # 0: [fl(0.1), fl(0.1)+fl(0.7)], zlo = fl32(double(fl(0.3)) + 0.01)
                (X08, 1.2, 0.0),          # 1: shares slab 0's upper limit; band z == 0 only
                (0.5, 0.2, 0.5),          # 2: wholly inside slab 0 — gets nothing
                (5.0, 0.0, 0.5),          # 3: x_length 0: x == 5 exactly
                (-4.0, 2.0, -1.0),        # 4: kept whole
                (-10.0, 4.0, 0.5),        # 5: out of x order
                (2.0, 3.0, 0.5),          # 6: [2, 5] — x == 5 belongs to slab 3, which comes first
                (4.0, 4.0, 1.0)]          # 7: [4, 8] — only (5, 8] is left to it
BORDER_Z_KEEP = 3.0
# an x that belongs to the slab alone (or, slab 2, would if slab 0 did not take it)
BORDER_INTERIOR_X = [0.3, 1.5, 0.6, 5.0, -3.0, -8.0, 3.0, 6.5]


def border_probes():
    """[(x, z, tag)]: for every x limit L the values L-, L, L+ crossed with z = 0 (inside every band) and z = 1.5 (kept
    above every band); for every z limit of every slab L-, L, L+ at an x of that slab's own"""
    from tests.ground_ref import slab_limits
    out = []
    for k, zone in enumerate(BORDER_ZONES):
        x0, x1, zm, zlo = slab_limits(zone)
        for name, lim in (("x0", x0), ("x1", x1)):
            for d in (-1, 0, 1):
                for z in (0.0, 1.5):
                    out.append((step(lim, d), F(z), f"s{k}.{name}{d:+d}"))
        if zm < 0:
            continue
        zlims = [("-zmax", F(-zm)), ("zmax", zm), ("zlo", zlo), ("zkeep", F(BORDER_Z_KEEP))]
        for name, lim in zlims:
            for d in (-1, 0, 1):
                out.append((F(BORDER_INTERIOR_X[k]), step(lim, d), f"s{k}.{name}{d:+d}"))
    return out


def border_frame(crop):
    """Probes on every limit of BORDER_ZONES, in two sensors: identity pose, and the same world points seen through a
    half-turn about z plus the translation (0, 2, 0) (sensor x = -world x exactly). crop: a box whose x faces are slab
    5's lower and slab 7's upper limit, whose lower z face is -zmax of slab 7 and whose upper one is z_keep_max."""
    rng = np.random.default_rng(101)
    probes = border_probes()
    y = (np.arange(len(probes)) % 97) / 32.0 - 1.5                                  # multiples of 1/32: exact under the pose
    pxyz = np.array([(x, yy, z) for (x, z, _), yy in zip(probes, y)], np.float32)
    patches = [ground_patch(rng, 300, 0.12, 0.79), np.stack([rng.uniform(0.85, 1.95, 300), rng.uniform(-2, 2, 300), np.zeros(300)], 1),
               np.stack([np.full(60, 5.0), rng.uniform(-2, 2, 60), 0.02 * rng.standard_normal(60)], 1),
               ground_patch(rng, 200, -3.9, -2.1), ground_patch(rng, 300, -9.9, -6.1), ground_patch(rng, 300, 2.1, 4.9),
               ground_patch(rng, 300, 5.1, 7.9)]
    world = np.concatenate([pxyz] + [p.astype(np.float32) for p in patches])
    world = world[rng.permutation(len(world))]
    inten = np.arange(len(world), dtype=np.float32)
    local2 = np.stack([-world[:, 0], F(2.0) - world[:, 1], world[:, 2]], 1).astype(np.float32)
    sensors = [xyzi_cloud(world, inten), xyzi_cloud(local2, inten + 0.5, q_xyzw=YAW_PI, t_xyz=(0.0, 2.0, 0.0))]
    box = dict(crop_min=(-10.0, -4.0, -1.0), crop_max=(8.0, 6.0, 3.0)) if crop else {}
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **box)
    return GroundFrame("border_crop" if crop else "border_nocrop", sensors, [BORDER_ZONES] * 2, params,
                       dict(GP, z_keep_max=BORDER_Z_KEEP), "closed intervals of kg_classify at exact limits", probes=probes,
                       world=world)


# ---- small_bands_frame ------------------------------------------------------------------------------------------------
SMALL_SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
LARGE_SIZES = (8191, 8192, 8193, 16385)


def _band(rng, n, x_lo, clutter):
    """n band points of a slab [x_lo, x_lo + 1.5] with zmax 0.3: ground + a share of clutter anywhere in the band"""
    p = ground_patch(rng, n, x_lo + 0.05, x_lo + 1.45)
    nc = int(round(n * clutter))
    if nc:
        p[rng.choice(n, nc, replace=False), 2] = rng.uniform(-0.29, 0.29, nc).astype(np.float32)
    return p


def small_bands_frame(large=False, max_iterations=33):
    """16 sensors x 8 slabs (slab k of every sensor: x in [2k, 2k + 1.5], zmax 0.3) with band sizes dealt from
    SMALL_SIZES, so that the sorted band's 1024-point runs hold many slabs, empty ones between them and slabs of
    several sensors; slab (15, 7) is occupied. Clutter shares from 0 to 90 % and a 1.5 cm threshold spread the loops'
    ends over the rounds. large: four sensors, bands of LARGE_SIZES besides small ones (the refit's chunk seams)."""
    rng = np.random.default_rng(202 if large else 201)
    n_sensors = 4 if large else 16
    sensors, zones, sizes = [], [], {}
    deal = list(rng.permutation(np.repeat(SMALL_SIZES, 9)))
    for s in range(n_sensors):
        nz = 8 if s in (0, n_sensors - 1) else int(rng.integers(5, 9))
        zones.append([(2.0 * k, 1.5, 0.3) for k in range(nz)])
        parts = []
        for k in range(nz):
            n = int(deal.pop())
            if large and k == 2 * s % 8:
                n = LARGE_SIZES[s]
            if not large and (s, k) == (15, 7):
                n = 65
            sizes[(s, k)] = n
            parts.append(_band(rng, n, 2.0 * k, rng.choice([0.0, 0.3, 0.6, 0.9])))
            parts.append(np.stack([rng.uniform(2.0 * k, 2.0 * k + 1.5, 3), rng.uniform(-2, 2, 3), rng.uniform(0.5, 2.5, 3)], 1))
        xyz = np.concatenate(parts).astype(np.float32)
        xyz = xyz[rng.permutation(len(xyz))]
        sensors.append(xyzi_cloud(xyz, rng.uniform(0, 255, len(xyz))))
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, crop_min=(-1.0, -5.0, -0.5), crop_max=(20.0, 5.0, 3.0))
    gp = dict(GP, threshold=0.015, max_iterations=max_iterations)
    return GroundFrame(f"{'large' if large else 'small'}_bands_it{max_iterations}", sensors, zones, params, gp,
                       "lead-slab / other-slab counting of kg_score0 and kg_apply, zone keys to 127, chunk seams", sizes=sizes)


# ---- skip_frame -------------------------------------------------------------------------------------------------------
def skip_frame():
    """16 x 8 bands of 40 .. 200 points, 50 to 90 % of them copies of one point off the ground: a sample with two copies
    is skipped, max_iterations 8 leaves 32 hypotheses, and the loop ends after 9 valid ones or when the 32 are used up
    — with a plane or, if all 32 were skipped, without."""
    rng = np.random.default_rng(303)
    sensors, zones = [], []
    for s in range(16):
        zones.append([(2.0 * k, 1.5, 0.3) for k in range(8)])
        parts = []
        for k in range(8):
            n = int(rng.integers(40, 201))
            p = ground_patch(rng, n, 2.0 * k + 0.05, 2.0 * k + 1.45)
            share = rng.choice([0.5, 0.7, 0.8, 0.85, 0.9])
            copies = rng.choice(n, int(n * share), replace=False)
            p[copies] = (F(2.0 * k + 0.7), F(0.3), F(0.2))
            parts.append(p)
        xyz = np.concatenate(parts)
        sensors.append(xyzi_cloud(xyz[rng.permutation(len(xyz))], rng.uniform(0, 255, len(xyz))))
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, crop_min=(-1.0, -5.0, -0.5), crop_max=(20.0, 5.0, 3.0))
    gp = dict(GP, threshold=0.02, max_iterations=8, optimize=False)
    return GroundFrame("skip", sensors, zones, params, gp, "valid and skipped samples alternate; loops end on the spare hypotheses")


# ---- threshold_frame --------------------------------------------------------------------------------------------------
def threshold_frame():
    """Slab 0: a quarter-metre lattice in the plane z = 0 and, over a patch, at z = +-0.25: once three points
    of the middle layer are sampled the plane is (0, 0, +-1, 0) exactly and the outer layers sit at exactly the
    threshold 0.25 — not inliers (strict <). Slab 1: the plane x' + 8 z = 0 (points exactly on it) and copies moved
    0.25 m along its normal (1, 0, 8) / sqrt(65), rounded to fp32: their fp32 distances fall on and one step beside
    the threshold."""
    rng = np.random.default_rng(404)
    # the outer layers only over a small patch in the middle: a tilted plane through one of their points then holds
    # fewer points than the middle layer, so the exact plane wins once it is sampled
    mid = np.array([(i, j, 0) for i in range(4, 37) for j in range(-12, 13)], np.float64)            # x 1 .. 9, y -3 .. 3
    outer = np.array([(i, j, k) for i in range(16, 27) for j in range(-2, 3) for k in (-1, 1)], np.float64)
    flat = np.concatenate([mid, outer]) * 0.25
    mj = np.array([(m, j) for m in range(-14, 15) for j in range(-12, 13)], np.float64)
    on = np.column_stack([25.0 - mj[:, 0] / 8.0, mj[:, 1] * 0.25, mj[:, 0] / 64.0])                  # x' = -8 z
    nrm = np.array([1.0, 0.0, 8.0]) / np.sqrt(65.0)
    patch = on[(np.abs(mj[:, 0]) <= 3) & (np.abs(mj[:, 1]) <= 4)]
    tilted = np.concatenate([on, patch + 0.25 * nrm, patch - 0.25 * nrm])
    xyz = np.concatenate([flat, tilted]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    sensors = [xyzi_cloud(xyz, rng.uniform(0, 255, len(xyz)))]
    zones = [[(0.0, 10.0, 0.5), (20.0, 10.0, 1.0)]]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    gp = dict(GP, threshold=0.25, optimize=False, max_iterations=200)
    return GroundFrame("threshold", sensors, zones, params, gp, "strict |d| < threshold with points at exactly the threshold")


# ---- extreme_frames ---------------------------------------------------------------------------------------------------
FRONT = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]


def front_scene(rng, n, tilt=0.01, ground_sigma=0.03, obj_frac=0.25, obj_z=(0.6, 2.9)):
    """tests/test_ground.py's scene: tilted noisy ground + boxes above it, vehicle frame"""
    ng = int(n * (1 - obj_frac))
    gx, gy = rng.uniform(-15, 60, ng), rng.uniform(-5, 5, ng)
    g = np.stack([gx, gy, -0.05 + tilt * gx + 0.02 * gy + ground_sigma * rng.standard_normal(ng)], 1)
    no = n - ng
    o = np.stack([rng.uniform(-15, 60, no), rng.uniform(-5, 5, no), rng.uniform(*obj_z, no)], 1)
    xyz = np.concatenate([g, o]).astype(np.float32)
    return xyz[rng.permutation(n)]


def no_band_frame():
    """(a) nothing in any band: points above the bands, in a keep-whole slab, in the gaps and outside every slab"""
    rng = np.random.default_rng(501)
    n = 6000
    xyz = np.stack([rng.uniform(-15, 60, n), rng.uniform(-5, 5, n), rng.uniform(0.51, 3.2, n)], 1).astype(np.float32)
    zones = [[(4.0, 15.0, 0.5), (-15.0, 19.0, -1.0), (19.0, 11.0, 0.3)]]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    return GroundFrame("no_band", [xyzi_cloud(xyz, rng.uniform(0, 255, n))], zones, params, dict(GP), "no band point in the frame")


def all_ground_frame():
    """(b) every point on the exact plane z = 0 inside a band: all ground, the no-ground cloud is empty"""
    rng = np.random.default_rng(502)
    ij = np.array([(i, j) for i in range(17, 116) for j in range(-16, 17)], np.float64) * 0.125       # x in (2, 14.5)
    xyz = np.column_stack([ij, np.zeros(len(ij))]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    zones = [[(2.0, 6.0, 0.5), (8.0, 7.0, 0.3)]]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    return GroundFrame("all_ground", [xyzi_cloud(xyz, rng.uniform(0, 255, len(xyz)))], zones, params, dict(GP),
                       "every point is ground: empty no-ground cloud")


def ordinary_frame(seed=503, n=20_000, n_sensors=2):
    rng = np.random.default_rng(seed)
    sensors = [xyzi_cloud(front_scene(rng, n, tilt=0.01 * (s + 1)), rng.uniform(0, 255, n)) for s in range(n_sensors)]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, **ROI)
    return GroundFrame("ordinary", sensors, [FRONT] * n_sensors, params, dict(GP), "a typical frame")


def no_zones_sensor_frame():
    """(c) sensor 0 has n_zones == 0 (all of its points vanish), sensor 1 the usual table"""
    f = ordinary_frame(504)
    return GroundFrame("no_zones_sensor", f.sensors, [[], FRONT], f.params, f.gp, "a sensor with n_zones == 0")


SPECIALS = [np.nan, np.inf, -np.inf, 3.4028235e38, -3.4028235e38, 1e38, 1e-40, -1e-40, 1.4e-45, -0.0]


def special_values_frame(with_vanishing=True):
    """(d) an ordinary frame with special values in x, y, z and intensity, spread through sensor 0. A point with a
    non-finite or huge coordinate vanishes (non-finite, or outside the crop box); denormal and -0.0 coordinates and
    every special intensity belong to ordinary band points and stay. with_vanishing=False: the same frame without the
    points that vanish — planes and clouds must be the same."""
    f = ordinary_frame(505)
    c = f.sensors[0]
    xyz = np.stack([c.data["x"], c.data["y"], c.data["z"]], 1)
    inten = c.data["intensity"].copy()
    rows, vanish = [], []
    for a in range(3):
        for v in SPECIALS:
            p = [8.0 + 0.01 * len(rows), 1.0, 0.05]
            p[a] = v
            rows.append(p)
            vanish.append(not np.isfinite(v) or abs(v) > 1e30)
    rng = np.random.default_rng(506)
    pos = np.sort(rng.choice(len(xyz), len(rows), replace=False))
    xyz = np.insert(xyz, pos, np.array(rows, np.float32), axis=0)
    inten = np.insert(inten, pos, np.float32(7.0))
    gone = np.zeros(len(xyz), bool)
    gone[pos + np.arange(len(pos))] = vanish
    band = np.nonzero((np.abs(xyz[:, 2]) < 0.2) & (xyz[:, 0] > 5) & (xyz[:, 0] < 18) & ~gone)[0][:len(SPECIALS)]
    inten[band] = np.array(SPECIALS, np.float32)                                   # ordinary band points, special intensity
    if not with_vanishing:
        xyz, inten = xyz[~gone], inten[~gone]
    sensors = [xyzi_cloud(xyz, inten)] + f.sensors[1:]
    return GroundFrame("special_values" if with_vanishing else "special_values_removed", sensors, f.zones, f.params, f.gp,
                       "non-finite and huge coordinates, denormals, -0.0 with the stage on", n_vanishing=int(gone.sum()))


def far_frame():
    """(e) the scene of tests/test_ground.py seen by a sensor at (1000, -1000, 0): slab tables and crop box moved there"""
    rng = np.random.default_rng(507)
    n = 30_000
    sensors = [xyzi_cloud(front_scene(rng, n), rng.uniform(0, 255, n), t_xyz=(1000.0, -1000.0, 0.0))]
    zones = [[(x0 + 1000.0, ln, zm) for x0, ln, zm in FRONT]]
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=2, crop_min=(985.0, -1005.0, -0.5), crop_max=(1060.0, -995.0, 3.0))
    return GroundFrame("far", sensors, zones, params, dict(GP), "a scene 1000 m from the origin")


def extreme_frames():
    return [no_band_frame(), all_ground_frame(), no_zones_sensor_frame(), special_values_frame(), far_frame()]


# ---- filter_frame -----------------------------------------------------------------------------------------------------
def filter_frame():
    """Band radius filter, radius 0.25, min 1 neighbour, threshold 0.1 around the ground z ~ 0; the band's non-ground
    points (z >= 0.5) are: a quarter-metre lattice (every neighbour at exactly the radius: d2 == r2, strict <, all
    lonely); the same lattice with a point in the middle of some cells (those cells' corners at 0.2165 m: kept); a pair
    10 cm apart split by the slab border x = 19; and two sensors' single points at the same coordinates."""
    rng = np.random.default_rng(606)
    zones = [[(4.0, 15.0, 1.5), (19.0, 11.0, 2.0)]] * 2
    lattice = np.array([(6.0 + 0.25 * i, 0.25 * j, 0.5 + 0.25 * k) for i in range(6) for j in range(6) for k in range(2)])
    lattice2 = lattice + (4.0, 0.0, 0.0)
    centres = np.array([(10.125 + 0.5 * i, 0.125 + 0.5 * j, 0.625) for i in range(3) for j in range(3)])
    pair = np.array([[18.95, 0.0, 1.0], [19.05, 0.0, 1.0]])
    shared = np.array([[15.0, -3.0, 1.0]])
    parts0 = [ground_patch(rng, 4000, 4.1, 29.9, y=(-4, 4), tilt=0.0), lattice, lattice2, centres, pair, shared]
    parts1 = [ground_patch(rng, 3000, 4.1, 29.9, y=(-4, 4), tilt=0.0), shared, lattice + (0.0, -3.0, 0.0)]
    sensors = []
    for parts in (parts0, parts1):
        xyz = np.concatenate(parts).astype(np.float32)
        sensors.append(xyzi_cloud(xyz[rng.permutation(len(xyz))], rng.uniform(0, 255, len(xyz))))
    params = MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=0, **ROI)
    gp = dict(GP, threshold=0.1, outlier_radius=0.25, outlier_min_neighbors=1)
    return GroundFrame("filter", sensors, zones, params, gp, "band radius filter with pairs at exactly the radius",
                       lattice=lattice.astype(np.float32), lattice2=lattice2.astype(np.float32), centres=centres.astype(np.float32),
                       pair=pair.astype(np.float32), shared=shared.astype(np.float32))


def all_frames():
    return ([border_frame(False), border_frame(True), small_bands_frame(False, 32), small_bands_frame(False, 33),
             small_bands_frame(True, 200), skip_frame(), threshold_frame()] + extreme_frames() + [filter_frame()])
