"""Designed inputs for the edge tests of the ego-motion compensation (tests/test_motion_edges.py): cloud sizes around the
2048 slots of a k_motion workgroup, empty clouds, sensor slots with holes, the time values and stamps at which an integer
or floating-point conversion can go wrong, and twists whose terms vanish, cancel or are fp32 denormals.

Pure numpy: no library and no GPU here. A `Cloud` carries what tests/test_motion.py's `Raw` carries (q, t, time, cloud,
compensated()), packed through tests/layouts.py, so the helpers of tests/test_motion.py take either. What the frames are
designed to hold (which values stay finite, what cancels, what overflows) is asserted on the restatement in the unmarked
tests of tests/test_motion_edges.py before a device byte is looked at."""
import numpy as np

from tests import layouts as wl
from tests import motion_ref as mr

F = np.float32
T_REF = 1_700_000_000_000_000_000
V = (15.0, 0.5, 0.0)
W = (0.01, -0.02, 0.3)
IDENT_Q, IDENT_T = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
IDENT_M = np.eye(3, 4, dtype=F)
INT64_MAX, INT64_MIN = 2 ** 63 - 1, -2 ** 63
WG = 2048                                              # CM_BLOCK * CM_MOTION_ITEMS: the slots of one k_motion workgroup


class Cloud:
    """A raw sensor cloud in layout `kind` (tests/layouts.py) and what the restatement needs to compensate it. tau: float32
    seconds or uint32 nanoseconds, per the layout's time field; None: the sensor has no time field (TIME_NONE). In the two
    xyzi16_t* layouts the time's four bytes are the intensity's: the intensity is then the time's bit pattern."""

    def __init__(self, kind, xyz, tau=None, inten=None, q=IDENT_Q, t=IDENT_T, seed=0):
        lay = wl.layout(kind)
        self.kind, self.q, self.t = kind, q, t
        self.xyz = np.asarray(xyz, F).reshape(-1, 3)
        n = len(self.xyz)
        if tau is None or lay.time is None:
            self.time, self.tau_raw = (0, wl.TIME_NONE), None
        else:
            self.time = lay.time
            self.tau_raw = np.asarray(tau, F if lay.time[1] == wl.TIME_F32_S else np.uint32).reshape(n)
            if lay.time[0] == lay.off[3]:
                inten = self.tau_raw.view(F)
        self.inten = np.zeros(n, F) if inten is None else np.asarray(inten, F).reshape(n)
        self.cloud = wl.repack(self.xyz, self.inten, kind, np.random.default_rng(seed), tau=self.tau_raw, q_xyzw=q, t_xyz=t)
        if lay.off[3] is None:
            self.inten = None

    def compensated(self, m, stamp_ns, t_ref, v, w):
        return mr.compensate(self.xyz, m, mr.time_of(self.tau_raw, self.time[1]), mr.dt0_s(stamp_ns, t_ref), v, w, self.inten)


def matrix_of(q_xyzw, t_xyz):
    """fp64 rotation matrix of a unit quaternion and the translation, rounded to fp32 (the CPU self-checks' transform; the
    GPU tests take the matrix the context holds)."""
    x, y, z, w = (float(a) for a in q_xyzw)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, np.asarray(t_xyz, np.float64).reshape(3, 1)], axis=1).astype(F)


def pose(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q), rng.uniform(-2, 2, 3)


def scene_points(rng, n, half=14.0):
    """70 % of the points on a noisy ground plane, the rest clutter: the extent of synth.ground_scene (the frames of
    tests/test_gpu_parity.py), so that a 1 m grid has voxels of many points and a 1 mm grid overflows."""
    xyz = np.empty((n, 3))
    xyz[:, :2] = rng.uniform(-half, half, (n, 2))
    ng = int(round(0.7 * n))
    xyz[:ng, 2] = rng.normal(-1.5, 0.03, ng)
    xyz[ng:, 2] = rng.uniform(-2.0, 4.0, n - ng)
    return xyz[rng.permutation(n)].astype(F), rng.uniform(0.0, 255.0, n).astype(F)


def times(rng, kind, n, span=0.1):
    """Per-point times over `span` seconds in the layout's type: sorted float32 seconds, or uint32 nanoseconds."""
    time = wl.layout(kind).time
    if time is None:
        return None
    if time[1] == wl.TIME_F32_S:
        return np.sort(rng.uniform(0, span, n)).astype(F)
    return rng.integers(0, int(span * 1e9), n).astype(np.uint32)


def random_cloud(rng, kind, n, span=0.1, identity=False):
    xyz, inten = scene_points(rng, n)
    q, t = (IDENT_Q, IDENT_T) if identity else pose(rng)
    return Cloud(kind, xyz, times(rng, kind, n, span), inten, q, t, seed=int(rng.integers(1 << 30)))


# ---- 1. frame geometry --------------------------------------------------------------------------------------------------
SIZES = [1, 2, 255, 256, 257, WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1, 3 * WG - 1, 3 * WG, 3 * WG + 1]
MIXED_KINDS = ("velo22", "u32ns20", "pcl32_t20")       # f32 at byte 18 (unaligned), u32 at 16 (generic), f32 in PCL32's padding
MIXED_STAMPS = [T_REF - 31_000_000, T_REF + 12_500_000, T_REF - 7_000_001]


def mixed3(n_mid, seed=1, n0=300, n2=4100, span=0.1, zeros=False):
    """Three sensors that differ in layout, time type, stamp and transform; the cloud under test is the middle one.
    zeros: sensor 0 has the identity transform and its first points have zero and minus-zero coordinates."""
    rng = np.random.default_rng(seed)
    clouds = [random_cloud(rng, kind, n, span, identity=zeros and s == 0) for s, (kind, n) in enumerate(zip(MIXED_KINDS, (n0, n_mid, n2)))]
    if zeros:
        c = clouds[0]
        xyz = c.xyz.copy()
        xyz[:6] = [[0.0, 1.5, -2.0], [-0.0, 1.5, -2.0], [3.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-4.0, 0.0, -0.0]]
        clouds[0] = Cloud(c.kind, xyz, c.tau_raw, c.inten, c.q, c.t, seed=seed)
    return clouds, list(MIXED_STAMPS)


FIVE_KINDS = ("velo22", "u32ns20", "pcl32_t20", "livox18_t", "odd17_t")
EMPTY_PATTERNS = [(0, 5, 0, 0, 4097), (2048, 0, 1), (0, 0, 7), (7, 0, 0)]
ALL_EMPTY = (0, 0, 0, 0, 0)


def sized(sizes, seed=2, step_ns=3_000_001):
    """One cloud per size, layouts cycling through FIVE_KINDS, stamps step_ns apart around T_REF."""
    rng = np.random.default_rng(seed)
    clouds = [random_cloud(rng, FIVE_KINDS[s % 5], n) for s, n in enumerate(sizes)]
    return clouds, [T_REF + (s - len(sizes) // 2) * step_ns for s in range(len(sizes))]


HOLE_SLOTS = (1, 4, 9, 15)
HOLE_KINDS = ("velo22", "u32ns20", "pcl32_t28", "odd17_t")
HOLE_SIZES = (700, WG + 1, 300, 1000)
HOLE_FRESH = (4, 15)                                   # the slots that deliver again in the second frame


def hole_stamps(t_ref, used):
    """All 16 entries differ. The used slots lie within tens of milliseconds of t_ref; every other entry is half a second
    and more away, which at 15 m/s would move a point by more than 7 m."""
    st = [t_ref + (1 if s % 2 else -1) * (500_000_000 + 100_000_000 * s) for s in range(16)]
    for s in used:
        st[s] = t_ref - 5_000_000 - 2_700_001 * s
    assert len(set(st)) == 16
    return st


def holes(seed=3):
    """(clouds of the first frame by slot, fresh clouds of the second frame by slot)"""
    rng = np.random.default_rng(seed)
    first = {s: random_cloud(rng, k, n) for s, k, n in zip(HOLE_SLOTS, HOLE_KINDS, HOLE_SIZES)}
    second = {s: random_cloud(rng, first[s].kind, first[s].cloud.n + 77) for s in HOLE_FRESH}
    return first, second


# ---- 2. time values -----------------------------------------------------------------------------------------------------
U32_NS = [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 129, 2 ** 32 - 257, 2 ** 32 - 129,
          2 ** 32 - 128, 2 ** 32 - 1, 10 ** 9, 3 * 10 ** 9]
F32_S = [0.0, -0.0, 0.03, -0.1, 1e-45, -1e-45, 1e-38, 1.1754944e-38, 1e-20, 1e10, 1e19, 1.9e19, 1e20, 3e38, -3e38, np.nan, np.inf, -np.inf]
F32_NON_FINITE = [1.9e19, 1e20, 3e38, -3e38, np.nan, np.inf, -np.inf]     # dt * dt overflows, or the time is not finite
REPEATS = 37                                           # 15 x 37 = 555 and 18 x 37 = 666 points: three items of a thread, every lane


def valued(kind, values, half, seed, q=IDENT_Q, t=IDENT_T):
    """One point per value, the list repeated REPEATS times; points uniform in [-half, half]^3."""
    rng = np.random.default_rng(seed)
    lay = wl.layout(kind)
    tau = np.tile(np.asarray(values, F if lay.time[1] == wl.TIME_F32_S else np.uint32), REPEATS)
    xyz = rng.uniform(-half, half, (len(tau), 3)).astype(F)
    return Cloud(kind, xyz, tau, rng.uniform(0, 255, len(tau)).astype(F), q, t, seed=seed)


def u32_frame():
    """The u32 values at an aligned offset (u32ns20, byte 16) and at an odd one (livox18_t, byte 19); |p| <= 50 (28 sqrt 3)."""
    return [valued("u32ns20", U32_NS, 28.0, 5), valued("livox18_t", U32_NS, 28.0, 6)], [T_REF - 20_000_000, T_REF + 3]


def f32_frame():
    """The f32 values at byte 18 (velo22), in PCL32's padding and at byte 17 (odd17_t), with dt0 = 0, -0.02 s and 1 ns.
    The coordinates stay within 5 m: then h (e + k) of the 1e19 s points stays below FLT_MAX (|e| <= |w|^2 |q| < 0.8,
    |k| components <= 4.5, h = 5e37: below 2.7e38)."""
    clouds = [valued(k, F32_S, 5.0, 7 + s) for s, k in enumerate(("velo22", "pcl32_t20", "odd17_t"))]
    return clouds, [T_REF, T_REF - 20_000_000, T_REF + 1]


CANCEL_STAMP = T_REF - 30_000_000                      # dt0 = -0.03f


def cancel_frame():
    """dt0 = -0.03f and tau = 0.03f for every point: dt = +0, every term vanishes, the output is q."""
    rng = np.random.default_rng(9)
    clouds = []
    for kind, n in (("velo22", 1500), ("pcl32_t20", WG + 1)):
        xyz, inten = scene_points(rng, n)
        clouds.append(Cloud(kind, xyz, np.full(n, F(0.03)), inten, *pose(rng), seed=n))
    return clouds, [CANCEL_STAMP, CANCEL_STAMP]


STAMP_DIFFS = [0, 1, -1, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 53 + 1, -(2 ** 53 + 1), 3_600_000_000_000, -3_600_000_000_000]
STAMP_CROP = ((-100.0,) * 3, (100.0,) * 3)             # drops the clouds that hours and months of motion displace
WRAP_T_REF, WRAP_STAMPS = INT64_MAX, [INT64_MIN + 5, INT64_MAX - 20_000_000]      # the first differs from t_ref by 6 ns modulo 2^64


def stamp_frame():
    clouds, _ = sized([200] * len(STAMP_DIFFS), seed=10)
    return clouds, [T_REF + d for d in STAMP_DIFFS]


def wrap_frame():
    clouds, _ = sized([600, 700], seed=11)
    return clouds, list(WRAP_STAMPS)


# ---- 3. twists ----------------------------------------------------------------------------------------------------------
AXES = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
ZERO3 = (0.0, 0.0, 0.0)
LARGE_TWISTS = [((300.0, -300.0, 300.0), (20.0, -20.0, 20.0)), ((-300.0, 300.0, -300.0), (-20.0, 20.0, -20.0))]
LARGE_SPAN = 0.2
TWISTS = ([("zero", ZERO3, ZERO3, 0.1), ("v_only", V, ZERO3, 0.1), ("w_only", ZERO3, W, 0.1)]
          + [(f"w{'xyz'[i]}_v{'xyz'[j]}", tuple(15.0 * a for a in AXES[j]), tuple(0.3 * a for a in AXES[i]), 0.1)
             for i in range(3) for j in range(3)]
          + [("minus_zero_components", (-0.0, 15.0, -0.0), (-0.0, -0.0, 0.3), 0.1), ("minus_zero_twist", (-0.0,) * 3, (-0.0,) * 3, 0.1)]
          + [(f"large{k}", v, w, LARGE_SPAN) for k, (v, w) in enumerate(LARGE_TWISTS)])

DENORMAL_V, DENORMAL_W, DENORMAL_TAU = (1e-36, 0.0, 0.0), (1e-3, 2e-3, 0.0), 1e-3
FLT_MIN = F(1.17549435e-38)


def denormal_frame():
    """Coordinates of 1e-36 and 3e-37 in every combination and sign, w x q an fp32 denormal; identity transform, dt0 = 0."""
    mags = [F(1e-36), F(3e-37)]
    pts = [(1e-36, 3e-37, 1e-36)] + [(sx * a, sy * b, sz * c) for a in mags for b in mags for c in mags
                                     for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    xyz = np.tile(np.asarray(pts, F), (5, 1))          # 325 points
    n = len(xyz)
    return [Cloud("velo22", xyz, np.full(n, F(DENORMAL_TAU)), np.arange(n, dtype=F), seed=12)], [T_REF]


# ---- 4. fast layouts with a time field ----------------------------------------------------------------------------------
FAST_KINDS = ("pcl32_t20", "pcl32_t28", "xyzi16_tu", "xyzi16_tf")
FAST_SIZES = (2500, WG + 1, 1500, 3000)


def fast_frame(seed=13):
    rng = np.random.default_rng(seed)
    clouds = []
    for kind, n in zip(FAST_KINDS, FAST_SIZES):
        xyz, inten = scene_points(rng, n)
        if kind == "xyzi16_tu":                        # bit patterns of normal floats (0.0005 .. 0.0078): 0.97 s .. 1.01 s as u32 ns
            tau = rng.integers(0x3A000000, 0x3C000000, n).astype(np.uint32)
        else:
            tau = times(rng, kind, n)                  # (xyzi16_tf: small positive intensities, read as seconds)
        clouds.append(Cloud(kind, xyz, tau, inten, *pose(rng), seed=seed + n))
    return clouds, [T_REF - 11_000_000 * (s + 1) - s for s in range(4)]


# ---- 5. sequences -------------------------------------------------------------------------------------------------------
SEQ_KINDS = ("velo22", "u32ns20", "pcl32_t20", "xyzi16")
V2, W2 = (-8.0, 2.0, 0.25), (0.05, 0.02, -0.4)


def seq_frame(sizes, seed):
    rng = np.random.default_rng(seed)
    clouds = [random_cloud(rng, SEQ_KINDS[s % 4], n) for s, n in enumerate(sizes)]
    return clouds, [T_REF - 9_000_000 * (s + 1) - 17 * s for s in range(len(sizes))]


OVERFLOW_LEAF = (0.001,) * 3                           # tests/test_gpu_parity.py test_overflow_guard_returns_merged_input: > 2^31 cells
