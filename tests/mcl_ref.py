"""A numpy restatement of the localisation layer (include/cloudmerge.h, cm_map_mcl_*), steps 1-11, written from the header and
independently of the kernels: the draws as Python and uint64 integer arithmetic, the noise integer, positions in np.float32 with
every operation rounded on its own, headings as integers mod 2^32, the beams as a sorted set of body cells, the score by the
field of tests/match_ref.py and the cell computation of tests/traj_ref.py, the weights with the spelled-out exponential of
tests/ndt_ref.py, every sum of the estimate as a Python integer, the resampling by a search in the prefix sums. No waves, no
lanes, no atomics. It takes the cloud A (cm_merged_copy) as an (n, 4) float32 array, dist2 as the cost layer holds it, the map's
parameters, anchor and image and the heading table (cm_traj_directions)."""
import math

import numpy as np

from tests import match_ref as mf
from tests import ndt_ref as nr
from tests import traj_ref as tj

F32 = np.float32
F64 = np.float64
U64 = np.uint64
M64 = (1 << 64) - 1
MAX_PARTICLES, MAX_BEAMS, MAX_RANGE_CELLS = 65536, 8192, 1024
W1 = 65536
RESAMPLE_ALWAYS = 1
K = tj.K
K1 = math.sqrt(3.0 / 4294967295.0)
LIMIT = F32(1073741824.0)
PARTICLE = np.dtype([("x", "<f4"), ("y", "<f4"), ("h", "<u4"), ("parent", "<u4"), ("acc", "<u8")])
WEIGHT = np.dtype([("score", "<u4"), ("weight", "<u4")])
SUMS = ("sum_w", "sum_w2", "sum_wqx", "sum_wqy", "sum_wc", "sum_ws", "sum_wdxx", "sum_wdyy", "sum_wdxy")


def params(n_particles=64, max_beams=64, range_cells=64, sigma=0.1, max_dist=0.5, tau=8.0, resample_frac=0.5, flags=0, seed=1):
    return dict(n_particles=n_particles, max_beams=max_beams, range_cells=range_cells, sigma=sigma, max_dist=max_dist, tau=tau,
                resample_frac=resample_frac, flags=flags, seed=seed)


def refusal(q, cell):
    """Why cm_map_mcl_configure refuses q over a map of this cell, or None."""
    if not 1 <= q["n_particles"] <= MAX_PARTICLES:
        return "n_particles"
    if not 1 <= q["max_beams"] <= MAX_BEAMS:
        return "max_beams"
    if not 1 <= q["range_cells"] <= MAX_RANGE_CELLS:
        return "range_cells"
    why = mf.refusal(dict(mf.params(), sigma=q["sigma"], max_dist=q["max_dist"]), cell)
    if why:
        return why
    tau, frac = F32(q["tau"]), F32(q["resample_frac"])
    if not (np.isfinite(tau) and tau > 0):
        return "tau"
    if not (np.isfinite(frac) and 0 <= frac <= 1):
        return "resample_frac"
    if q["flags"] & ~RESAMPLE_ALWAYS:
        return "flags"
    return None


def values_refusal(v):
    """Why init_pose or predict refuses (x, y, yaw, sd_x, sd_y, sd_yaw), or None."""
    v = [F32(t) for t in v]
    if not all(np.isfinite(t) for t in v):
        return "finite"
    if abs(v[2]) > 1024:
        return "yaw"
    if any(t < 0 or t > 1024 for t in v[3:]):
        return "sd"
    return None


# ---- step 2: the draws ------------------------------------------------------------------------------------------------------
def splitmix64(x):
    """The ground stage's function on a Python integer."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def splitmix64_array(x):
    """The same on a uint64 array (numpy's uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def base_of(seed, gen):
    return splitmix64((seed + gen) & M64)


def draws(seed, gen, first_p, n_p, i):
    """draw(p, i) for p = first_p .. first_p + n_p - 1: (n_p,) uint64."""
    assert 0 <= i < 256
    p = np.arange(first_p, first_p + n_p, dtype=U64)
    return splitmix64_array(U64(base_of(seed, gen)) ^ (p << U64(8)) ^ U64(i))


def noise(u):
    """n(u): int64 in [-131070, 131070]."""
    u = np.asarray(u, U64)
    m = U64(0xFFFF)
    return ((u & m) + ((u >> U64(16)) & m) + ((u >> U64(32)) & m) + (u >> U64(48))).astype(np.int64) - 131070


def scale(sd):
    return F32(F64(F32(sd)) * F64(K1))


def noise_values(seed, gen, n, i, sd):
    """(float)n(draw(p, i)) * sc for p < n: fp32."""
    return noise(draws(seed, gen, 0, n, i)).astype(F32) * scale(sd)


def turns(yaw, nz):
    """The low 32 bits of (int64)rint(((double)yaw + (double)nz) * K): uint32."""
    v = np.rint((F64(F32(yaw)) + nz.astype(F64)) * K).astype(np.int64)
    return (v & 0xFFFFFFFF).astype(np.uint32)


# ---- steps 3-5 ---------------------------------------------------------------------------------------------------------------
def init_pose(q, gen, x0, y0, yaw0, sd_x, sd_y, sd_yaw):
    n, seed = q["n_particles"], q["seed"]
    out = np.zeros(n, PARTICLE)
    out["x"] = F32(x0) + noise_values(seed, gen, n, 0, sd_x)
    out["y"] = F32(y0) + noise_values(seed, gen, n, 1, sd_y)
    out["h"] = turns(yaw0, noise_values(seed, gen, n, 2, sd_yaw))
    out["parent"] = np.arange(n)
    return out


def free_cells(image):
    return np.flatnonzero(np.asarray(image, np.int8).reshape(-1) == 0)


def init_uniform(q, gen, image, anchor, cell):
    """None where the image holds no free cell (CM_BAD_ARG)."""
    n, seed = q["n_particles"], q["seed"]
    ny, nx = image.shape
    free = free_cells(image)
    if len(free) == 0:
        return None
    rank = np.array([(int(d) * len(free)) >> 64 for d in draws(seed, gen, 0, n, 0)], np.int64)
    c = free[rank]
    ix, iy = c % nx, c // nx
    ux = (draws(seed, gen, 0, n, 1) >> U64(40)).astype(F32) * F32(2.0 ** -24)
    uy = (draws(seed, gen, 0, n, 2) >> U64(40)).astype(F32) * F32(2.0 ** -24)
    out = np.zeros(n, PARTICLE)
    out["x"] = ((anchor[0] + ix).astype(F32) + ux) * F32(cell)
    out["y"] = ((anchor[1] + iy).astype(F32) + uy) * F32(cell)
    out["h"] = (draws(seed, gen, 0, n, 3) >> U64(32)).astype(np.uint32)
    out["parent"] = np.arange(n)
    return out


def directions(h, tab):
    e = ((h.astype(np.uint64) + np.uint64(0x80000)) >> np.uint64(20)).astype(np.int64) & 4095
    return tab[e, 0].astype(F32), tab[e, 1].astype(F32)


def predict(parts, q, gen, d_fwd, d_left, d_yaw, sd_fwd, sd_left, sd_yaw, tab):
    n, seed = q["n_particles"], q["seed"]
    out = parts.copy()
    c, s = directions(parts["h"], tab)
    a = F32(d_fwd) + noise_values(seed, gen, n, 0, sd_fwd)
    b = F32(d_left) + noise_values(seed, gen, n, 1, sd_left)
    with np.errstate(over="ignore", invalid="ignore"):
        out["x"] = (parts["x"] + c * a) - s * b
        out["y"] = (parts["y"] + s * a) + c * b
    out["h"] = ((parts["h"].astype(np.int64) + turns(d_yaw, noise_values(seed, gen, n, 2, sd_yaw)).astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
    return out


# ---- steps 6-11 --------------------------------------------------------------------------------------------------------------
def beams(A, mq, q):
    """Step 6: dict(n_cells, stride, n_beams, bx, by, fx, fy)."""
    A = np.asarray(A, F32).reshape(-1, 4)
    R = q["range_cells"]
    inv = F32(1.0) / F32(mq["cell"])
    x, y, z = A[:, 0], A[:, 1], A[:, 2]
    with np.errstate(all="ignore"):
        cx, cy = np.floor(x * inv), np.floor(y * inv)
        ok = (cx > -LIMIT) & (cx < LIMIT) & (cy > -LIMIT) & (cy < LIMIT)
        ok &= (F32(mq["z_band"][0]) <= z) & (z <= F32(mq["z_band"][1]))
    bx, by = np.where(ok, cx, 0).astype(np.int64), np.where(ok, cy, 0).astype(np.int64)
    ok &= (np.abs(bx) <= R) & (np.abs(by) <= R)
    side = 2 * R + 1
    cells = np.unique(((by + R) * side + (bx + R))[ok])                # ascending (b_y, b_x)
    n_cells = len(cells)
    stride = max(1, -(-n_cells // q["max_beams"]))
    pick = cells[::stride]
    bx, by = pick % side - R, pick // side - R
    fx = (bx.astype(F32) + F32(0.5)) * F32(mq["cell"])
    fy = (by.astype(F32) + F32(0.5)) * F32(mq["cell"])
    return dict(n_cells=n_cells, stride=stride, n_beams=len(pick), bx=bx, by=by, fx=fx, fy=fy)


def scores(parts, bm, L, mq, anchor, tab, chunk=2048):
    """Step 7: S_p as (n,) uint32."""
    ny, nx = L.shape
    S = np.zeros(len(parts), np.int64)
    fx, fy = bm["fx"][None, :], bm["fy"][None, :]
    for lo in range(0, len(parts), chunk):
        p = parts[lo:lo + chunk]
        c, s = directions(p["h"], tab)
        c, s, x, y = c[:, None], s[:, None], p["x"][:, None], p["y"][:, None]
        with np.errstate(over="ignore", invalid="ignore"):
            wx = (x + c * fx) - s * fy
            wy = (y + s * fx) + c * fy
        assert wx.dtype == F32 and wy.dtype == F32
        on, ix, iy = tj.cells_of(wx, wy, mq["cell"], anchor, nx, ny)
        S[lo:lo + chunk] = np.where(on, L[iy, ix], 0).astype(np.int64).sum(axis=1)
    assert S.max(initial=0) < 1 << 32
    return S.astype(np.uint32)


def weights_of(acc, tau):
    """Step 8: W_p as (n,) int64."""
    beta = 1.0 / (255.0 * float(F32(tau)))
    d = (acc.max() - acc).astype(U64)
    return np.floor(65536.0 * nr.exp_neg(d.astype(F64) * beta)).astype(np.int64)


def quant(v):
    """Step 9's q(v): int64."""
    v = np.asarray(v, F32)
    fin = np.isfinite(v)
    x = np.where(fin, v, 0).astype(F64) * 1024.0
    return np.where(fin, np.rint(np.clip(x, -float(1 << 30), float(1 << 30))), 0).astype(np.int64)


def estimate(parts, W, tab):
    """Step 9: the nine integer sums and best, then the host's doubles."""
    c, s = directions(parts["h"], tab)
    ci, si = np.rint(c * F32(32768.0)).astype(np.int64), np.rint(s * F32(32768.0)).astype(np.int64)
    qx, qy = quant(parts["x"]), quant(parts["y"])
    isum = lambda a: sum(int(v) for v in a.tolist())
    r = dict(sum_w=isum(W), sum_w2=isum(W * W), sum_wqx=isum(W * qx), sum_wqy=isum(W * qy), sum_wc=isum(W * ci), sum_ws=isum(W * si))
    mqx, mqy = r["sum_wqx"] // r["sum_w"], r["sum_wqy"] // r["sum_w"]
    dx, dy = np.clip(qx - mqx, -32768, 32767), np.clip(qy - mqy, -32768, 32767)
    r.update(sum_wdxx=isum(W * dx * dx), sum_wdyy=isum(W * dy * dy), sum_wdxy=isum(W * dx * dy))
    assert all(abs(r[k]) < 1 << 63 for k in SUMS)
    r["best"] = int(np.argmax(parts["acc"]))           # (the first of the largest)
    sw = float(r["sum_w"])
    r["mean_x"] = (float(r["sum_wqx"]) / sw) / 1024.0
    r["mean_y"] = (float(r["sum_wqy"]) / sw) / 1024.0
    r["mean_yaw"] = math.atan2(float(r["sum_ws"]), float(r["sum_wc"]))
    den = sw * 1048576.0
    r["var_xx"], r["var_yy"], r["var_xy"] = float(r["sum_wdxx"]) / den, float(r["sum_wdyy"]) / den, float(r["sum_wdxy"]) / den
    r["n_eff"] = (sw * sw) / float(r["sum_w2"])
    return r


def resample_parents(W, r_draw):
    """Step 10: the parent of every new particle, from the weights and splitmix64(base ^ 1 << 63)."""
    W = [int(w) for w in np.asarray(W).tolist()]
    N, T = len(W), sum(W)
    r = (r_draw * T) >> 64
    C = np.cumsum(np.array(W, np.int64))
    t = np.array([(j * T + r) // N for j in range(N)], np.int64)
    return np.searchsorted(C, t, side="right")         # the smallest p with C_p > t


def update(parts, A, dist2, mq, anchor, q, gen, tab):
    """Steps 6-11: (the particles afterwards, the weight table, the info dictionary)."""
    L = mf.field(dist2, mf.table(mq["cell"], q["sigma"], q["max_dist"]))
    bm = beams(A, mq, q)
    S = scores(parts, bm, L, mq, anchor, tab)
    found = parts.copy()
    found["acc"] = parts["acc"] + S.astype(U64)
    W = weights_of(found["acc"], q["tau"])
    table = np.zeros(len(parts), WEIGHT)
    table["score"], table["weight"] = S, W
    info = estimate(found, W, tab)
    b = found[info["best"]]
    info.update(n_particles=len(parts), n_cells=bm["n_cells"], stride=bm["stride"], n_beams=bm["n_beams"], gen=gen, best_x=b["x"], best_y=b["y"],
                best_h=int(b["h"]))
    do = bool(q["flags"] & RESAMPLE_ALWAYS) or info["n_eff"] < float(F32(q["resample_frac"])) * float(q["n_particles"])
    info["resampled"] = int(do)
    out = found.copy()
    if do:
        par = resample_parents(W, splitmix64(base_of(q["seed"], gen) ^ (1 << 63)))
        out["x"], out["y"], out["h"] = found["x"][par], found["y"][par], found["h"][par]
        out["parent"] = par
        out["acc"] = 0
    else:
        out["parent"] = np.arange(len(parts))
    return out, table, info


class Filter:
    """The layer's calls in order: it counts gen as the library does (a refused call does not count)."""

    def __init__(self, q, mq, tab):
        assert refusal(q, mq["cell"]) is None
        self.q, self.mq, self.tab, self.gen, self.parts = q, mq, tab, 0, None

    def init_pose(self, x0, y0, yaw0, sd_x=0.0, sd_y=0.0, sd_yaw=0.0):
        assert values_refusal((x0, y0, yaw0, sd_x, sd_y, sd_yaw)) is None
        self.parts = init_pose(self.q, self.gen, x0, y0, yaw0, sd_x, sd_y, sd_yaw)
        self.gen += 1

    def init_uniform(self, image, anchor):
        parts = init_uniform(self.q, self.gen, image, anchor, self.mq["cell"])
        if parts is None:
            return False
        self.parts = parts
        self.gen += 1
        return True

    def predict(self, d_fwd, d_left, d_yaw, sd_fwd=0.0, sd_left=0.0, sd_yaw=0.0):
        assert self.parts is not None and values_refusal((d_fwd, d_left, d_yaw, sd_fwd, sd_left, sd_yaw)) is None
        self.parts = predict(self.parts, self.q, self.gen, d_fwd, d_left, d_yaw, sd_fwd, sd_left, sd_yaw, self.tab)
        self.gen += 1

    def update(self, A, dist2, anchor):
        assert self.parts is not None
        self.parts, table, info = update(self.parts, A, dist2, self.mq, anchor, self.q, self.gen, self.tab)
        self.gen += 1
        return table, info
