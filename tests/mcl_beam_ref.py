"""A restatement of the localisation layer's beam model (include/cloudmerge.h, cm_map_mcl_beam_configure), steps 1-8, written
from the header and independently of the kernel: the two cells in np.float32 by the map's step 1 with
every operation rounded on its own, then integers only: the line by rdiv, the walk cell by cell through the image (the plain
walk), the outcome, the table in double with the spelled-out exponential of tests/ndt_ref.py, the score and the counts as
integer sums. Everything else of an update (beams, weights_of, estimate, resample_parents, Filter) is tests/mcl_ref.py's. A
jump walk over dist2 stands beside the plain one for the CPU equivalence test and the measurement script. No waves, no lanes,
no atomics."""
import numpy as np

from tests import mcl_ref as mr
from tests import ndt_ref as nr

F32 = np.float32
F64 = np.float64
MAX_OVER, MAX_D, PLAIN = 64, 1450, 1
STEP_CAP = 255
COUNTS = ("n_early", "n_at", "n_late", "n_beyond", "n_off", "n_skipped")
EARLY, AT, LATE, BEYOND, OFF, SKIPPED = range(6)


def params(over_cells=8, sigma=0.1, z_hit=0.75, z_short=0.125, z_rand=0.125, flags=0):
    return dict(over_cells=over_cells, sigma=sigma, z_hit=z_hit, z_short=z_short, z_rand=z_rand, flags=flags)


def refusal(b, cell):
    """Why cm_map_mcl_beam_configure refuses b over a map of this cell, or None."""
    if not (np.isfinite(F32(cell)) and F32(cell) > 0):
        return "cell"
    if not 0 <= b["over_cells"] <= MAX_OVER:
        return "over_cells"
    s, zh, zs, zr = (F32(b[k]) for k in ("sigma", "z_hit", "z_short", "z_rand"))
    if not (np.isfinite(s) and s > 0):
        return "sigma"
    if not (np.isfinite(zh) and np.isfinite(zs) and np.isfinite(zr)):
        return "z finite"
    if not zh > 0:
        return "z_hit"
    if not (zs >= 0 and zr >= 0):
        return "z sign"
    if not (float(zh) + float(zs)) + float(zr) <= 1.0:
        return "z sum"
    if b["flags"] & ~PLAIN:
        return "flags"
    return None


def table(b, cell):
    """Step 6: (2E + 3,) uint8. Python floats are doubles; round() of a float is ties to even, as rint."""
    E = b["over_cells"]
    sc = float(F32(b["sigma"])) / float(F32(cell))
    s2 = (2.0 * sc) * sc
    zh, zs, zr = (float(F32(b[k])) for k in ("z_hit", "z_short", "z_rand"))
    out = np.zeros(2 * E + 3, np.uint8)
    for e in range(-E, E + 1):
        v = zh * float(nr.exp_neg(np.array([float(e * e) / s2], F64))[0])
        v = v + (zs if e > 0 else 0.0)
        v = v + zr
        out[e + E] = round(255.0 * min(1.0, v))
    out[2 * E + 1] = round(255.0 * (zs + zr))
    out[2 * E + 2] = round(255.0 * zr)
    return out


# ---- steps 3-5 on Python integers: one ray -----------------------------------------------------------------------------------
def rdiv(a, L):
    """cm_result_grid_rays' step 5: the quotient rounded to nearest, a half away from zero."""
    s = -1 if a < 0 else 1
    return s * ((2 * abs(a) + L) // (2 * L))


def cell_at(k, dx, dy, L):
    return (rdiv(k * dx, L), rdiv(k * dy, L)) if L else (0, 0)


def outcome(hit_k, L, E):
    """Step 5 of a hit at step hit_k: (class, table index)."""
    e = max(hit_k - L, -E)
    return (EARLY if e < 0 else AT if e == 0 else LATE), e + E


def walk_plain(image, ox, oy, dx, dy, E):
    """Steps 3 to 5 of one ray from a cell inside the window: (class, table index, cells read)."""
    ny, nx = image.shape
    L = max(abs(dx), abs(dy))
    reach = L + E if L else 0
    for k in range(reach + 1):
        jx, jy = cell_at(k, dx, dy, L)
        cx, cy = ox + jx, oy + jy
        if not (0 <= cx < nx and 0 <= cy < ny):
            return OFF, 2 * E + 2, k
        if image[cy, cx] == 100:
            return outcome(k, L, E) + (k + 1,)
    return BEYOND, 2 * E + 1, reach + 1


def steps_of(dist2, cap=STEP_CAP):
    """The skip bytes of the cast layer from dist2: 0 on an occupied cell, otherwise the smallest j >= 1 with
    2 j^2 >= dist2, capped."""
    d2 = np.asarray(dist2, np.int64)
    j = np.maximum(np.floor(np.sqrt(np.maximum(d2, 1) / 2.0)).astype(np.int64) - 1, 1)
    for _ in range(3):
        j = np.where(2 * j * j < d2, j + 1, j)
    assert ((2 * j * j >= d2) & ((j == 1) | (2 * (j - 1) ** 2 < d2)))[d2 > 0].all()
    return np.where(d2 == 0, 0, np.minimum(j, cap))


def walk_skip(steps, ox, oy, dx, dy, E):
    """The same ray by the skip bytes: it jumps steps[cell] steps from an unoccupied cell and never looks past the last step
    inside the window, found by scanning the line (membership is monotone in k). Returns what walk_plain returns; the cells
    read are those of steps."""
    ny, nx = steps.shape
    L = max(abs(dx), abs(dy))
    reach = L + E if L else 0
    K = -1
    for k in range(reach + 1):
        jx, jy = cell_at(k, dx, dy, L)
        if not (0 <= ox + jx < nx and 0 <= oy + jy < ny):
            break
        K = k
    k, reads = 0, 0
    while k <= K:
        jx, jy = cell_at(k, dx, dy, L)
        t = int(steps[oy + jy, ox + jx])
        reads += 1
        if t == 0:
            return outcome(k, L, E) + (reads,)
        k += t
    return (BEYOND, 2 * E + 1, reads) if K == reach else (OFF, 2 * E + 2, reads)


# ---- the same walk for many rays at once (int64 arrays; every value stays below 2^32) --------------------------------------------
def walk_plain_many(image, ox, oy, dx, dy, E):
    """walk_plain for flat int64 arrays of rays whose origins lie inside the window: (class, table index, cells read)."""
    ny, nx = image.shape
    ox, oy, dx, dy = (np.asarray(v, np.int64) for v in (ox, oy, dx, dy))
    n = len(ox)
    L = np.maximum(np.abs(dx), np.abs(dy))
    reach = np.where(L > 0, L + E, 0)
    Ls = np.maximum(L, 1)
    cls, idx, reads = np.full(n, BEYOND, np.int64), np.full(n, 2 * E + 1, np.int64), reach + 1
    live = np.arange(n)
    for k in range(int(reach.max()) + 1 if n else 0):
        live = live[k <= reach[live]]
        if not len(live):
            break
        l = Ls[live]
        cx = ox[live] + np.sign(dx[live]) * ((2 * k * np.abs(dx[live]) + l) // (2 * l))
        cy = oy[live] + np.sign(dy[live]) * ((2 * k * np.abs(dy[live]) + l) // (2 * l))
        inside = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        out = live[~inside]
        cls[out], idx[out], reads[out] = OFF, 2 * E + 2, k
        live, cx, cy = live[inside], cx[inside], cy[inside]
        hit = image[cy, cx] == 100
        h = live[hit]
        e = np.maximum(k - L[h], -E)
        cls[h], idx[h], reads[h] = np.where(e < 0, EARLY, np.where(e == 0, AT, LATE)), e + E, k + 1
        live = live[~hit]
    return cls, idx, reads


def walk_skip_many(steps, ox, oy, dx, dy, E):
    """walk_skip for flat int64 arrays of rays whose origins lie inside the window: (class, table index, cells read)."""
    ny, nx = steps.shape
    ox, oy, dx, dy = (np.asarray(v, np.int64) for v in (ox, oy, dx, dy))
    n = len(ox)
    L = np.maximum(np.abs(dx), np.abs(dy))
    reach, Ls = np.where(L > 0, L + E, 0), np.maximum(L, 1)
    cell = lambda k, i: (ox[i] + np.sign(dx[i]) * ((2 * k * np.abs(dx[i]) + Ls[i]) // (2 * Ls[i])),
                         oy[i] + np.sign(dy[i]) * ((2 * k * np.abs(dy[i]) + Ls[i]) // (2 * Ls[i])))
    K = np.zeros(n, np.int64)
    live = np.arange(n)
    for k in range(1, int(reach.max()) + 1 if n else 0):
        live = live[k <= reach[live]]
        cx, cy = cell(k, live)
        live = live[(cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)]
        K[live] = k
    cls = np.where(K == reach, BEYOND, OFF)
    idx = np.where(K == reach, 2 * E + 1, 2 * E + 2)
    k, reads, live = np.zeros(n, np.int64), np.zeros(n, np.int64), np.arange(n)
    while len(live):
        cx, cy = cell(k[live], live)
        t = steps[cy, cx]
        reads[live] += 1
        h = live[t == 0]
        e = np.maximum(k[h] - L[h], -E)
        cls[h], idx[h] = np.where(e < 0, EARLY, np.where(e == 0, AT, LATE)), e + E
        k[live] += t
        live = live[(t > 0) & (k[live] <= K[live])]
    return cls, idx, reads


def rays_of(parts, bm, mq, anchor, tab, shape):
    """Steps 1 to 3 for every (particle, beam): (ox, oy, dx, dy, p) as flat int64 arrays over the rays that are cast, p the
    ray's particle; the pairs left out are the skipped ones."""
    ny, nx = shape
    c, s = mr.directions(parts["h"], tab)
    c, s, x, y = c[:, None], s[:, None], parts["x"][:, None], parts["y"][:, None]
    fx, fy = bm["fx"][None, :], bm["fy"][None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        wx = (x + c * fx) - s * fy
        wy = (y + s * fx) + c * fy
        assert wx.dtype == F32 and wy.dtype == F32
        inv = F32(1.0) / F32(mq["cell"])
        lim = F32(1073741824.0)
        cells = []
        for v in (parts["x"], parts["y"], wx, wy):
            cv = np.floor(v * inv)
            ok = (cv > -lim) & (cv < lim)
            cells.append((np.where(ok, cv, 0).astype(np.int64), ok))
    (px, pxok), (py, pyok), (gx, gxok), (gy, gyok) = cells
    ox, oy = px - anchor[0], py - anchor[1]
    origin = pxok & pyok & (ox >= 0) & (ox < nx) & (oy >= 0) & (oy < ny)
    dx, dy = gx - px[:, None], gy - py[:, None]
    cast = origin[:, None] & gxok & gyok & (np.maximum(np.abs(dx), np.abs(dy)) <= MAX_D)
    pi, bi = np.nonzero(cast)
    return ox[pi], oy[pi], dx[pi, bi], dy[pi, bi], pi


def scores(parts, bm, image, mq, anchor, tab, b):
    """Steps 1 to 8: (S_p as (n,) uint32, the six counts, the image cells read)."""
    image = np.asarray(image, np.int8)
    E, T = b["over_cells"], table(b, mq["cell"]).astype(np.int64)
    n, nb = len(parts), bm["n_beams"]
    counts = [0] * 6
    S = np.zeros(n, np.int64)
    if nb == 0:
        return S.astype(np.uint32), counts, 0
    ox, oy, dx, dy, pi = rays_of(parts, bm, mq, anchor, tab, image.shape)
    counts[SKIPPED] = n * nb - len(pi)
    cls, idx, reads = walk_plain_many(image, ox, oy, dx, dy, E)
    for k in range(5):
        counts[k] = int((cls == k).sum())
    np.add.at(S, pi, T[idx])
    assert sum(counts) == n * nb and S.max(initial=0) <= 8192 * 255
    return S.astype(np.uint32), counts, int(reads.sum())


def update(parts, A, dist2, image, mq, anchor, q, b, gen, tab):
    """An update with the beam model on: (the particles afterwards, the weight table, the info dictionary, the beam info
    dictionary). Steps 6 and 8 to 11 are tests/mcl_ref.py's."""
    bm = mr.beams(A, mq, q)
    S, counts, reads = scores(parts, bm, image, mq, anchor, tab, b)
    found = parts.copy()
    found["acc"] = parts["acc"] + S.astype(np.uint64)
    W = mr.weights_of(found["acc"], q["tau"])
    wt = np.zeros(len(parts), mr.WEIGHT)
    wt["score"], wt["weight"] = S, W
    info = mr.estimate(found, W, tab)
    best = found[info["best"]]
    info.update(n_particles=len(parts), n_cells=bm["n_cells"], stride=bm["stride"], n_beams=bm["n_beams"], gen=gen, best_x=best["x"], best_y=best["y"],
                best_h=int(best["h"]))
    do = bool(q["flags"] & mr.RESAMPLE_ALWAYS) or info["n_eff"] < float(F32(q["resample_frac"])) * float(q["n_particles"])
    info["resampled"] = int(do)
    out = found.copy()
    if do:
        par = mr.resample_parents(W, mr.splitmix64(mr.base_of(q["seed"], gen) ^ (1 << 63)))
        out["x"], out["y"], out["h"] = found["x"][par], found["y"][par], found["h"][par]
        out["parent"] = par
        out["acc"] = 0
    else:
        out["parent"] = np.arange(len(parts))
    binfo = dict(zip(COUNTS, counts), n_rays=len(parts) * bm["n_beams"], reads=reads)
    return out, wt, info, binfo


class Filter(mr.Filter):
    """tests/mcl_ref.py's Filter with the mode: beam None scores by the field, a params() dictionary by the beam model. The
    configure call takes no gen."""

    def __init__(self, q, mq, tab, beam=None):
        super().__init__(q, mq, tab)
        self.beam_configure(beam)

    def beam_configure(self, beam):
        assert beam is None or refusal(beam, self.mq["cell"]) is None
        self.beam, self.binfo = beam, None

    def update(self, A, dist2, anchor, image=None):
        if self.beam is None:
            self.binfo = None
            return super().update(A, dist2, anchor)
        assert self.parts is not None and image is not None
        self.parts, wt, info, self.binfo = update(self.parts, A, dist2, image, self.mq, anchor, self.q, self.beam, self.gen, self.tab)
        self.gen += 1
        return wt, info
