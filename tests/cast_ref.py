"""The cast layer restated in numpy from include/cloudmerge.h (steps 1 to 7 of "the cast layer"), by the plain walk: no
skipping, no distance field, Python's integer division. tests/test_map_cast.py compares every byte the library returns with
it. Beside it, for the CPU tests and scripts/map_cast_cost.py only: the skip rule of DESIGN.md §30 as a second walk (with the
cell reads of both counted) and the kernel's quotient without a division (cm_cast_math.hpp) in fp32."""
import numpy as np

F32 = np.float32
MAX_POSES, MAX_BEARINGS, MAX_RANGE_CELLS, MAX_RAYS, PLAIN = 65536, 4096, 1024, 1 << 24, 1
S_MAX, S_HIT, S_OFF_MAP, S_NO_ORIGIN = 0, 1, 2, 3
DIST_NONE = 0xFFFFFFFF
POSE = np.dtype([("x", "<f4"), ("y", "<f4"), ("h", "<u4")])
RAY = np.dtype([("k", "<u2"), ("status", "u1"), ("_pad", "u1"), ("jx", "<i2"), ("jy", "<i2")])
K_TURN = 4294967296.0 / 6.283185307179586


def heading(yaw):
    """The rollout layer's binary angle of a yaw in radians."""
    return int(np.rint(float(yaw) * K_TURN)) & 0xFFFFFFFF


def poses_of(rows):
    """A POSE array from (x, y, h) rows, h a binary angle."""
    out = np.zeros(len(rows), POSE)
    for i, (x, y, h) in enumerate(rows):
        out[i] = (F32(x), F32(y), int(h) & 0xFFFFFFFF)
    return out


def refusal(q):
    if not 1 <= q["max_poses"] <= MAX_POSES:
        return "max_poses"
    if not 1 <= q["n_bearings"] <= MAX_BEARINGS:
        return "n_bearings"
    if not 1 <= q["range_cells"] <= MAX_RANGE_CELLS:
        return "range_cells"
    if q["max_poses"] * q["n_bearings"] > MAX_RAYS:
        return "rays"
    if q["flags"] & ~PLAIN:
        return "flags"
    return None


def directions(range_cells, table):
    """Step 3: (4096, 2) int16 from the (4096, 2) float32 heading table; rint is ties to even."""
    return np.rint(np.asarray(table, np.float32).astype(np.float64) * float(range_cells)).astype(np.int16)


def even_bearings(n):
    return np.array([((a << 32) // n) & 0xFFFFFFFF for a in range(n)], np.uint32)


def entries(h, bearings):
    """Step 2: (n_poses, n_bearings) direction entries."""
    H = (np.asarray(h, np.uint64)[:, None] + np.asarray(bearings, np.uint64)[None, :]) & 0xFFFFFFFF
    return (((H + 0x80000) & 0xFFFFFFFF) >> 20).astype(np.int64) & 4095


def origin_cells(poses, cell, anchor, nx, ny):
    """Step 1: (ox, oy, ok) per pose; ok False where the cell does not exist or lies outside the window."""
    inv = F32(1.0) / F32(cell)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for v, a, n in ((poses["x"], anchor[0], nx), (poses["y"], anchor[1], ny)):
            c = np.floor((v.astype(F32) * inv).astype(F32))
            exists = (c > F32(-1073741824.0)) & (c < F32(1073741824.0))
            g = np.where(exists, c, 0).astype(np.int64) - int(a)
            out.append((g, exists & (g >= 0) & (g < n)))
    return out[0][0], out[1][0], out[0][1] & out[1][1]


def rdiv(a, L):
    """cm_result_grid_rays' step 5: the quotient rounded to nearest, a half away from zero (arrays of int64)."""
    return np.sign(a) * ((2 * np.abs(a) + L) // (2 * L))


def walk_plain(image, ox, oy, dx, dy):
    """Steps 4 and 5 for flat arrays of rays whose origins lie inside the window. Returns (k, status, jx, jy, reads): reads
    counts the image cells looked at."""
    ny, nx = image.shape
    ox, oy, dx, dy = (np.asarray(v, np.int64) for v in (ox, oy, dx, dy))
    L = np.maximum(np.abs(dx), np.abs(dy))
    assert (L >= 1).all()
    n = len(ox)
    k_out, status = L.copy(), np.full(n, S_MAX, np.int64)
    reads = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for k in range(int(L.max()) + 1 if n else 0):
        live &= k <= L
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        cx, cy = ox[idx] + rdiv(k * dx[idx], L[idx]), oy[idx] + rdiv(k * dy[idx], L[idx])
        off = (cx < 0) | (cx >= nx) | (cy < 0) | (cy >= ny)
        assert k >= 1 or not off.any()
        k_out[idx[off]], status[idx[off]] = k - 1, S_OFF_MAP
        ins = idx[~off]
        reads[ins] += 1
        hit = image[cy[~off], cx[~off]] == 100
        k_out[ins[hit]], status[ins[hit]] = k, S_HIT
        live[idx[off]] = False
        live[ins[hit]] = False
    return k_out, status, rdiv(k_out * dx, L), rdiv(k_out * dy, L), reads


def cast(image, cell, anchor, q, bearings, poses, table):
    """Steps 1 to 7: ((n_poses, n_bearings) RAY array, info dict). bearings None: evenly spaced. table: the heading table."""
    ny, nx = image.shape
    b = even_bearings(q["n_bearings"]) if bearings is None else (np.asarray(bearings, np.uint64) & 0xFFFFFFFF).astype(np.uint32)
    assert len(b) == q["n_bearings"] and 1 <= len(poses) <= q["max_poses"] and refusal(q) is None
    E = directions(q["range_cells"], table).astype(np.int64)[entries(poses["h"], b)]          # (n, nb, 2)
    ox, oy, ok = origin_cells(poses, cell, anchor, nx, ny)
    n, nb = len(poses), len(b)
    rays = np.zeros((n, nb), RAY)
    rays["status"][~ok] = S_NO_ORIGIN
    sel = np.flatnonzero(np.repeat(ok, nb))
    if len(sel):
        k, status, jx, jy, _ = walk_plain(image, np.repeat(ox, nb)[sel], np.repeat(oy, nb)[sel], E[..., 0].reshape(-1)[sel], E[..., 1].reshape(-1)[sel])
        flat = rays.reshape(-1)
        flat["k"][sel], flat["status"][sel], flat["jx"][sel], flat["jy"][sel] = k, status, jx, jy
    st = rays["status"]
    info = dict(n_poses=n, n_bearings=nb, n_max=int((st == S_MAX).sum()), n_hit=int((st == S_HIT).sum()), n_off_map=int((st == S_OFF_MAP).sum()),
                n_no_origin=int((st == S_NO_ORIGIN).sum()))
    return rays, info


def ranges(rays, cell):
    return float(F32(cell)) * np.sqrt(rays["jx"].astype(np.float64) ** 2 + rays["jy"].astype(np.float64) ** 2)


# ---- the skip rule, for the CPU tests and the measurement script ---------------------------------------------------
def dist2_of(image):
    """The cost layer's step 2 by brute force (small windows only)."""
    ny, nx = image.shape
    oy, ox = np.nonzero(image == 100)
    out = np.full((ny, nx), DIST_NONE, np.int64)
    if len(ox):
        yy, xx = np.mgrid[0:ny, 0:nx]
        out = ((xx[..., None] - ox) ** 2 + (yy[..., None] - oy) ** 2).min(axis=2)
    return out


def jstar(d2):
    """The smallest j >= 1 with 2 j^2 >= d2, by integers (arrays); d2 >= 1."""
    d2 = np.asarray(d2, np.int64)
    j = np.maximum(np.floor(np.sqrt(d2 / 2.0)).astype(np.int64) - 1, 1)
    for _ in range(3):
        j = np.where(2 * j * j < d2, j + 1, j)
    assert (2 * j * j >= d2).all() and ((j == 1) | (2 * (j - 1) ** 2 < d2)).all()
    return j


def walk_skip(image, dist2, ox, oy, dx, dy, cap=None):
    """The same rays by the skip rule: from an unoccupied cell at step k the ray jumps j* = jstar(dist2(cell)) steps (at most
    cap), and no step beyond the last one inside the window is looked at; that step is found by scanning the line, which is
    monotone per axis. Returns what walk_plain returns; reads counts the dist2 cells looked at."""
    ny, nx = image.shape
    ox, oy, dx, dy = (np.asarray(v, np.int64) for v in (ox, oy, dx, dy))
    L = np.maximum(np.abs(dx), np.abs(dy))
    n = len(ox)
    K = L.copy()                                       # the last step inside
    found = np.zeros(n, bool)
    for k in range(1, int(L.max()) + 1 if n else 0):
        idx = np.flatnonzero(~found & (k <= L))
        if not len(idx):
            break
        cx, cy = ox[idx] + rdiv(k * dx[idx], L[idx]), oy[idx] + rdiv(k * dy[idx], L[idx])
        off = (cx < 0) | (cx >= nx) | (cy < 0) | (cy >= ny)
        K[idx[off]] = k - 1
        found[idx[off]] = True
    k = np.zeros(n, np.int64)
    status = np.full(n, -1, np.int64)
    reads = np.zeros(n, np.int64)
    while True:
        idx = np.flatnonzero((status < 0) & (k <= K))
        if not len(idx):
            break
        cx, cy = ox[idx] + rdiv(k[idx] * dx[idx], L[idx]), oy[idx] + rdiv(k[idx] * dy[idx], L[idx])
        d2 = dist2[cy, cx]
        reads[idx] += 1
        hit = d2 == 0
        status[idx[hit]] = S_HIT
        j = np.where(d2 == DIST_NONE, 1 << 20, jstar(np.where(hit | (d2 == DIST_NONE), 1, d2)))
        if cap is not None:
            j = np.minimum(j, cap)
        k[idx[~hit]] += j[~hit]
    miss = status < 0
    k[miss] = K[miss]
    status[miss] = np.where(K[miss] == L[miss], S_MAX, S_OFF_MAP)
    return k, status, rdiv(k * dx, L), rdiv(k * dy, L), reads


# ---- the kernel's quotient (cm_cast_math.hpp) in fp32 ------------------------------------------------------------------------------
def quot(n, d, rd):
    """floor(n / d) as cm_cast_quot computes it: one fp32 product with rd (about 1 / d), truncation, one correction either way."""
    n, d = np.asarray(n, np.int64), np.asarray(d, np.int64)
    q = (n.astype(F32) * np.asarray(rd, F32)).astype(F32).astype(np.int64)
    r = n - q * d
    return np.where(r < 0, q - 1, np.where(r >= d, q + 1, q))


def minor_cell(k, d, L, ulps=0):
    """rdiv(k * d, L) for d >= 0 as the kernel computes it: quot(2 k d + L, 2 L) with the reciprocal moved by `ulps` units."""
    two_l = (2 * np.asarray(L, np.int64)).astype(F32)
    rd = (F32(1.0) / two_l).astype(F32)
    for _ in range(abs(ulps)):
        rd = np.nextafter(rd, F32(np.inf if ulps > 0 else -np.inf))
    return quot(2 * np.asarray(k, np.int64) * d + L, 2 * np.asarray(L, np.int64), rd)
