"""numpy restatements of the 2-D grid map (include/cloudmerge.h, cm_result_grid_map), steps 1-5, written twice and
independently of the kernels: grid_vectorised (np.float32 arithmetic, np.minimum.at / np.maximum.at on the integer images) and
grid_loop (one point after the other, Python integers for the images). Both take the clouds A (cm_merged_copy) and G
(cm_ground_copy) as (n, 4) float32 arrays of x, y, z, intensity and return (table, image): GRID_DTYPE of shape (ny, nx) and
int8 of shape (ny, nx)."""
import numpy as np

F32 = np.float32
GRID_DTYPE = np.dtype([("n", "<u4"), ("n_ground", "<u4"), ("z_lo", "<f4"), ("z_hi", "<f4"), ("g_lo", "<f4"), ("g_hi", "<f4"),
                       ("i_max", "<f4"), ("state", "<u4")])
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
MAX_CELLS = 1 << 22
NAN_BITS = 0x7FC00000
IMAGE_OF_STATE = np.array([-1, 0, 100], np.int8)


def a4(cloud):
    """A structured XYZI array (capi.CloudMerger.merged / ground) or anything (n, 4)-shaped as (n, 4) float32."""
    if getattr(cloud, "dtype", None) is not None and cloud.dtype.names:
        return np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]], axis=1).astype(F32).reshape(-1, 4)
    return np.asarray(cloud, F32).reshape(-1, 4)


# ---- vectorised --------------------------------------------------------------------------------------------------------
def ord_image(f):
    b = np.ascontiguousarray(f, F32).view(np.uint32)
    return np.where(b >> 31 != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def ord_back(o):
    o = np.asarray(o, np.uint32)
    return np.where(o >> 31 != 0, o ^ np.uint32(0x80000000), o ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(F32)


def cells_of(pts, origin, cell, nx, ny, z_min, z_max):
    """Index of the cell of every counted point, and which points are counted (steps 1 and 2)."""
    inv = F32(1.0) / F32(cell)
    with np.errstate(all="ignore"):
        cx = np.floor((pts[:, 0] - F32(origin[0])) * inv)
        cy = np.floor((pts[:, 1] - F32(origin[1])) * inv)
        ok = (cx >= F32(0)) & (cx < F32(nx)) & (cy >= F32(0)) & (cy < F32(ny))
        ok &= (F32(z_min) <= pts[:, 2]) & (pts[:, 2] <= F32(z_max))
    ix = np.where(ok, cx, 0).astype(np.int64)
    iy = np.where(ok, cy, 0).astype(np.int64)
    return (ix + iy * nx)[ok], ok


def grid_vectorised(A, G, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1):
    A, G = a4(A), a4(G)
    n_cells = nx * ny
    t = np.zeros(n_cells, GRID_DTYPE)
    lo = {}
    hi = {}
    i_img = np.zeros(n_cells, np.uint32)               # images of non-NaN floats are never 0: 0 is "none"
    for name, pts, cnt in (("z", A, "n"), ("g", G, "n_ground")):
        idx, ok = cells_of(pts, origin, cell, nx, ny, *z_band)
        q = pts[ok]
        t[cnt] = np.bincount(idx, minlength=n_cells).astype(np.uint32)
        lo[name] = np.full(n_cells, 0xFFFFFFFF, np.uint32)
        hi[name] = np.zeros(n_cells, np.uint32)
        np.minimum.at(lo[name], idx, ord_image(q[:, 2]))
        np.maximum.at(hi[name], idx, ord_image(q[:, 2]))
        has_i = ~np.isnan(q[:, 3])
        np.maximum.at(i_img, idx[has_i], ord_image(q[has_i, 3]))
    nan = np.uint32(NAN_BITS).view(F32)
    for name, cnt in (("z", "n"), ("g", "n_ground")):
        t[name + "_lo"] = np.where(t[cnt] > 0, ord_back(lo[name]), nan)
        t[name + "_hi"] = np.where(t[cnt] > 0, ord_back(hi[name]), nan)
    t["i_max"] = np.where(i_img != 0, ord_back(i_img), nan)
    # step 4
    low = ord_back(np.where(t["n_ground"] > 0, np.minimum(lo["z"], lo["g"]), lo["z"]))
    with np.errstate(all="ignore"):
        tall = (t["z_hi"] - low) >= F32(obstacle_height)
    seen = (t["n"].astype(np.uint64) + t["n_ground"]) >= min_points
    t["state"] = np.where(~seen, UNKNOWN, np.where((t["n"] > 0) & tall, OCCUPIED, FREE))
    image = IMAGE_OF_STATE[t["state"]]
    return t.reshape(ny, nx), image.reshape(ny, nx)


# ---- one point after the other --------------------------------------------------------------------------------------------
def _bits(f):
    return int(np.array([f], F32).view(np.uint32)[0])


def _float(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def _image(f):
    b = _bits(f)
    return b ^ 0xFFFFFFFF if b & 0x80000000 else b ^ 0x80000000


def _back(o):
    return _float(o ^ 0x80000000 if o & 0x80000000 else o ^ 0xFFFFFFFF)


def grid_loop(A, G, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3, min_points=1):
    A, G = a4(A), a4(G)
    n_cells = nx * ny
    inv = F32(1.0) / F32(cell)
    ox, oy, z_min, z_max = F32(origin[0]), F32(origin[1]), F32(z_band[0]), F32(z_band[1])
    count = [[0, 0] for _ in range(n_cells)]
    low = [[None, None] for _ in range(n_cells)]
    high = [[None, None] for _ in range(n_cells)]
    imax = [None] * n_cells
    with np.errstate(all="ignore"):
        for which, pts in enumerate((A, G)):
            for x, y, z, inten in pts:
                cx = np.floor(F32(F32(x - ox) * inv))
                cy = np.floor(F32(F32(y - oy) * inv))
                if not (cx >= 0 and cx < F32(nx) and cy >= 0 and cy < F32(ny)):
                    continue
                if not (z_min <= z and z <= z_max):
                    continue
                k = int(cx) + int(cy) * nx
                o = _image(z)
                count[k][which] += 1
                low[k][which] = o if low[k][which] is None else min(low[k][which], o)
                high[k][which] = o if high[k][which] is None else max(high[k][which], o)
                if inten == inten:
                    oi = _image(inten)
                    imax[k] = oi if imax[k] is None else max(imax[k], oi)
    t = np.zeros(n_cells, GRID_DTYPE)
    image = np.zeros(n_cells, np.int8)
    nan = _float(NAN_BITS)
    with np.errstate(all="ignore"):
        for k in range(n_cells):
            n, ng = count[k]
            rec = t[k]
            rec["n"], rec["n_ground"] = n, ng
            rec["z_lo"] = _back(low[k][0]) if n else nan
            rec["z_hi"] = _back(high[k][0]) if n else nan
            rec["g_lo"] = _back(low[k][1]) if ng else nan
            rec["g_hi"] = _back(high[k][1]) if ng else nan
            rec["i_max"] = _back(imax[k]) if imax[k] is not None else nan
            if n + ng < min_points:
                state = UNKNOWN
            elif n == 0:
                state = FREE
            else:
                lo = low[k][0] if ng == 0 else min(low[k][0], low[k][1])
                state = OCCUPIED if F32(_back(high[k][0]) - _back(lo)) >= F32(obstacle_height) else FREE
            rec["state"] = state
            image[k] = (-1, 0, 100)[state]
    return t.reshape(ny, nx), image.reshape(ny, nx)
