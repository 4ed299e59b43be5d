"""Two restatements of the cost layer over the occupancy map (include/cloudmerge.h, cm_map_cost_configure: steps 1-4), both a
function of the map's image (ny x nx int8: -1 / 0 / 100), the map's cell and the four parameters alone.

  cost_brute      for every cell the minimum over the list of obstacle cells, in int64; then the table and step 4.
  cost_separable  column scans (the vertical distance to the nearest obstacle, by a running last-seen row down and up), then
                  for every row the minimum over x' of (x - x')^2 + g(x', y)^2.

The table is step 3 in numpy doubles (sqrt and the product are IEEE-exact, so numpy computes the bits the library's host code
does) with tests/ndt_ref.py's exp_neg for the exponential."""
import math

import numpy as np

from tests import ndt_ref as nr

F32 = np.float32
F64 = np.float64
DIST_NONE = 0xFFFFFFFF
LETHAL, INSCRIBED, NO_INFORMATION = 254, 253, 255
INFLATE_UNKNOWN = 1
MAX_RADIUS_CELLS = 256
MAX_AXIS = 2048


def params(inscribed_radius, inflation_radius, cost_scaling, flags=0):
    return dict(inscribed_radius=inscribed_radius, inflation_radius=inflation_radius, cost_scaling=cost_scaling, flags=flags)


def widened(v):
    """The fp32 value of v as a double."""
    with np.errstate(all="ignore"):
        return F64(F32(v))


def radius_cells(cell, inflation_radius):
    """R of step 3 as a float (it may be beyond every integer type)."""
    with np.errstate(all="ignore"):
        return float(np.ceil(widened(inflation_radius) / widened(cell)))


def refusal(q, cell=0.5, nx=8, ny=8, have_map=True, in_flight=False):
    """Why cm_map_cost_configure refuses q behind a map of nx x ny cells of edge `cell`, or None."""
    if in_flight:
        return "flight"
    if not have_map:
        return "map"
    for key in ("inscribed_radius", "inflation_radius", "cost_scaling"):
        v = widened(q[key])
        if not np.isfinite(v) or v < 0.0:
            return key
    if widened(q["inflation_radius"]) < widened(q["inscribed_radius"]):
        return "order"
    if not radius_cells(cell, q["inflation_radius"]) <= MAX_RADIUS_CELLS:
        return "radius"
    if q["flags"] & ~INFLATE_UNKNOWN:
        return "flags"
    if nx > MAX_AXIS or ny > MAX_AXIS:
        return "axis"
    return None


def table(cell, q, exp_neg=nr.exp_neg):
    """(R * R + 1,) uint8: step 3. exp_neg: the exponential of -x on an array (the project's own; math.exp for comparison)."""
    cell, ri, ro, k = (widened(v) for v in (cell, q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"]))
    R = int(radius_cells(cell, ro))
    d2 = np.arange(R * R + 1, dtype=np.uint32)
    m = np.sqrt(d2.astype(F64)) * cell
    decay = np.floor(252.0 * exp_neg(k * np.maximum(m - ri, 0.0)))
    lut = np.where(m <= ri, 253, np.where(m > ro, 0, decay)).astype(np.uint8)
    lut[0] = LETHAL
    return lut


def cost_of(image, dist2, lut, flags):
    """Step 4."""
    r2 = len(lut) - 1
    infl = np.where(dist2 <= r2, lut[np.minimum(dist2, r2)], 0).astype(np.int64)
    keep = infl > 0 if flags & INFLATE_UNKNOWN else infl >= INSCRIBED
    unknown = np.where(keep, infl, NO_INFORMATION)
    return np.where(image == 100, LETHAL, np.where(image == 0, infl, unknown)).astype(np.uint8)


def dist2_brute(image):
    ny, nx = image.shape
    oy, ox = np.nonzero(image == 100)
    if len(ox) == 0:
        return np.full((ny, nx), DIST_NONE, np.uint32)
    assert nx <= MAX_AXIS and ny <= MAX_AXIS             # (2 * 2047^2 fits the uint32 arithmetic below)
    ys, xs = np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64)
    best = np.full((ny, nx), DIST_NONE, np.uint32)
    tmp = np.empty((ny, nx), np.uint32)
    for x, y in zip(ox.tolist(), oy.tolist()):           # one obstacle at a time over the whole window
        np.add(((ys - y) ** 2).astype(np.uint32)[:, None], ((xs - x) ** 2).astype(np.uint32)[None, :], out=tmp)
        np.minimum(best, tmp, out=best)
    return best


def column_distance(image):
    """(ny, nx) int64: the vertical distance to the nearest obstacle of the column, -1 where the column holds none."""
    ny, nx = image.shape
    far = 1 << 40
    g = np.full((ny, nx), far, np.int64)
    last = np.full(nx, -far, np.int64)
    for y in range(ny):
        last = np.where(image[y] == 100, y, last)
        g[y] = np.minimum(g[y], y - last)
    last = np.full(nx, far, np.int64)
    for y in range(ny - 1, -1, -1):
        last = np.where(image[y] == 100, y, last)
        g[y] = np.minimum(g[y], last - y)
    return np.where(g >= far // 2, -1, g)


def dist2_separable(image):
    ny, nx = image.shape
    g = column_distance(image)
    far = 1 << 50
    g2 = np.where(g < 0, far, g * g)
    xs = np.arange(nx, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2              # (x, x')
    out = np.empty((ny, nx), np.int64)
    for y in range(ny):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    return np.where(out >= far // 2, DIST_NONE, out).astype(np.uint32)


def cost_brute(image, cell, q):
    """(cost uint8, dist2 uint32, table uint8) of the image, by brute force."""
    image = np.asarray(image, np.int8)
    lut = table(cell, q)
    d = dist2_brute(image)
    return cost_of(image, d, lut, q["flags"]), d, lut


def cost_separable(image, cell, q):
    image = np.asarray(image, np.int8)
    lut = table(cell, q)
    d = dist2_separable(image)
    return cost_of(image, d, lut, q["flags"]), d, lut


def libm_exp_neg(x):
    return np.array([math.exp(-float(v)) for v in np.asarray(x, F64).ravel()], F64).reshape(np.shape(x))


def guards(image, cost_plain, cost_unknown, dist2, lut):
    """What a named case must hold before its bytes are compared: all three image values; costs 254, 253, a decayed value,
    0 and 255; an unknown cell whose cost differs between the two flag settings; a dist2 beyond the table; a cell whose
    nearest obstacle lies in another row and another column."""
    assert set(np.unique(image).tolist()) == {-1, 0, 100}, "image values"
    have = set(np.unique(cost_plain).tolist())
    assert {254, 253, 0, 255} <= have and any(0 < v < 253 for v in have), f"costs {sorted(have)}"
    unknown = image == -1
    assert (cost_plain[unknown] != cost_unknown[unknown]).any(), "flag"
    assert ((dist2 != DIST_NONE) & (dist2 > len(lut) - 1)).any(), "beyond the table"
    g = column_distance(image)
    row = column_distance(image.T).T
    diagonal = (dist2 != DIST_NONE) & (dist2 > 0) & ((g < 0) | (dist2 < g * g)) & ((row < 0) | (dist2 < row * row))
    assert diagonal.any(), "diagonal"
