"""The frontier layer behind the plan layer (cm_map_frontier_configure, cm_map_frontier_update; the numbered semantics in
include/cloudmerge.h) restated twice with numpy and the standard library only: a flood fill per component with
everything else in plain loops (frontiers_flood), and a minimum propagation over the whole image at once, run to its fixed
point, with vectorised reductions behind it (frontiers_propagate). Both are written from the header's steps, not from the
kernels: no tiles, no unions, no scan. Every quantity is an integer, so the two and the device agree in every byte or one of
them is wrong. With them: the refusals of cm_map_frontier_configure (refusal) and the named guards that say what a designed
case holds (guards), evaluated on a restatement's output alone."""
import numpy as np

NONE = 0xFFFFFFFF
UNREACHABLE = 0xFFFFFFFF
MAX_TABLE = 1 << 16
INT64_MAX = (1 << 63) - 1
FRONTIER_DTYPE = np.dtype([("first_cell", "<u4"), ("n_cells", "<u4"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("min_pot", "<u4"),
                           ("min_pot_cell", "<u4"), ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")])
EIGHT = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
FOUR = ((1, 0), (0, 1), (-1, 0), (0, -1))


def params(min_cells=1, max_frontiers=MAX_TABLE, max_cost=252, pot_scale=1, gain_scale=0):
    return dict(min_cells=min_cells, max_frontiers=max_frontiers, max_cost=max_cost, pot_scale=pot_scale, gain_scale=gain_scale)


def refusal(q, have_plan=True, in_flight=False):
    """Why cm_map_frontier_configure refuses, or None."""
    if in_flight:
        return "flight"
    if not have_plan:
        return "plan"
    if q["min_cells"] < 1:
        return "min_cells"
    if not 1 <= q["max_frontiers"] <= MAX_TABLE:
        return "max_frontiers"
    if not 0 <= q["max_cost"] <= 252:
        return "max_cost"
    return None


def score(q, min_pot, n_cells):
    """Step 6 in Python's integers: exact, and INT64_MAX where it is above that."""
    s = q["pot_scale"] * int(min_pot) - q["gain_scale"] * int(n_cells)
    return min(s, INT64_MAX) if s >= -INT64_MAX else -INT64_MAX - 1          # (below: unreachable with a window's 2^22 cells)


def info_tuple(n_frontier_cells, n_components, n_frontiers, n_written, best, best_score):
    return (int(n_frontier_cells), int(n_components), int(n_frontiers), int(n_written), int(best), 0, int(best_score))


# ---- one thing after the other --------------------------------------------------------------------------------------------
def frontiers_flood(image, cost, pot, q):
    """(labels (ny, nx) uint32, table FRONTIER_DTYPE, info tuple) by steps 1 to 7 in loops: a flood fill per component."""
    ny, nx = image.shape
    I, cst, p = image.tolist(), cost.tolist(), pot.tolist()
    front = [[False] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            if I[y][x] != 0 or cst[y][x] > q["max_cost"]:
                continue
            for dx, dy in FOUR:
                if 0 <= x + dx < nx and 0 <= y + dy < ny and I[y + dy][x + dx] == -1:
                    front[y][x] = True
    seen = [[False] * nx for _ in range(ny)]
    comps = []
    for y in range(ny):                                # ascending cell index: every component is met at its first_cell
        for x in range(nx):
            if not front[y][x] or seen[y][x]:
                continue
            seen[y][x] = True
            cells, stack = [], [(x, y)]
            while stack:
                cx, cy = stack.pop()
                cells.append((cx, cy))
                for dx, dy in EIGHT:
                    ax, ay = cx + dx, cy + dy
                    if 0 <= ax < nx and 0 <= ay < ny and front[ay][ax] and not seen[ay][ax]:
                        seen[ay][ax] = True
                        stack.append((ax, ay))
            assert min(cx + cy * nx for cx, cy in cells) == x + y * nx
            comps.append(cells)
    labels = np.full((ny, nx), NONE, np.uint32)
    rows = []
    k = 0
    for cells in comps:
        if len(cells) < q["min_cells"]:
            continue
        for cx, cy in cells:
            labels[cy, cx] = k
        if k < q["max_frontiers"]:
            reach = [(p[cy][cx], cx + cy * nx) for cx, cy in cells if p[cy][cx] != UNREACHABLE]
            mp, mc = min(reach) if reach else (UNREACHABLE, NONE)
            xs, ys = [c[0] for c in cells], [c[1] for c in cells]
            rows.append((min(cx + cy * nx for cx, cy in cells), len(cells), sum(xs), sum(ys), mp, mc, min(xs), min(ys), max(xs), max(ys)))
        k += 1
    table = np.array(rows, FRONTIER_DTYPE) if rows else np.zeros(0, FRONTIER_DTYPE)
    best, best_score = NONE, 0
    for j, r in enumerate(rows):
        if r[4] == UNREACHABLE:
            continue
        s = score(q, r[4], r[1])
        if best == NONE or s < best_score:
            best, best_score = j, s
    n_cells = sum(len(c) for c in comps)
    return labels, table, info_tuple(n_cells, len(comps), k, len(rows), best, best_score)


# ---- the whole image at once ----------------------------------------------------------------------------------------------
def frontier_mask(image, cost, q):
    """Step 1: (ny, nx) bool."""
    unknown = np.pad(image == -1, 1, constant_values=False)        # (outside the window: not unknown)
    beside = unknown[1:-1, 2:] | unknown[1:-1, :-2] | unknown[2:, 1:-1] | unknown[:-2, 1:-1]
    return (image == 0) & (cost.astype(np.int64) <= q["max_cost"]) & beside


def roots_of(mask, dirs=EIGHT):
    """Step 2: per frontier cell the smallest cell index of its component (int64, -1 elsewhere): every cell takes the minimum
    over itself and its neighbours among the frontier cells until nothing changes."""
    ny, nx = mask.shape
    big = np.int64(1) << 40
    lab = np.where(mask, np.arange(nx * ny, dtype=np.int64).reshape(ny, nx), big)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        m = lab
        for dx, dy in dirs:
            m = np.minimum(m, p[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
        m = np.where(mask, m, big)
        if (m == lab).all():
            break
        lab = m
    return np.where(mask, lab, -1)


def frontiers_propagate(image, cost, pot, q):
    """The same three results with numpy's reductions over the roots of a whole-image minimum propagation."""
    ny, nx = image.shape
    mask = frontier_mask(image, cost, q)
    root = roots_of(mask)
    cell = np.arange(nx * ny, dtype=np.int64)
    r = root.ravel()
    on = r >= 0
    firsts, inverse, counts = np.unique(r[on], return_inverse=True, return_counts=True)       # (ascending first_cell)
    is_front = counts >= q["min_cells"]
    number = np.where(is_front, np.cumsum(is_front) - 1, -1)
    labels = np.full(nx * ny, NONE, np.uint32)
    num_of_cell = number[inverse]
    labels[cell[on][num_of_cell >= 0]] = num_of_cell[num_of_cell >= 0]
    n_frontiers = int(is_front.sum())
    n_written = min(n_frontiers, q["max_frontiers"])
    table = np.zeros(n_written, FRONTIER_DTYPE)
    keep = (num_of_cell >= 0) & (num_of_cell < n_written)
    k, c = num_of_cell[keep], cell[on][keep]
    x, y, p = c % nx, c // nx, pot.ravel().astype(np.int64)[c]
    table["first_cell"] = firsts[is_front][:n_written]
    table["n_cells"] = counts[is_front][:n_written]
    table["sum_x"] = np.bincount(k, x, n_written).astype(np.uint64)
    table["sum_y"] = np.bincount(k, y, n_written).astype(np.uint64)
    key = np.full(n_written, (UNREACHABLE << 32) | NONE, np.uint64)
    np.minimum.at(key, k[p != UNREACHABLE], ((p.astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64))[p != UNREACHABLE])
    table["min_pot"] = (key >> np.uint64(32)).astype(np.uint32)
    table["min_pot_cell"] = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for name, v, f, start in (("x0", x, np.minimum, 0xFFFF), ("y0", y, np.minimum, 0xFFFF), ("x1", x, np.maximum, 0), ("y1", y, np.maximum, 0)):
        acc = np.full(n_written, start, np.int64)
        f.at(acc, k, v)
        table[name] = acc
    scores = [(score(q, int(t["min_pot"]), int(t["n_cells"])), j) for j, t in enumerate(table) if t["min_pot"] != UNREACHABLE]
    best_score, best = min(scores) if scores else (0, NONE)
    return labels.reshape(ny, nx), table, info_tuple(on.sum(), len(firsts), n_frontiers, n_written, best, best_score)


# ---- guards -----------------------------------------------------------------------------------------------------------------
def _tiles_of(cells, nx, tile):
    return {((c % nx) // tile, (c // nx) // tile) for c in cells}


def guards(image, cost, pot, q, result, names, tile=32):
    """What a designed case must hold, on the restatement's result for the image at hand; raises AssertionError by name.
    several_tiles: one frontier has cells in at least four tiles. corner_only: two frontier cells of one frontier are diagonal
    neighbours in tiles that differ along both axes, and 4-connectivity puts them into different components. re_enters: the
    cells of one frontier inside one tile form two or more components of that tile alone. unreachable: a table entry has no
    reachable cell. three_frontiers, small_component, all_three_values, none: what they say."""
    labels, table, info = result
    ny, nx = image.shape
    flat = labels.ravel()
    cells_of = {}
    for c in np.flatnonzero(flat != NONE).tolist():
        cells_of.setdefault(int(flat[c]), []).append(c)
    mask = frontier_mask(image, cost, q)
    for name in names:
        if name == "several_tiles":
            ok = any(len(_tiles_of(cs, nx, tile)) >= 4 for cs in cells_of.values())
        elif name == "corner_only":
            four = roots_of(mask, FOUR)
            ok = False
            for y, x in np.argwhere(mask[:-1]).tolist():
                for dx in (-1, 1):
                    if 0 <= x + dx < nx and mask[y + 1, x + dx] and x // tile != (x + dx) // tile and y // tile != (y + 1) // tile:
                        ok |= bool(four[y, x] != four[y + 1, x + dx] and labels[y, x] == labels[y + 1, x + dx] != NONE)
        elif name == "re_enters":
            ok = False
            for cs in cells_of.values():
                for tx, ty in _tiles_of(cs, nx, tile):
                    sub = np.zeros((tile, tile), bool)
                    for c in cs:
                        if ((c % nx) // tile, (c // nx) // tile) == (tx, ty):
                            sub[c // nx - ty * tile, c % nx - tx * tile] = True
                    ok |= len(np.unique(roots_of(sub)[sub])) >= 2
        elif name == "unreachable":
            ok = bool((table["min_pot"] == UNREACHABLE).any()) and bool((table["min_pot_cell"][table["min_pot"] == UNREACHABLE] == NONE).all())
        elif name == "three_frontiers":
            ok = info[2] >= 3
        elif name == "small_component":
            ok = info[1] > info[2]
        elif name == "all_three_values":
            ok = set(np.unique(image).tolist()) == {-1, 0, 100}
        elif name == "none":
            ok = info[0] == 0 and info[2] == 0 and (flat == NONE).all()
        else:
            raise KeyError(name)
        assert ok, f"the case does not hold '{name}'"
