"""The plan layer behind the cost layer (cm_map_plan_configure, cm_map_plan_update, cm_map_plan_path; the numbered semantics in
include/cloudmerge.h) restated twice with numpy and the standard library only: a heap Dijkstra from the goal
(potential_dijkstra) and a relaxation of the whole image at once, run to its fixed point (potential_relaxed). Both are written
from the header's steps, not from the kernels: no tiles, no flags, no sweeps. All step costs are positive integers, so the two
and the device agree in every word or one of them is wrong. With them: the walk of step 6 (walk), the goal's and the start's
window cell (window_cell), the refusals of cm_map_plan_configure (refusal) and the guards that say what a designed case holds."""
import heapq

import numpy as np

F32 = np.float32
UNREACHABLE = 0xFFFFFFFF
ALLOW_UNKNOWN = 1
FOUND, PATH_UNREACHABLE, TRUNCATED = 0, 1, 2
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))         # step 3: direction d is DIRS[d]


def params(neutral=50, cost_factor_q8=205, flags=0, max_path_cells=None):
    return dict(neutral=neutral, cost_factor_q8=cost_factor_q8, flags=flags, max_path_cells=max_path_cells)


def weights(cost, q):
    """Step 1: (ny, nx) int64, 0 where the cell is impassable."""
    v = np.asarray(cost).astype(np.int64)
    if q["flags"] & ALLOW_UNKNOWN:
        v = np.where(v == 255, 252, v)
    return np.where(v >= 253, 0, q["neutral"] + ((v * q["cost_factor_q8"]) >> 8))


def w_max(q):
    return q["neutral"] + ((252 * q["cost_factor_q8"]) >> 8)


def refusal(q, nx=16, ny=8, have_cost=True, in_flight=False):
    """Why cm_map_plan_configure refuses, or None."""
    if in_flight:
        return "flight"
    if not have_cost:
        return "cost"
    if not 1 <= q["neutral"] <= 255:
        return "neutral"
    if not 0 <= q["cost_factor_q8"] <= 256:
        return "factor"
    if q["flags"] & ~ALLOW_UNKNOWN:
        return "flags"
    if not 1 <= q["max_path_cells"] <= nx * ny:
        return "max_path_cells"
    if 7 * w_max(q) * (nx * ny - 1) > 0xFFFFFFFE:                                       # step 5, in Python's integers
        return "range"
    return None


def window_cell(x, y, cell, anchor, nx, ny):
    """Step 2: the window cell (ix, iy) of a world position, or None."""
    inv = F32(1.0) / F32(cell)
    out = []
    for w, a, n in ((x, anchor[0], nx), (y, anchor[1], ny)):
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.floor(F32(w) * inv)
        if not (c > F32(-1073741824.0) and c < F32(1073741824.0)):
            return None
        i = int(c) - a
        if not 0 <= i < n:
            return None
        out.append(i)
    return tuple(out)


def cell_centre(ix, iy, cell, anchor):
    """A world position inside window cell (ix, iy)."""
    return (anchor[0] + ix + 0.5) * cell, (anchor[1] + iy + 0.5) * cell


def passable_of(w, goal):
    p = w > 0
    p[goal[1], goal[0]] = True                                                           # step 2: in the corner rule
    return p


def step_exists(p, x, y, d):
    """Step 3 between (x, y) and its neighbour in direction d, as far as it depends on other cells: the neighbour lies in the
    window and, for a diagonal step, both cells that share an edge with both are passable."""
    ny, nx = p.shape
    dx, dy = DIRS[d]
    if not (0 <= x + dx < nx and 0 <= y + dy < ny):
        return False
    return dx == 0 or dy == 0 or bool(p[y, x + dx] and p[y + dy, x])


def potential_dijkstra(cost, q, goal):
    """Step 4 by a heap from the goal: settling n offers pot(n) + k * w(c) to every passable c with a step to n."""
    w = weights(cost, q)
    p = passable_of(w, goal)
    ny, nx = w.shape
    pot = np.full((ny, nx), UNREACHABLE, np.uint64)
    pot[goal[1], goal[0]] = 0
    heap = [(0, goal[0], goal[1])]
    done = np.zeros((ny, nx), bool)
    while heap:
        d0, x, y = heapq.heappop(heap)
        if done[y, x]:
            continue
        done[y, x] = True
        for d, (dx, dy) in enumerate(DIRS):
            if not step_exists(p, x, y, d):
                continue
            cx, cy = x + dx, y + dy
            if w[cy, cx] == 0 or done[cy, cx]:
                continue
            nd = d0 + (7 if dx and dy else 5) * int(w[cy, cx])
            if nd < pot[cy, cx]:
                pot[cy, cx] = nd
                heapq.heappush(heap, (nd, cx, cy))
    assert int(pot[pot != UNREACHABLE].max()) < UNREACHABLE
    return pot.astype(np.uint32)


def potential_relaxed(cost, q, goal):
    """Step 4 by relaxing every cell of the image at once from all eight neighbours until nothing changes."""
    w = weights(cost, q)
    p = passable_of(w, goal)
    ny, nx = w.shape
    FAR = 1 << 62
    pot = np.full((ny + 2, nx + 2), FAR, np.int64)
    pot[goal[1] + 1, goal[0] + 1] = 0
    pp = np.zeros((ny + 2, nx + 2), bool)
    pp[1:-1, 1:-1] = p
    inner = lambda a, dx, dy: a[1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx]
    movable = w > 0
    movable[goal[1], goal[0]] = False
    for _ in range(nx * ny + 1):
        best = inner(pot, 0, 0).copy()
        for dx, dy in DIRS:
            ok = movable & (inner(pot, dx, dy) < FAR)
            if dx and dy:
                ok &= inner(pp, dx, 0) & inner(pp, 0, dy)
            cand = np.where(ok, inner(pot, dx, dy) + (7 if dx and dy else 5) * w, FAR)
            best = np.minimum(best, cand)
        if (best == inner(pot, 0, 0)).all():
            break
        pot[1:-1, 1:-1] = best
    else:
        raise AssertionError("no fixed point")
    out = inner(pot, 0, 0)
    return np.where(out >= FAR, UNREACHABLE, out).astype(np.uint32)


def walk(pot, cost, q, goal, start, max_path_cells):
    """Step 6: (cells as a uint32 array of ix + iy * nx, status, pot(start))."""
    w = weights(cost, q)
    p = passable_of(w, goal)
    ny, nx = w.shape
    x, y = start
    pot_start = int(pot[y, x])
    if pot_start == UNREACHABLE:
        return np.zeros(0, np.uint32), PATH_UNREACHABLE, pot_start
    cells = []
    while len(cells) < max_path_cells:
        cells.append(x + y * nx)
        if (x, y) == tuple(goal):
            return np.array(cells, np.uint32), FOUND, pot_start
        best = None
        for d, (dx, dy) in enumerate(DIRS):
            if step_exists(p, x, y, d) and pot[y + dy, x + dx] != UNREACHABLE:
                v = int(pot[y + dy, x + dx]) + (7 if dx and dy else 5) * int(w[y, x])
                if best is None or v < best[0]:                                          # (a tie keeps the lower direction)
                    best = (v, d)
        assert best is not None and best[0] == int(pot[y, x]), "pot is not a fixed point"
        x, y = x + DIRS[best[1]][0], y + DIRS[best[1]][1]
    return np.array(cells, np.uint32), TRUNCATED, pot_start


def ties(pot, cost, q, goal, x, y):
    """The directions that reach the minimum of step 6 at (x, y)."""
    w = weights(cost, q)
    p = passable_of(w, goal)
    vals = {d: int(pot[y + dy, x + dx]) + (7 if dx and dy else 5) * int(w[y, x]) for d, (dx, dy) in enumerate(DIRS)
            if step_exists(p, x, y, d) and pot[y + dy, x + dx] != UNREACHABLE}
    return sorted(d for d, v in vals.items() if v == min(vals.values())) if vals else []


def check_path(cells, status, pot, cost, q, goal):
    """The invariants of a path that was not cut: every step exists, pot strictly decreases along it, the step costs sum to
    pot(start), it ends at the goal."""
    w = weights(cost, q)
    p = passable_of(w, goal)
    ny, nx = w.shape
    xy = [(int(c) % nx, int(c) // nx) for c in cells]
    total = 0
    for (x, y), (u, v) in zip(xy, xy[1:]):
        d = DIRS.index((u - x, v - y))
        assert step_exists(p, x, y, d) and w[y, x] > 0 and pot[v, u] < pot[y, x]
        total += (7 if d & 1 else 5) * int(w[y, x])
    if status == FOUND:
        assert xy[-1] == tuple(goal) and total == int(pot[xy[0][1], xy[0][0]])
    else:
        assert status == TRUNCATED and tuple(goal) not in xy
    return total


def closed_form(nx, ny, goal, neutral):
    """pot of an image of uniform cost 0: |dx - dy| straight steps and min(dx, dy) diagonal ones."""
    dx = np.abs(np.arange(nx, dtype=np.int64) - goal[0])[None, :]
    dy = np.abs(np.arange(ny, dtype=np.int64) - goal[1])[:, None]
    return (neutral * (5 * np.abs(dx - dy) + 7 * np.minimum(dx, dy))).astype(np.uint32)


def guards(pot, cost, q, goal, need):
    """What a designed case must contain, by name, asserted on the restatement's output."""
    w = weights(cost, q)
    passable = w > 0
    reach = pot != UNREACHABLE
    assert pot[goal[1], goal[0]] == 0 and not (reach & ~passable_of(w, goal)).any()
    for name in need:
        if name == "mostly_reachable":
            assert (reach & passable).sum() > 0.9 * passable.sum(), name
        elif name == "some_unreachable":
            assert (passable & ~reach).any(), name
        elif name == "goal_impassable":
            assert not passable[goal[1], goal[0]], name
        elif name == "nothing_passable":
            assert not passable.any() and reach.sum() == 1, name
        elif name == "graded":
            assert len(np.unique(w[passable])) > 3, name
        elif name == "several_tiles":
            assert reach[:, 0].any() and reach[:, -1].any() and reach[0].any() and reach[-1].any(), name
        elif name == "detour":                          # some cell's path is far longer than the straight line
            assert (pot[reach].astype(np.int64) > 3 * closed_form(pot.shape[1], pot.shape[0], goal, int(w[passable].max()))[reach]).any(), name
        else:
            raise KeyError(name)
