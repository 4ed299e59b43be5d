"""numpy restatements of the free-space ray casting over the grid map (include/cloudmerge.h, cm_result_grid_rays), steps 2-7,
written twice and independently of the kernels: rays_vectorised (per ray the closed form of step 5 over np.arange(K) in int64,
np.add.at) and rays_loop (one step after the other with the incremental error term: it starts at L, grows by 2 |d| per step
and wraps at 2 L, all below 2^32). Both take the clouds A (cm_merged_copy) and G (cm_ground_copy) as (n, 4) float32 arrays, the
descriptor sensor of every point of either, and the sensors' (x, y) translations, and return (table, cleared, info): RAY_DTYPE
of shape (ny, nx), int8 of shape (ny, nx), and what the vacuity guards look at. The base map is tests/grid_ref.py's."""
import numpy as np

from tests import grid_ref as gr

F32 = np.float32
RAY_DTYPE = np.dtype([("n_pass", "<u4"), ("n_end", "<u4")])


def origin_cells(translations, origin, cell, nx, ny):
    """Step 3: per sensor (ox, oy), or None where the origin is outside the grid or not finite."""
    inv = F32(1.0) / F32(cell)
    out = []
    with np.errstate(all="ignore"):
        for t in translations:
            cx = np.floor(F32(F32(F32(t[0]) - F32(origin[0])) * inv))
            cy = np.floor(F32(F32(F32(t[1]) - F32(origin[1])) * inv))
            ok = cx >= F32(0) and cx < F32(nx) and cy >= F32(0) and cy < F32(ny)
            out.append((int(cx), int(cy)) if ok else None)
    return out


def ray_set(A, G, sensor_a, sensor_g, n_sensors, origin, cell, nx, ny, z_band):
    """Steps 2 and 4: per sensor the sorted distinct cells of its counted points (of A and G alike)."""
    pts = np.concatenate([gr.a4(A), gr.a4(G)])
    tag = np.concatenate([np.asarray(sensor_a, np.int64).reshape(-1), np.asarray(sensor_g, np.int64).reshape(-1)])
    assert len(tag) == len(pts) and (tag >= 0).all() and (tag < n_sensors).all()
    idx, ok = gr.cells_of(pts, origin, cell, nx, ny, *z_band)
    tag = tag[ok]
    return [np.unique(idx[tag == s]) for s in range(n_sensors)]


def cleared_image(base, n_pass, min_pass):
    """Step 7."""
    state = base["state"]
    img = np.where(state == gr.OCCUPIED, 100, np.where((state == gr.FREE) | (n_pass >= min_pass), 0, -1))
    return img.astype(np.int8)


def _finish(base, base_image, per_sensor_pass, n_end, min_pass, ties, steep, nx, ny):
    t = np.zeros(nx * ny, RAY_DTYPE)
    total = np.zeros(nx * ny, np.int64)
    for p in per_sensor_pass:
        total += p
    t["n_pass"] = total
    t["n_end"] = n_end
    t = t.reshape(ny, nx)
    cleared = cleared_image(base, t["n_pass"], min_pass)
    info = dict(base=base, base_image=base_image, ties=ties, steep=steep,
                two_sensors=int((np.sum([p > 0 for p in per_sensor_pass], axis=0) >= 2).sum()) if per_sensor_pass else 0,
                n_rays=int(n_end.sum()))
    return t, cleared, info


def rays_vectorised(A, G, sensor_a, sensor_g, translations, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3,
                    min_points=1, min_pass=1, max_range_cells=0):
    base, base_image = gr.grid_vectorised(A, G, origin, cell, nx, ny, z_band, obstacle_height, min_points)
    ends = ray_set(A, G, sensor_a, sensor_g, len(translations), origin, cell, nx, ny, z_band)
    per = []
    n_end = np.zeros(nx * ny, np.int64)
    ties = steep = 0
    for o, cells in zip(origin_cells(translations, origin, cell, nx, ny), ends):
        if o is None:
            continue
        p = np.zeros(nx * ny, np.int64)
        np.add.at(n_end, cells, 1)
        dx, dy = cells % nx - o[0], cells // nx - o[1]
        L = np.maximum(np.abs(dx), np.abs(dy))
        K = L if max_range_cells == 0 else np.minimum(L, max_range_cells)
        steep += int((np.abs(dy) > np.abs(dx)).sum())
        # every ray's np.arange(K), one behind the other (int64 throughout)
        ray = np.repeat(np.arange(len(cells), dtype=np.int64), K)
        k = np.arange(int(K.sum()), dtype=np.int64) - np.repeat(np.cumsum(K) - K, K)
        ax, ay, l = k * dx[ray], k * dy[ray], L[ray]
        x = o[0] + np.sign(ax) * ((2 * np.abs(ax) + l) // (2 * l))
        y = o[1] + np.sign(ay) * ((2 * np.abs(ay) + l) // (2 * l))
        tie = ((2 * np.abs(ax)) % (2 * l) == l) | ((2 * np.abs(ay)) % (2 * l) == l)
        ties += len(np.unique(ray[tie]))
        np.add.at(p, x + y * nx, 1)
        per.append(p)
    return _finish(base, base_image, per, n_end, min_pass, int(ties), int(steep), nx, ny)


def walk(o, e, max_range_cells=0):
    """The cells one ray crosses, in order, by the incremental form of step 5."""
    dx, dy = e[0] - o[0], e[1] - o[1]
    ax, ay = abs(dx), abs(dy)
    L = max(ax, ay)
    K = L if max_range_cells == 0 else min(L, max_range_cells)
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    x, y = o
    ex = ey = L                                    # the error terms: (2 k |d| + L) mod 2 L
    out = []
    for _ in range(K):
        out.append((x, y))
        ex += 2 * ax
        ey += 2 * ay
        assert ex < 1 << 32 and ey < 1 << 32
        if ex >= 2 * L:
            ex -= 2 * L
            x += sx
        if ey >= 2 * L:
            ey -= 2 * L
            y += sy
    return out


def rays_loop(A, G, sensor_a, sensor_g, translations, origin, cell, nx, ny, z_band=(-np.inf, np.inf), obstacle_height=0.3,
              min_points=1, min_pass=1, max_range_cells=0):
    base, base_image = gr.grid_loop(A, G, origin, cell, nx, ny, z_band, obstacle_height, min_points)
    ends = ray_set(A, G, sensor_a, sensor_g, len(translations), origin, cell, nx, ny, z_band)
    per = []
    n_end = np.zeros(nx * ny, np.int64)
    steep = 0
    for o, cells in zip(origin_cells(translations, origin, cell, nx, ny), ends):
        if o is None:
            continue
        p = np.zeros(nx * ny, np.int64)
        for e in cells.tolist():
            n_end[e] += 1
            steep += abs(e // nx - o[1]) > abs(e % nx - o[0])
            for x, y in walk(o, (e % nx, e // nx), max_range_cells):
                p[x + y * nx] += 1
        per.append(p)
    return _finish(base, base_image, per, n_end, min_pass, -1, int(steep), nx, ny)


def guards(table, cleared, info, min_pass=1):
    """The conditions that keep a comparison from being vacuous, on the restatement's own output."""
    base = info["base"]["state"]
    assert set(cleared.ravel().tolist()) == {-1, 0, 100}, "the cleared image does not hold all three values"
    assert ((base == gr.UNKNOWN) & (cleared == 0)).any(), "no cell flips from UNKNOWN to FREE"
    assert ((base == gr.OCCUPIED) & (table["n_pass"] >= min_pass) & (cleared == 100)).any(), "no OCCUPIED cell is crossed"
    assert info["two_sensors"] > 0, "no cell is crossed by rays of two sensors"
    assert info["ties"] > 0, "no ray takes a tie step"
    assert info["steep"] > 0, "no ray has |dy| > |dx|"
