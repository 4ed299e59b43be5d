"""numpy restatements of the rolling log-odds occupancy map (include/cloudmerge.h, cm_map_integrate), steps 1-8, written twice
and independently of the kernels. MapVectorised keeps the window as an array and scrolls it by slices; per integration the cells
are np.float32 array arithmetic, the rays the closed form of the grid rays' step 5 in int64 and the evidence whole-array
integer arithmetic. MapLoop keeps a dictionary of absolute cells, so that scrolling is forgetting the keys outside the new
window; it takes one point, one ray (tests/rays_ref.py's walk) and one cell after the other with Python integers. Both take
per frame the clouds A (cm_merged_copy) and G (cm_ground_copy) as (n, 4) float32 arrays, the descriptor sensor of every point
of either, the sensors' (x, y, z) translations and the pose, and return (table, image, info): MAP_DTYPE of shape (ny, nx), int8
of shape (ny, nx) and a dictionary with the cm_map_info fields and what the vacuity guards look at."""
import numpy as np

from tests import grid_ref as gr
from tests import rays_ref as rr

F32 = np.float32
MAP_DTYPE = np.dtype([("logodds", "<i4"), ("n_obs", "<u4")])
MAX_CELLS = 1 << 22
MAX_LOGODDS = 1 << 20
LIMIT = F32(1073741824.0)
DEFAULTS = dict(z_band=(-np.inf, np.inf), l_hit=85, l_miss=40, l_min=-200, l_max=350, l_free=-40, l_occ=85, max_range_cells=0)


def params(cell, nx, ny, **kw):
    q = dict(DEFAULTS, cell=cell, nx=nx, ny=ny)
    assert set(kw) <= set(DEFAULTS), kw
    q.update(kw)
    return q


def refusal(q):
    """Why cm_map_configure refuses q, or None: the list of include/cloudmerge.h in its order."""
    with np.errstate(all="ignore"):
        cell = F32(q["cell"])
        if not (np.isfinite(cell) and cell > 0):
            return "cell"
        inv = F32(1.0) / cell
        if not (np.isfinite(inv) and inv > 0):
            return "inv"
    if q["nx"] == 0 or q["ny"] == 0 or q["nx"] * q["ny"] > MAX_CELLS:
        return "size"
    z0, z1 = F32(q["z_band"][0]), F32(q["z_band"][1])
    if np.isnan(z0) or np.isnan(z1) or z0 > z1:
        return "band"
    if q["l_hit"] < 1 or q["l_miss"] < 1:
        return "step"
    if any(abs(q[k]) > MAX_LOGODDS for k in ("l_hit", "l_miss", "l_min", "l_max", "l_free", "l_occ")):
        return "magnitude"
    if not (q["l_min"] <= q["l_free"] < q["l_occ"] <= q["l_max"]) or not (q["l_min"] <= 0 <= q["l_max"]):
        return "order"
    return None


def pose_ok(P):
    return bool(np.isfinite(np.asarray(P, F32)).all())


def cell_of_scalar(w, inv):
    """Step 1 on one axis for one value: the absolute cell, or None where it does not exist."""
    with np.errstate(all="ignore"):
        c = np.floor(F32(F32(w) * inv))
    return int(c) if (c > -LIMIT and c < LIMIT) else None


def row_scalar(P, r, t):
    with np.errstate(all="ignore"):
        a = F32(F32(P[r, 0] * F32(t[0])) + F32(P[r, 1] * F32(t[1])))
        return F32(F32(a + F32(P[r, 2] * F32(t[2]))) + P[r, 3])


def vehicle_cell(P, cell):
    """Step 2: (vx, vy), or None where the cell does not exist."""
    P = np.asarray(P, F32).reshape(3, 4)
    inv = F32(1.0) / F32(cell)
    v = (cell_of_scalar(P[0, 3], inv), cell_of_scalar(P[1, 3], inv))
    return None if None in v else v


def anchor_of(v, nx, ny):
    return v[0] - nx // 2, v[1] - ny // 2


def image_of(logodds, n_obs, q):
    img = np.where(n_obs == 0, -1, np.where(logodds >= q["l_occ"], 100, np.where(logodds <= q["l_free"], 0, -1)))
    return img.astype(np.int8)


def _info(anchor, q, n_frames, cast, **guards):
    mask = sum(1 << s for s in cast)
    return dict(anchor=tuple(anchor), nx=q["nx"], ny=q["ny"], n_frames=n_frames, sensors_cast=mask, **guards)


# ---- vectorised ---------------------------------------------------------------------------------------------------------
class MapVectorised:
    def __init__(self, q):
        assert refusal(q) is None, refusal(q)
        self.q = q
        self.table = np.zeros((q["ny"], q["nx"]), MAP_DTYPE)
        self.anchor = None
        self.n_frames = 0

    def window_cells(self, pts, tag, P, anchor):
        """Steps 1 and 3: per counted point its window cell index, and its sensor."""
        q = self.q
        nx, ny = q["nx"], q["ny"]
        inv = F32(1.0) / F32(q["cell"])
        x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
        with np.errstate(all="ignore"):
            wx = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
            wy = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
            assert wx.dtype == F32 and wy.dtype == F32
            cx, cy = np.floor(wx * inv), np.floor(wy * inv)
            ok = (cx > -LIMIT) & (cx < LIMIT) & (cy > -LIMIT) & (cy < LIMIT)
            ok &= (F32(q["z_band"][0]) <= z) & (z <= F32(q["z_band"][1]))
        gx = np.where(ok, cx, 0).astype(np.int64) - anchor[0]
        gy = np.where(ok, cy, 0).astype(np.int64) - anchor[1]
        ok &= (gx >= 0) & (gx < nx) & (gy >= 0) & (gy < ny)
        return (gx + gy * nx)[ok], tag[ok]

    def integrate(self, A, G, sensor_a, sensor_g, translations, P):
        q = self.q
        nx, ny = q["nx"], q["ny"]
        n_cells = nx * ny
        P = np.asarray(P, F32).reshape(3, 4)
        A, G = gr.a4(A), gr.a4(G)
        v = vehicle_cell(P, q["cell"])
        assert pose_ok(P) and v is not None
        anchor = anchor_of(v, nx, ny)
        n_sensors = len(translations)
        ia, ta = self.window_cells(A, np.asarray(sensor_a, np.int64).reshape(-1), P, anchor)
        ig, tg = self.window_cells(G, np.asarray(sensor_g, np.int64).reshape(-1), P, anchor)
        assert ((ta >= 0) & (ta < n_sensors)).all() and ((tg >= 0) & (tg < n_sensors)).all()
        inv = F32(1.0) / F32(q["cell"])
        n_pass = np.zeros(n_cells, np.int64)
        n_hit = np.zeros(n_cells, np.int64)
        n_ground = np.zeros(n_cells, np.int64)
        cast, n_rays, longest = [], 0, 0
        for s in range(n_sensors):
            H = np.unique(ia[ta == s])
            E = np.union1d(H, ig[tg == s])
            n_hit[H] += 1
            n_ground[np.setdiff1d(E, H)] += 1
            o = (cell_of_scalar(row_scalar(P, 0, translations[s]), inv), cell_of_scalar(row_scalar(P, 1, translations[s]), inv))
            if None in o:
                continue
            o = (o[0] - anchor[0], o[1] - anchor[1])
            if not (0 <= o[0] < nx and 0 <= o[1] < ny):
                continue
            cast.append(s)
            n_rays += len(E)
            # the closed form of the grid rays' step 5, every ray's np.arange(K) one behind the other
            dx, dy = E % nx - o[0], E // nx - o[1]
            L = np.maximum(np.abs(dx), np.abs(dy))
            longest = max(longest, int(L.max()) if len(L) else 0)
            K = L if q["max_range_cells"] == 0 else np.minimum(L, q["max_range_cells"])
            ray = np.repeat(np.arange(len(E), dtype=np.int64), K)
            k = np.arange(int(K.sum()), dtype=np.int64) - np.repeat(np.cumsum(K) - K, K)
            ax_, ay_, l = k * dx[ray], k * dy[ray], L[ray]
            x = o[0] + np.sign(ax_) * ((2 * np.abs(ax_) + l) // (2 * l))
            y = o[1] + np.sign(ay_) * ((2 * np.abs(ay_) + l) // (2 * l))
            np.add.at(n_pass, x + y * nx, 1)
        d = np.where(n_hit > 0, q["l_hit"] * n_hit, -q["l_miss"] * (n_pass + n_ground)).reshape(ny, nx)
        # step 7: the part of the old window that the new one still covers, by slices
        new = np.zeros((ny, nx), MAP_DTYPE)
        carried = dropped = 0
        if self.anchor is not None:
            sx, sy = anchor[0] - self.anchor[0], anchor[1] - self.anchor[1]
            x0, x1 = max(0, -sx), min(nx, nx - sx)
            y0, y1 = max(0, -sy), min(ny, ny - sy)
            seen = int((self.table["n_obs"] > 0).sum())
            if x0 < x1 and y0 < y1:
                part = self.table[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
                new[y0:y1, x0:x1] = part
                carried = int((part["n_obs"] > 0).sum())
            dropped = seen - carried
        total = new["logodds"].astype(np.int64) + d
        clamped = int(((d != 0) & ((total < q["l_min"]) | (total > q["l_max"]))).sum())
        new["logodds"] = np.where(d != 0, np.clip(total, q["l_min"], q["l_max"]), new["logodds"])
        new["n_obs"] = np.where(d != 0, np.minimum(new["n_obs"].astype(np.int64) + 1, 0xFFFFFFFF), new["n_obs"])
        self.table, self.anchor = new, anchor
        self.n_frames += 1
        image = image_of(new["logodds"], new["n_obs"], q)
        info = _info(anchor, q, self.n_frames, cast, clamped=clamped, carried=carried, dropped=dropped,
                     hit_over_pass=int(((n_hit > 0) & (n_pass > 0)).sum()), ground_only=int(((n_hit == 0) & (n_ground > 0)).sum()),
                     n_rays=n_rays, longest=longest, steps=int(n_pass.sum()))
        return new.copy(), image, info


# ---- one thing after the other --------------------------------------------------------------------------------------------
class MapLoop:
    def __init__(self, q):
        assert refusal(q) is None, refusal(q)
        self.q = q
        self.cells = {}                                  # absolute cell -> [logodds, n_obs]
        self.n_frames = 0

    def integrate(self, A, G, sensor_a, sensor_g, translations, P):
        q = self.q
        nx, ny = q["nx"], q["ny"]
        P = np.asarray(P, F32).reshape(3, 4)
        inv = F32(1.0) / F32(q["cell"])
        v = vehicle_cell(P, q["cell"])
        assert pose_ok(P) and v is not None
        ax, ay = anchor_of(v, nx, ny)
        z0, z1 = F32(q["z_band"][0]), F32(q["z_band"][1])
        n_sensors = len(translations)
        E = [set() for _ in range(n_sensors)]
        H = [set() for _ in range(n_sensors)]
        for pts, tags, sets in ((gr.a4(A), sensor_a, (E, H)), (gr.a4(G), sensor_g, (E,))):
            for (x, y, z, _), s in zip(pts, np.asarray(tags, np.int64).reshape(-1).tolist()):
                if not (z0 <= z and z <= z1):
                    continue
                g = (cell_of_scalar(row_scalar(P, 0, (x, y, z)), inv), cell_of_scalar(row_scalar(P, 1, (x, y, z)), inv))
                if None in g or not (ax <= g[0] < ax + nx and ay <= g[1] < ay + ny):
                    continue
                for group in sets:
                    group[s].add(g)
        n_pass = {}
        cast = []
        for s in range(n_sensors):
            o = (cell_of_scalar(row_scalar(P, 0, translations[s]), inv), cell_of_scalar(row_scalar(P, 1, translations[s]), inv))
            if None in o or not (ax <= o[0] < ax + nx and ay <= o[1] < ay + ny):
                continue
            cast.append(s)
            for e in E[s]:
                for c in rr.walk(o, e, q["max_range_cells"]):          # (the walk is translation-invariant: absolute cells)
                    n_pass[c] = n_pass.get(c, 0) + 1
        kept = {}
        for gy in range(ay, ay + ny):
            for gx in range(ax, ax + nx):
                c = (gx, gy)
                logodds, n_obs = self.cells.get(c, (0, 0))
                n_hit = sum(c in H[s] for s in range(n_sensors))
                n_ground = sum(c in E[s] and c not in H[s] for s in range(n_sensors))
                d = q["l_hit"] * n_hit if n_hit else -q["l_miss"] * (n_pass.get(c, 0) + n_ground)
                if d != 0:
                    logodds = min(max(logodds + d, q["l_min"]), q["l_max"])
                    n_obs = min(n_obs + 1, 0xFFFFFFFF)
                if logodds or n_obs:
                    kept[c] = (logodds, n_obs)
        self.cells = kept
        self.n_frames += 1
        table = np.zeros((ny, nx), MAP_DTYPE)
        image = np.full((ny, nx), -1, np.int8)
        for (gx, gy), (logodds, n_obs) in kept.items():
            table[gy - ay, gx - ax] = (logodds, n_obs)
            if n_obs:
                image[gy - ay, gx - ax] = 100 if logodds >= q["l_occ"] else 0 if logodds <= q["l_free"] else -1
        return table, image, _info((ax, ay), q, self.n_frames, cast)


def guards(history, ground=False):
    """The conditions that keep a comparison from being vacuous, on the restatement's own output over a whole sequence:
    history is the list of (table, image, info) of MapVectorised."""
    values = set()
    for _, image, _ in history:
        values |= set(image.ravel().tolist())
    assert values == {-1, 0, 100}, "the images do not hold all three values"
    assert any(i["clamped"] for _, _, i in history), "no cell is clamped"
    assert any(i["hit_over_pass"] for _, _, i in history), "no hit overrides passes"
    if ground:
        assert any(i["ground_only"] for _, _, i in history), "no cell is a ground-only end"


def scroll_guards(history):
    assert any(i["carried"] for _, _, i in history), "no observed cell is carried across a scroll"
    assert any(i["dropped"] for _, _, i in history), "no observed cell is dropped by a scroll"
    assert len({i["anchor"] for _, _, i in history}) > 1, "the window never moves"
