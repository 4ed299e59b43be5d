"""The rollout layer restated from the numbered list of include/cloudmerge.h alone (cm_map_traj_configure, cm_map_traj_evaluate):
numpy fp32 and double scalars, one trajectory and one pose at a time, the points of a pose as one fp32 array. No waves, no
lanes, no batches. Every fp32 operation is a numpy float32 operation of its own, so nothing is fused."""
import numpy as np

F32 = np.float32
F64 = np.float64
MAX_SAMPLES, MAX_STEPS, MAX_FOOT, HEADINGS = 16384, 256, 256, 4096
ALLOW_UNKNOWN = 1
NONE = 0xFFFFFFFF
VALID, COLLISION, OFF_MAP, NO_POTENTIAL = 0, 1, 2, 3
UNREACHABLE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
K = F64(4294967296.0) / F64(6.283185307179586)
PI = 3.141592653589793
SCORE = np.dtype([("status", "<u4"), ("bad_step", "<u4"), ("occ", "<u4"), ("pot_end", "<u4"), ("total", "<u8"), ("end_x", "<f4"), ("end_y", "<f4")])


def params(nv=1, nw=1, n_steps=1, occ_scale=1, goal_scale=1, flags=0):
    return dict(nv=nv, nw=nw, n_steps=n_steps, occ_scale=occ_scale, goal_scale=goal_scale, flags=flags)


def window(x, y, yaw=0.0, v=(0.0, 0.0), w=(0.0, 0.0), dt=0.1):
    return dict(x=x, y=y, yaw=yaw, v_lo=v[0], v_hi=v[1], w_lo=w[0], w_hi=w[1], dt=dt)


def table():
    """Step 2 with numpy's cos and sin (the library's comes from libm: the two may differ by an ulp off the axes)."""
    th = np.arange(HEADINGS, dtype=F64) * (F64(6.283185307179586) / F64(4096.0))
    t = np.stack([np.cos(th), np.sin(th)], axis=1).astype(F32)
    t[0], t[1024], t[2048], t[3072] = (1, 0), (0, 1), (-1, 0), (0, -1)
    return t


def samples(lo, hi, n):
    """Step 1: n fp32 samples."""
    lo, hi = F32(lo), F32(hi)
    if n == 1:
        return [lo]
    with np.errstate(over="ignore", invalid="ignore"):
        step = (hi - lo) / F32(n - 1)
        return [lo + F32(i) * step for i in range(n)]


def increment(w, dt):
    """Step 1: dh of one angular sample, mod 2^32."""
    return int(np.rint((F64(F32(w)) * F64(F32(dt))) * K)) & 0xFFFFFFFF


def start_heading(yaw):
    return int(np.rint(F64(F32(yaw)) * K)) & 0xFFFFFFFF


def entry(h):
    return (((h + 0x80000) & 0xFFFFFFFF) >> 20) & 4095


def cells_of(wx, wy, cell, anchor, nx, ny):
    """Step 4's cells of fp32 arrays of world coordinates: (on map, ix, iy)."""
    inv = F32(1.0) / F32(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        cx, cy = np.floor(wx * inv), np.floor(wy * inv)
    lim = F32(1073741824.0)
    exists = (cx > -lim) & (cx < lim) & (cy > -lim) & (cy < lim)
    ix = np.where(exists, cx, 0).astype(np.int64) - anchor[0]
    iy = np.where(exists, cy, 0).astype(np.int64) - anchor[1]
    on = exists & (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    return on, np.where(on, ix, 0), np.where(on, iy, 0)


def refusal(q, foot, win=None, cell=0.1, anchor=(0, 0), nx=16, ny=8, have_plan=True, pot_fresh=True, in_flight=False):
    """Why cm_map_traj_configure (win None) or cm_map_traj_evaluate refuses, or None."""
    if in_flight:
        return "flight"
    if not have_plan:
        return "plan"
    if win is None:
        if q["nv"] < 1 or q["nw"] < 1 or q["nv"] * q["nw"] > MAX_SAMPLES:
            return "samples"
        if not 1 <= q["n_steps"] <= MAX_STEPS:
            return "steps"
        if q["flags"] & ~ALLOW_UNKNOWN:
            return "flags"
        if foot is None:
            return "footprint"
        foot = np.asarray(foot, F32).reshape(-1, 2)
        if not 1 <= len(foot) <= MAX_FOOT:
            return "n_foot"
        if not np.isfinite(foot).all():
            return "footprint"
        return None
    if not pot_fresh:
        return "stale"
    vals = [F32(win[k]) for k in ("x", "y", "yaw", "v_lo", "v_hi", "w_lo", "w_hi", "dt")]
    if not all(np.isfinite(v) for v in vals):
        return "finite"
    if F32(win["v_hi"]) < F32(win["v_lo"]):
        return "v"
    if F32(win["w_hi"]) < F32(win["w_lo"]):
        return "w"
    if not F32(win["dt"]) > 0:
        return "dt"
    if abs(F32(win["yaw"])) > 1024:
        return "yaw"
    on, _, _ = cells_of(np.array([win["x"]], F32), np.array([win["y"]], F32), cell, anchor, nx, ny)
    if not on[0]:
        return "start"
    with np.errstate(over="ignore", invalid="ignore"):
        for v in samples(win["v_lo"], win["v_hi"], q["nv"]):
            if not (np.isfinite(v) and np.isfinite(v * F32(win["dt"]))):
                return "finite"
    for w in samples(win["w_lo"], win["w_hi"], q["nw"]):
        if not np.isfinite(w) or abs(F64(w) * F64(F32(win["dt"]))) >= PI:
            return "turn"
    return None


def rollout(cost, pot, anchor, cell, q, foot, win, tab):
    """Steps 1 to 7: ((nv * nw,) SCORE array, info dict with best, n_valid, best_v, best_w, start)."""
    cost, pot = np.asarray(cost), np.asarray(pot)
    ny, nx = cost.shape
    foot = np.asarray(foot, F32).reshape(-1, 2)
    bx = np.concatenate([np.zeros(1, F32), foot[:, 0]])                # (point 0: the centre)
    by = np.concatenate([np.zeros(1, F32), foot[:, 1]])
    centre = np.zeros(len(bx), bool)
    centre[0] = True
    allow = bool(q["flags"] & ALLOW_UNKNOWN)
    dt = F32(win["dt"])
    vs, ws = samples(win["v_lo"], win["v_hi"], q["nv"]), samples(win["w_lo"], win["w_hi"], q["nw"])
    h0 = start_heading(win["yaw"])
    out = np.zeros(q["nv"] * q["nw"], SCORE)
    on, sx, sy = cells_of(np.array([win["x"]], F32), np.array([win["y"]], F32), cell, anchor, nx, ny)
    assert on[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for i, v in enumerate(vs):
            s = v * dt
            for j, w in enumerate(ws):
                dh = increment(w, win["dt"])
                x, y, h = F32(win["x"]), F32(win["y"]), h0
                rec = out[i * q["nw"] + j]
                status, bad, occ = VALID, 0, 0
                for k in range(1, q["n_steps"] + 1):
                    c, sn = tab[entry(h)]
                    x = x + s * c                                      # step 3
                    y = y + s * sn
                    h = (h + dh) & 0xFFFFFFFF
                    c, sn = tab[entry(h)]
                    wx = np.concatenate([[x], (x + c * bx[1:]) - sn * by[1:]]).astype(F32)     # step 4 (the centre is (x_k, y_k) itself)
                    wy = np.concatenate([[y], (y + sn * bx[1:]) + c * by[1:]]).astype(F32)
                    pon, ix, iy = cells_of(wx, wy, cell, anchor, nx, ny)
                    b = cost[iy, ix].astype(np.int64)                  # step 5
                    hit = pon & ((b == 254) | ((b == 255) & (not allow)) | (centre & (b == 253)))
                    if (~pon).any() or hit.any():
                        status, bad = (OFF_MAP if (~pon).any() else COLLISION), k
                        break
                    occ = max(occ, int(np.where(b == 255, 0, b).max()))
                pot_end = UNREACHABLE
                if status == VALID:                                    # step 6
                    pot_end = int(pot[iy[0], ix[0]])
                    if pot_end == UNREACHABLE:
                        status, bad = NO_POTENTIAL, q["n_steps"]
                valid = status == VALID
                rec["status"], rec["bad_step"] = status, bad
                rec["occ"] = occ if valid else 0
                rec["pot_end"] = pot_end if valid else UNREACHABLE
                rec["total"] = q["occ_scale"] * occ + q["goal_scale"] * pot_end if valid else U64_MAX
                rec["end_x"], rec["end_y"] = x, y
    good = np.flatnonzero(out["status"] == VALID)
    best = int(good[np.argmin(out["total"][good])]) if len(good) else NONE          # step 7 (argmin: the first of equals)
    info = dict(best=best, n_valid=len(good), best_v=F32(0) if best == NONE else vs[best // q["nw"]],
                best_w=F32(0) if best == NONE else ws[best % q["nw"]], start=(int(sx[0]), int(sy[0])))
    return out, info


def guards(scores, need=("share_valid", "all_statuses", "three_occ", "two_bad_steps")):
    """Named properties of a restated table, asserted before any device byte is looked at."""
    st = scores["status"]
    valid = st == VALID
    for name in need:
        if name == "share_valid":
            assert 0.10 <= valid.mean() <= 0.90, (name, float(valid.mean()))
        elif name == "all_statuses":
            assert set(st.tolist()) == {VALID, COLLISION, OFF_MAP, NO_POTENTIAL}, (name, sorted(set(st.tolist())))
        elif name == "three_occ":
            assert len(set(scores["occ"][valid].tolist())) >= 3, name
        elif name == "two_bad_steps":
            assert len(set(scores["bad_step"][(st == COLLISION) | (st == OFF_MAP)].tolist())) >= 2, name
        elif name == "some_valid":
            assert valid.any(), name
        elif name == "none_valid":
            assert not valid.any(), name
        elif name == "some_collision":
            assert (st == COLLISION).any(), name
        elif name == "some_off_map":
            assert (st == OFF_MAP).any(), name
        else:
            raise KeyError(name)
