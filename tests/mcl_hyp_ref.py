"""A restatement of the hypotheses and the recovery of the localisation layer (include/cloudmerge.h, cm_map_mcl_hyp_*), steps
H1-H6 and R1-R4, written from the header on top of tests/mcl_ref.py and independently of the kernels: the bins as a dictionary
from (by, bx, bh) to particle lists, a plain union-find over its keys, every sum as a Python integer, the doubles of the
recovery as Python floats with one operation per line. No hash table, no slots, no waves, no atomics."""
import math

import numpy as np

from tests import mcl_ref as mr

F32 = np.float32
HYP_MAX = 64
NO_PARENT = 0xFFFFFFFF
OFF = 1 << 24
HYP_SUMS = ("sum_w", "sum_wqx", "sum_wqy", "sum_wc", "sum_ws", "sum_wdxx", "sum_wdyy", "sum_wdxy")
HYP_DOUBLES = ("share", "mean_x", "mean_y", "mean_yaw", "var_xx", "var_yy", "var_xy")
INFO_INTS = ("gen", "n_bins", "n_components", "n_hyp", "n_kld", "n_inject", "n_free", "sum_s")
INFO_DOUBLES = ("w_avg", "w_slow", "w_fast", "p_inject")


def params(bin_q=512, heading_bits=5, max_hyp=8, inject_max=0, alpha_slow=0.05, alpha_fast=0.5, kld_err=0.05, kld_z=2.326, flags=0, pad=0):
    return dict(bin_q=bin_q, heading_bits=heading_bits, max_hyp=max_hyp, inject_max=inject_max, alpha_slow=alpha_slow, alpha_fast=alpha_fast,
                kld_err=kld_err, kld_z=kld_z, flags=flags, pad=pad)


def refusal(hq, n_particles):
    """Why cm_map_mcl_hyp_configure refuses hq on a layer of n_particles, or None."""
    if not 64 <= hq["bin_q"] <= 1048576:
        return "bin_q"
    if not 0 <= hq["heading_bits"] <= 8:
        return "heading_bits"
    if not 1 <= hq["max_hyp"] <= HYP_MAX:
        return "max_hyp"
    if not 0 <= hq["inject_max"] <= n_particles - 1:
        return "inject_max"
    a, b = F32(hq["alpha_slow"]), F32(hq["alpha_fast"])
    if not (np.isfinite(a) and np.isfinite(b) and 0 <= a <= b <= 1):
        return "alpha"
    e, z = F32(hq["kld_err"]), F32(hq["kld_z"])
    if not (np.isfinite(e) and 0 < e <= 1):
        return "kld_err"
    if not (np.isfinite(z) and z > 0):
        return "kld_z"
    if hq["flags"] or hq["pad"]:
        return "flags"
    return None


def kld_bound(k, err, z):
    """H6, every operation on its own line."""
    if k <= 1:
        return 1
    err, z = float(F32(err)), float(F32(z))
    k1 = float(k - 1)
    a = 2.0 / (9.0 * k1)
    r = math.sqrt(a)
    b = (1.0 - a) + r * z
    cube = (b * b) * b
    n = math.ceil((k1 / (2.0 * err)) * cube)
    return max(1, min(n, (1 << 32) - 1))


def key_of(by, bx, bh):
    return ((by + OFF) << 34) | ((bx + OFF) << 8) | bh


def bins_of(parts, hq):
    """H1: (by, bx, bh) per particle as Python integers (// is floor division)."""
    qx, qy = mr.quant(parts["x"]).tolist(), mr.quant(parts["y"]).tolist()
    hb = hq["heading_bits"]
    bh = [(int(h) >> (32 - hb)) if hb else 0 for h in parts["h"].tolist()]
    return [(y // hq["bin_q"], x // hq["bin_q"], h) for x, y, h in zip(qx, qy, bh)]


def components(occupied, heading_bits):
    """H3: a dictionary from every occupied bin to its component's label (the smallest key of the component)."""
    parent = {b: b for b in occupied}

    def find(b):
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        return b

    H = 1 << heading_bits
    for b in occupied:
        by, bx, bh = b
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                for dh in (-1, 0, 1):
                    o = (by + dy, bx + dx, (bh + dh) % H)
                    if o in parent and o != b:
                        ra, rb = find(b), find(o)
                        if ra != rb:
                            parent[ra] = rb
    label = {}
    for b in occupied:
        r = find(b)
        label[r] = min(label.get(r, 1 << 64), key_of(*b))
    return {b: label[find(b)] for b in occupied}


def hypotheses(found, W, tab, hq, total_sum_w):
    """H1-H5 over the particles as the update found them and their weights: (the records, n_bins, n_components)."""
    W = [int(w) for w in np.asarray(W).tolist()]
    bins = bins_of(found, hq)
    label_of = components(set(bins), hq["heading_bits"])
    c, s = mr.directions(found["h"], tab)
    ci, si = np.rint(c * F32(32768.0)).astype(np.int64).tolist(), np.rint(s * F32(32768.0)).astype(np.int64).tolist()
    qx, qy = mr.quant(found["x"]).tolist(), mr.quant(found["y"]).tolist()
    members = {}
    for p, b in enumerate(bins):
        members.setdefault(label_of[b], []).append(p)
    recs = []
    for label, ps in members.items():
        r = dict(label=label, n=len(ps), sum_w=sum(W[p] for p in ps), sum_wqx=sum(W[p] * qx[p] for p in ps), sum_wqy=sum(W[p] * qy[p] for p in ps),
                 sum_wc=sum(W[p] * ci[p] for p in ps), sum_ws=sum(W[p] * si[p] for p in ps))
        r["top"] = min(ps, key=lambda p: (-W[p], p))
        sw = r["sum_w"]
        mx, my = (r["sum_wqx"] // sw, r["sum_wqy"] // sw) if sw else (0, 0)
        clamp = lambda d: max(-32768, min(32767, d))
        dx, dy = {p: clamp(qx[p] - mx) for p in ps}, {p: clamp(qy[p] - my) for p in ps}
        r["sum_wdxx"], r["sum_wdyy"], r["sum_wdxy"] = (sum(W[p] * dx[p] * dx[p] for p in ps), sum(W[p] * dy[p] * dy[p] for p in ps),
                                                      sum(W[p] * dx[p] * dy[p] for p in ps))
        assert all(abs(r[k]) < 1 << 63 for k in HYP_SUMS)
        if sw:
            f, den = float(sw), float(sw) * 1048576.0
            r.update(share=f / float(total_sum_w), mean_x=(float(r["sum_wqx"]) / f) / 1024.0, mean_y=(float(r["sum_wqy"]) / f) / 1024.0,
                     mean_yaw=math.atan2(float(r["sum_ws"]), float(r["sum_wc"])), var_xx=float(r["sum_wdxx"]) / den, var_yy=float(r["sum_wdyy"]) / den,
                     var_xy=float(r["sum_wdxy"]) / den)
        else:
            r.update({k: 0.0 for k in HYP_DOUBLES})
        recs.append(r)
    recs.sort(key=lambda r: (-r["sum_w"], r["label"]))
    return recs[:hq["max_hyp"]], len(set(bins)), len(recs)


def recovery(state, sum_s, n, n_beams, hq, n_free):
    """R1-R3: the new (w_slow, w_fast) and dict(w_avg, w_slow, w_fast, p_inject, n_inject)."""
    slow, fast = state
    if n_beams == 0:
        return (slow, fast), dict(w_avg=0.0, w_slow=slow, w_fast=fast, p_inject=0.0, n_inject=0)
    den = (float(n) * float(n_beams)) * 255.0
    w_avg = float(sum_s) / den
    a_slow, a_fast = float(F32(hq["alpha_slow"])), float(F32(hq["alpha_fast"]))
    if slow == 0.0:
        slow = w_avg
    else:
        d = w_avg - slow
        t = a_slow * d
        slow = slow + t
    if fast == 0.0:
        fast = w_avg
    else:
        d = w_avg - fast
        t = a_fast * d
        fast = fast + t
    p = 0.0
    if slow > 0.0 and fast < slow:
        ratio = fast / slow
        p = 1.0 - ratio
    n_inject = min(hq["inject_max"], int(math.floor(p * float(n))))
    if n_free == 0:
        n_inject = 0
    return (slow, fast), dict(w_avg=w_avg, w_slow=slow, w_fast=fast, p_inject=p, n_inject=n_inject)


def resample_parents(W, r_draw, m):
    """R4 for the new particles j < m: the smallest p with C_p > (j * T + r) / m."""
    W = [int(w) for w in np.asarray(W).tolist()]
    T = sum(W)
    r = (r_draw * T) >> 64
    C = np.cumsum(np.array(W, np.int64))
    t = np.array([(j * T + r) // m for j in range(m)], np.int64)
    return np.searchsorted(C, t, side="right")


def injected(q, gen, first, n, free, nx, anchor, cell):
    """Step 4 for particles first .. n - 1 over the free cells `free`, with the draws of the call gen."""
    seed, k = q["seed"], n - first
    d = [mr.draws(seed, gen, first, k, i) for i in range(4)]
    rank = np.array([(int(v) * len(free)) >> 64 for v in d[0]], np.int64)
    c = free[rank]
    ix, iy = c % nx, c // nx
    ux = (d[1] >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    uy = (d[2] >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)
    out = np.zeros(k, mr.PARTICLE)
    out["x"] = ((anchor[0] + ix).astype(F32) + ux) * F32(cell)
    out["y"] = ((anchor[1] + iy).astype(F32) + uy) * F32(cell)
    out["h"] = (d[3] >> np.uint64(32)).astype(np.uint32)
    out["parent"] = NO_PARENT
    return out


def update(parts, A, dist2, mq, anchor, q, gen, tab, hq, state, image, score=None):
    """An update with the mode on: (the particles afterwards, the weight table, the info, the hypotheses, the hyp info, the new
    averages). image: the map's current image (ny, nx). score: a replacement of step 7, (particles) -> S; None is the field."""
    n = len(parts)
    bm = mr.beams(A, mq, q)
    if score is None:
        L = mr.mf.field(dist2, mr.mf.table(mq["cell"], q["sigma"], q["max_dist"]))
        S = mr.scores(parts, bm, L, mq, anchor, tab)
    else:
        S = score(parts, bm)
    found = parts.copy()
    found["acc"] = parts["acc"] + S.astype(np.uint64)
    W = mr.weights_of(found["acc"], q["tau"])
    table = np.zeros(n, mr.WEIGHT)
    table["score"], table["weight"] = S, W
    info = mr.estimate(found, W, tab)
    b = found[info["best"]]
    info.update(n_particles=n, n_cells=bm["n_cells"], stride=bm["stride"], n_beams=bm["n_beams"], gen=gen, best_x=b["x"], best_y=b["y"], best_h=int(b["h"]))
    hyps, n_bins, n_comp = hypotheses(found, W, tab, hq, info["sum_w"])
    free = mr.free_cells(image) if hq["inject_max"] else np.zeros(0, np.int64)
    sum_s = sum(int(v) for v in S.tolist())
    assert sum_s < 1 << 38
    state, rec = recovery(state, sum_s, n, bm["n_beams"], hq, len(free))
    hinfo = dict(rec, gen=gen, n_bins=n_bins, n_components=n_comp, n_hyp=len(hyps), n_kld=kld_bound(n_bins, hq["kld_err"], hq["kld_z"]), n_free=len(free),
                 sum_s=sum_s)
    k = hinfo["n_inject"]
    do = bool(q["flags"] & mr.RESAMPLE_ALWAYS) or info["n_eff"] < float(F32(q["resample_frac"])) * float(q["n_particles"]) or k > 0
    info["resampled"] = int(do)
    out = found.copy()
    if do:
        m = n - k
        par = resample_parents(W, mr.splitmix64(mr.base_of(q["seed"], gen) ^ (1 << 63)), m)
        out["x"][:m], out["y"][:m], out["h"][:m] = found["x"][par], found["y"][par], found["h"][par]
        out["parent"][:m] = par
        out["acc"] = 0
        if k:
            out[m:] = injected(q, gen, m, n, free, image.shape[1], anchor, mq["cell"])
    else:
        out["parent"] = np.arange(n)
    return out, table, info, hyps, hinfo, state


class Filter(mr.Filter):
    """mcl_ref's Filter with the mode on: the averages restart at every init, as after the configure call."""

    def __init__(self, q, mq, tab, hq):
        super().__init__(q, mq, tab)
        assert refusal(hq, q["n_particles"]) is None
        self.hq, self.state, self.image = hq, (0.0, 0.0), None

    def init_pose(self, *v, **kw):
        super().init_pose(*v, **kw)
        self.state = (0.0, 0.0)

    def init_uniform(self, image, anchor):
        ok = super().init_uniform(image, anchor)
        if ok:
            self.state = (0.0, 0.0)
        return ok

    def update(self, A, dist2, anchor, image=None, score=None):
        """(the weight table, the info, the hypotheses, the hyp info). image: the map's current image (needed with inject_max > 0)."""
        image = self.image if image is None else image
        assert image is not None or not self.hq["inject_max"]
        self.parts, table, info, hyps, hinfo, self.state = update(self.parts, A, dist2, self.mq, anchor, self.q, self.gen, self.tab, self.hq, self.state,
                                                                  image, score)
        self.gen += 1
        return table, info, hyps, hinfo
