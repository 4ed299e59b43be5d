"""Branch-and-bound scan matching over wide windows, the search layer: cm_map_match_search_configure, cm_map_match_search,
cm_map_match_search_result, cm_map_match_search_level_copy (include/cloudmerge.h, cm_kernels_msearch.hip).

The bar: no tolerance anywhere. Where the exhaustive layer can run (wx, wy <= 64) the 96 bytes of the result equal
cm_map_match_evaluate's on the same context; everywhere they equal the restatement (tests/match_search_ref.py), whose search is
in turn compared with its own plain exhaustive steps 5 and 6, and the info (the bound, the nodes scored and kept per level, the
probe count, the overflow) equals the restatement's. The scenes are built as tests/test_map_match.py builds its own (its
helpers are imported): one point of A per wanted window cell, both sensors outside the window. Every designed scene is first
run on the CPU alone, where its guards are asserted."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi
from tests import cost_ref as cr
from tests import match_ref as mf
from tests import match_search_ref as ms
from tests import map_ref as mr
from tests import test_grid_map as tg
from tests import test_map_cost as tc
from tests import test_map_match as tmm
from tests import test_occupancy_map as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
NAMES = ("cm_map_match_search_configure", "cm_map_match_search", "cm_map_match_search_result", "cm_map_match_search_level_copy")
SEARCH_TYPES = (capi.MatchSearchParams, capi.MatchSearchInfo)      # (a library without the layer fails every test here, at import)
F32 = np.float32
CELL, NX, NY = tmm.CELL, tmm.NX, tmm.NY
SHARP = tmm.SHARP


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_search_structs_and_constants_match_header(tmp_path):
    structs = {"cm_match_search_params": (capi.MatchSearchParams, ["sigma", "max_dist", "n_a", "a_stride", "wx", "wy", "depth", "max_nodes", "max_cells", "flags"]),
               "cm_match_search_info": (capi.MatchSearchInfo, ["depth", "n_roots", "bound", "scored", "live", "n_probe", "overflow_level"])}
    names = ["CM_MATCH_SEARCH_MAX_SHIFT", "CM_MATCH_SEARCH_MAX_DEPTH", "CM_MATCH_SEARCH_MAX_NODES", "-CM_MATCH_SEARCH_OVERFLOW_CELLS"]
    items, want = [], []
    for s, (T, fields) in structs.items():
        items += [f"sizeof({s})"] + [f"offsetof({s},{f})" for f in fields]
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%llu ",(unsigned long long)({it}));' for it in items + names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(want)] == want == [40, 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 84, 0, 4, 8, 12, 44, 76, 80]
    assert got[len(want):] == [capi.MATCH_SEARCH_MAX_SHIFT, capi.MATCH_SEARCH_MAX_DEPTH, capi.MATCH_SEARCH_MAX_NODES, -capi.MATCH_SEARCH_OVERFLOW_CELLS]
    assert got[len(want):] == [ms.MAX_SHIFT, ms.MAX_DEPTH, ms.MAX_NODES, -ms.OVERFLOW_CELLS] == [1024, 7, 1 << 22, 2]
    assert 255 * (2 * ms.MAX_SHIFT + 1) ** 2 < 1 << 32                 # the entry index fits uint32_t at the caps
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.MatchSearchParams(0.1, 0.3, 1, 1, 1, 1, 1, 64, 64, 0)
    pose = np.eye(3, 4, dtype=F32)
    res, info = capi.MatchResult(), capi.MatchSearchInfo()
    before = bytes(res), bytes(info)
    buf = np.full(27, 7, np.uint8)
    dims = (C.c_uint32 * 2)(5, 6)
    assert L.cm_map_match_search_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_match_search_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_match_search(None, pose.ctypes.data, C.byref(res), C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_match_search_result(None, C.byref(res), C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_match_search_level_copy(None, 0, buf.ctypes.data, 27, C.byref(dims)) == capi.BAD_ARG
    assert (buf == 7).all() and (bytes(res), bytes(info)) == before and tuple(dims) == (5, 6)


REFUSED_PARAMS = [dict(sigma=0.0), dict(sigma=np.nan), dict(max_dist=-1.0), dict(max_dist=np.inf), dict(max_dist=6.5), dict(n_a=128), dict(a_stride=0),
                  dict(n_a=127, a_stride=9), dict(wx=1025), dict(wy=1025), dict(depth=8), dict(max_nodes=0), dict(max_nodes=(1 << 22) + 1), dict(max_cells=0),
                  dict(max_cells=(1 << 22) + 1), dict(wx=40, wy=33, depth=3, max_nodes=98), dict(wx=3, wy=2, depth=0, max_nodes=34), dict(flags=2),
                  dict(flags=1 << 31)]
ACCEPTED_PARAMS = [dict(max_dist=6.4), dict(n_a=127, a_stride=8), dict(wx=1024, wy=0, depth=7), dict(wx=0, wy=1024, depth=7), dict(wx=0, wy=0, depth=7),
                   dict(wx=40, wy=33, depth=3, max_nodes=99), dict(wx=3, wy=2, depth=0, max_nodes=35), dict(max_nodes=1 << 22), dict(max_cells=1), dict(flags=1)]


def test_refusals_of_the_restatement():
    ok = ms.params()
    assert ms.refusal(ok, CELL) is None
    for kw in REFUSED_PARAMS:
        assert ms.refusal(dict(ok, **kw), CELL) is not None, kw
    for kw in ACCEPTED_PARAMS:
        assert ms.refusal(dict(ok, **kw), CELL) is None, kw
    assert ms.refusal(ok, CELL, 65536, 1) is not None and ms.refusal(ok, CELL, 65535, 64) is None
    assert ms.roots_along(40, 3) == 11 and ms.roots_along(33, 3) == 9 and ms.roots_along(0, 7) == 1 and ms.roots_along(1024, 7) == 17


def test_the_pyramid_by_hand():
    L = np.zeros((3, 4), np.uint8)
    L[0, 0], L[2, 3], L[1, 2] = 9, 7, 200
    l1 = ms.level(L, 1)
    assert l1.shape == (4, 5) and l1[0, 0] == 9 and l1[0, 1] == 9 and l1[1, 1] == 9           # L_1(-1, -1) = L(0, 0): the ring on the negative side
    assert l1[3, 4] == 7 and l1[3, 3] == 7 and l1[2, 3] == 200 and l1[2, 4] == 7 and l1[0, 4] == 0     # L_1(3, 2) = L(3, 2); L_1(3, -1) = 0
    l2 = ms.level(L, 2)
    assert l2.shape == (6, 7) and l2[0, 0] == 9 and l2[5, 6] == 7 and l2[0, 6] == 0 and l2[3, 3] == 200
    assert (ms.level(L, 0) == L).all()


def test_the_search_equals_the_plain_steps_on_random_small_cases():
    """Windows of 3 to 14 cells, depth 0 to 4, empty maps and empty frames included: the best entry of the level loop is that of
    the exhaustive steps 5 and 6, the bound is an entry's score, the counts add up."""
    rng = np.random.default_rng(28)
    pruned = 0
    for case in range(60):
        nx, ny = int(rng.integers(3, 15)), int(rng.integers(3, 15))
        q = ms.params(n_a=int(rng.integers(0, 2)), wx=int(rng.integers(0, 15)), wy=int(rng.integers(0, 15)), depth=int(rng.integers(0, 5)))
        L = np.zeros((ny, nx), np.uint8)
        n_hit = 0 if case % 10 == 0 else int(rng.integers(1, nx * ny // 2 + 1))
        hits = rng.choice(nx * ny, n_hit, replace=False)
        L.reshape(-1)[hits] = rng.choice([255, 255, 154, 93, 12], n_hit)
        D = [np.sort(rng.choice(nx * ny, int(rng.integers(0 if case % 7 == 0 else 1, nx * ny // 3 + 2)), replace=False)) for _ in range(2 * q["n_a"] + 1)]
        status, best, info, scores = ms.search(D, L, q)
        want, s_max = ms.exhaustive(D, L, q)
        assert status == "ok" and best == want, (case, best, want)
        assert scores[best] == s_max and info["bound"] <= s_max and info["live"][0] >= 1 and info["scored"][q["depth"]] == info["n_roots"]
        assert all(info["live"][h] <= info["scored"][h] for h in range(8)) and info["overflow_level"] == -1
        assert all(s == ms.leaf(D, L, kk, ii - q["wx"], jj - q["wy"]) for (kk, jj, ii), s in scores.items())
        pruned += info["live"][0] < (2 * q["n_a"] + 1) * (2 * q["wx"] + 1) * (2 * q["wy"] + 1)
    assert pruned > 30                                                     # (the bound does something in most of them)


# ---- the designed scenes ---------------------------------------------------------------------------------------------------
WIDE = dict(n_a=0, wx=40, wy=33, depth=3, max_nodes=1 << 14, max_cells=4096)     # 81 x 67 shifts: partial root blocks (81 = 10 * 8 + 1, 67 = 8 * 8 + 3)
ELL = [(x, 0) for x in range(7)] + [(0, y) for y in range(1, 5)]           # an L: no shift but (0, 0) maps it onto itself


def ell(x0, y0):
    return [(x0 + x, y0 + y) for x, y in ELL]


def tie_guard(*entries):
    """The entries (k, i, j) tie at the largest score of the whole volume."""
    def check(res, D, L, sc):
        n_a = sc["q"]["n_a"]
        got = [ms.leaf(D, L, k + n_a, i, j) for k, i, j in entries]
        assert len(set(got)) == 1 and got[0] == res["score"] == ms.exhaustive(D, L, sc["q"])[1] and len(entries) >= 2, got
    return check


def live_is_scored(res, D, L, sc):
    pass                                                                   # (asserted on the info: see check_scene)


def designed():
    S = tmm.scene
    out = []
    out.append(S("partial root blocks", [ell(50, 40), []], scan_cells=[ell(37, 51), []], q=dict(WIDE), expect=dict(k=0, i=13, j=-11, score=255 * 11)))
    out.append(S("the peak at (wx, wy)", [ell(50, 40), []], scan_cells=[ell(10, 7), []], q=dict(WIDE), expect=dict(k=0, i=40, j=33, score=255 * 11, best=81 * 67 - 1)))
    out.append(S("the peak at (-wx, -wy)", [ell(20, 10), []], scan_cells=[ell(60, 43), []], q=dict(WIDE), expect=dict(k=0, i=-40, j=-33, score=255 * 11, best=0)))
    out.append(S("the ring", tmm.EDGE_CELLS, q=dict(WIDE), expect=dict(k=0, i=0, j=0, n_cells=12, score=255 * 12)))
    out.append(S("the ring, turned: cells leave on all four sides", tmm.EDGE_CELLS, q=dict(WIDE, n_a=2, a_stride=16, max_nodes=1 << 15), prior=(0.3, -0.2), expect=dict(k=0, i=-3, j=2)))
    # two equal structures: the scan's L lies 10 right and 5 up of one and 3 left and 2 down of the other
    out.append(S("two structures tie at different i * i + j * j", [ell(50, 40), ell(37, 33)], scan_cells=[ell(40, 35), []], q=dict(WIDE, **SHARP),
                 expect=dict(k=0, i=-3, j=-2, score=255 * 11), check=tie_guard((0, 10, 5), (0, -3, -2))))
    # the point 4.0748 m ahead moves one row per candidate (tests/test_map_match.py's scene): k = -1 and k = +1 hit at shift (0, 0)
    out.append(S("a +-k tie", [[(88, 39)], [(88, 41)]], scan_cells=[[], []], scan_extra=([(4.0748, 0.05, 0.0)], []), q=dict(WIDE, n_a=2, a_stride=16, **SHARP),
                 expect=dict(k=-1, i=0, j=0, score=255, n_cells=1), check=tie_guard((-1, 0, 0), (1, 0, 0))))
    # i = -5 lies in the root block of i0 = -8, i = +5 in that of i0 = 0: the same score, i * i + j * j and k, the lower index wins
    out.append(S("a tie across two root blocks", [ell(45, 40), ell(55, 40)], scan_cells=[ell(50, 40), []], q=dict(WIDE, **SHARP),
                 expect=dict(k=0, i=-5, j=0, score=255 * 11), check=tie_guard((0, -5, 0), (0, 5, 0))))
    out.append(S("depth 0", [ell(50, 40), []], scan_cells=[ell(46, 43), []], q=dict(WIDE, wx=6, wy=5, depth=0), expect=dict(k=0, i=4, j=-3, score=255 * 11)))
    out.append(S("depth 7 on a window narrower than 128", [ell(50, 40), []], scan_cells=[ell(37, 51), []], q=dict(WIDE, depth=7, n_a=1), expect=dict(k=0, i=13, j=-11, score=255 * 11)))
    out.append(S("200 x 160, displaced by (+97, -71)", [ell(130, 30), []], scan_cells=[ell(33, 101), []], nx=200, ny=160, q=dict(WIDE, wx=150, wy=120, depth=5, max_nodes=1 << 16),
                 expect=dict(k=0, i=97, j=-71, score=255 * 11, n_cells=11)))
    out.append(S("an empty map with room", [[], []], scan_cells=tmm.BASE, q=dict(WIDE), expect=dict(k=0, i=0, j=0, score=0, n_cells=tmm.N_BASE), check=live_is_scored))
    out.append(S("an empty map, max_nodes too small", [[], []], scan_cells=tmm.BASE, q=dict(WIDE, max_nodes=200), expect=dict(capacity=2)))
    out.append(S("max_cells one below the cells", [ell(50, 40), []], scan_cells=tmm.BASE, q=dict(WIDE, max_cells=tmm.N_BASE - 1), expect=dict(capacity=ms.OVERFLOW_CELLS)))
    out.append(S("max_cells exactly the cells", [ell(50, 40), []], scan_cells=tmm.BASE, q=dict(WIDE, max_cells=tmm.N_BASE), expect=dict(n_cells=tmm.N_BASE)))
    # tests/test_map_match.py's sub-cell scenes: the best entry inside the range, and on its edge (no neighbour beyond it)
    out.append(S("sub-cell inside", [[(40, 40), (50, 40)], [(41, 40)]], scan_cells=[[(40, 40)], [(50, 40)]], q=dict(WIDE, flags=1),
                 expect=dict(k=0, i=0, j=0, score=510, n_cells=2, sub=(0.5 * (308.0 - 409.0) / (308.0 - 1020.0 + 409.0), 0.0))))
    out.append(S("sub-cell on the range's edge", [[(43, 40)], []], scan_cells=[[(40, 40)], []], q=dict(WIDE, wx=3, wy=2, depth=1, flags=1), expect=dict(k=0, i=3, j=0, score=255, sub=(0.0, 0.0))))
    return out


DESIGNED = designed()


def search_q(sc):
    """The search layer's parameters of a scene; a scene of tests/test_map_match.py gets depth 2 and room."""
    return dict(dict(depth=2, max_nodes=1 << 16, max_cells=4096), **sc["q"])


def check_scene(sc, status, res, info, LQD):
    """The scene's expectations and guards on the restatement's answer, and the search against the plain steps 5 and 6."""
    q = search_q(sc)
    L, Q, D = LQD
    assert info["depth"] == q["depth"] and info["n_roots"] == ms.n_roots(q) <= q["max_nodes"]
    if "capacity" in sc["expect"]:
        assert status == "capacity" and res is None and info["overflow_level"] == sc["expect"]["capacity"], info
        return
    assert status == "ok" and info["overflow_level"] == -1
    for f, v in sc["expect"].items():
        assert res[f] == v, (sc["name"], f, res[f], v)
    kk, jj, ii = res["k"] + q["n_a"], res["j"] + q["wy"], res["i"] + q["wx"]
    assert ms.exhaustive(D, L, q) == ((kk, jj, ii), res["score"]), sc["name"]
    assert info["bound"] <= res["score"] and info["live"][0] >= 1 and info["scored"][q["depth"]] == info["n_roots"]
    if sc["check"] is live_is_scored:
        assert info["live"] == info["scored"] and info["bound"] == 0 and info["live"][0] == (2 * q["wx"] + 1) * (2 * q["wy"] + 1)
    elif sc["check"] in (tmm.hits_back, tmm.one_k_only, tmm.shifts_leave):
        pass                                                               # (guards on the volume: tests/test_map_match.py asserts them)
    elif sc["check"]:
        sc["check"](res, D, L, sc)


@pytest.mark.parametrize("sc", DESIGNED + tmm.SCENES, ids=lambda s: s["name"])
def test_every_scene_on_the_restatements_alone(sc):
    """No GPU: cost_ref's distance field of the wanted image and the points of the frame, through the level loop and through the
    plain steps 5 and 6."""
    dist2 = cr.dist2_separable(tmm.image_of(sc["map_cells"], sc["nx"], sc["ny"]))
    _, A = tmm.scan_of(sc)
    q = search_q(sc)
    status, res, info, LQD = ms.match(A, dist2, sc["mq"], tmm.anchor_of(sc["nx"], sc["ny"]), q, tmm.prior_of(sc, tmm.TAB()), tmm.TAB())
    check_scene(sc, status, res, info, LQD)
    if sc in DESIGNED and status == "ok" and sc["name"] == "partial root blocks":
        print(f"{sc['name']}: scored {info['scored']}, live {info['live']}, probe {info['n_probe']}, B {info['bound']} of {res['score']}")
        assert sum(info["scored"]) < 81 * 67 // 4                          # the bound prunes: far fewer nodes than entries


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def info_dict(i):
    return dict(depth=i.depth, n_roots=i.n_roots, bound=i.bound, scored=list(i.scored), live=list(i.live), n_probe=i.n_probe, overflow_level=i.overflow_level)


def configure_search(cm, q):
    cm.map_match_search_configure(q["sigma"], q["max_dist"], q["n_a"], q["a_stride"], q["wx"], q["wy"], q["depth"], q["max_nodes"], q["max_cells"],
                                  bool(q["flags"] & 1))


def evaluate(cm, sc, n_cap=4096):
    """Configure the layer, search, compare result and info with the restatement of the library's own tables and, where the
    exhaustive layer can run, the result's bytes with cm_map_match_evaluate's on the same context."""
    if sc["scan_cells"] is not None:
        tg.run_frame(cm, tmm.scan_of(sc)[0], tc.PARAMS)
    A = tg.host_clouds(cm, n_cap, False)[0]
    _, dist2, minfo = cm.map_cost()
    prior = tmm.prior_of(sc, tmm.TAB())
    q = search_q(sc)
    status, want, winfo, LQD = ms.match(A, dist2, sc["mq"], tuple(minfo.anchor), q, prior, tmm.TAB())
    check_scene(sc, status, want, winfo, LQD)
    configure_search(cm, q)
    if status == "capacity":
        with pytest.raises(capi.CloudMergeError) as e:
            cm.map_match_search(prior)
        assert e.value.status == capi.CAPACITY and info_dict(e.value.info) == winfo, (info_dict(e.value.info), winfo)
        tm.refused(cm, cm.map_match_search_result, text=b"stale")          # the result stays stale
        tm.refused(cm, cm.map_match_search_level, 0, text=b"stale")
        return
    res, info = cm.map_match_search(prior)
    got = tmm.result_dict(res)
    print(f"{sc['name']}: (k, i, j) = ({got['k']}, {got['i']}, {got['j']}) score {got['score']} B {info.bound} scored {list(info.scored)} live {list(info.live)} probe {info.n_probe}")
    assert info_dict(info) == winfo, (sc["name"], info_dict(info), winfo)
    assert tmm.same_result(got, want), (sc["name"], got, want)
    again, info2 = cm.map_match_search(prior)                              # two evaluates: identical result and info
    kept, info3 = cm.map_match_search_result()
    assert bytes(again) == bytes(res) == bytes(kept) and bytes(info2) == bytes(info) == bytes(info3)
    if q["wx"] <= 64 and q["wy"] <= 64:                                    # both layers on one context
        tmm.configure_match(cm, sc["q"])
        ex = cm.map_match(prior)
        assert bytes(ex) == bytes(res), (sc["name"], tmm.result_dict(ex), got)
        assert bytes(cm.map_match_search_result()[0]) == bytes(res)        # the exhaustive layer's evaluate left this one alone
    return res, info, LQD


def groups(scenes):
    out = {}
    for sc in scenes:
        key = (sc["nx"], sc["ny"], repr(sc["map_cells"]), repr(sc["map_extra"]), repr(sorted(sc["mq"].items())))
        out.setdefault(key, []).append(sc)
    return list(out.values())


@pytest.mark.gpu
@pytest.mark.parametrize("group", groups(tmm.SCENES), ids=lambda g: g[0]["name"])
def test_every_exhaustive_scene_through_both_layers(group):
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm:
        tmm.build_map(cm, group[0])
        for sc in group:
            evaluate(cm, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("group", groups(DESIGNED), ids=lambda g: g[0]["name"])
def test_every_designed_scene(group):
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm:
        tmm.build_map(cm, group[0])
        for sc in group:
            evaluate(cm, sc)


@pytest.mark.gpu
def test_every_level_of_the_pyramid():
    sc = DESIGNED[4]                                                       # the ring, with n_a = 2
    assert sc["name"].startswith("the ring, turned")
    q = dict(search_q(sc), depth=7)
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm:
        tmm.build_map(cm, sc)
        configure_search(cm, q)
        tm.refused(cm, cm.map_match_search_level, 0, text=b"cm_map_match_search_configure")      # stale until the evaluate
        cm.map_match_search(tmm.prior_of(sc, tmm.TAB()))
        L = mf.field(cm.map_cost()[1], mf.table(CELL, q["sigma"], q["max_dist"]))
        assert L[0, 0] == 255 and L[NY - 1, NX - 1] == 255 and L[0, NX - 1] == 255 and L[NY - 1, 0] == 255     # the ring is there
        for h in range(8):
            got, want = cm.map_match_search_level(h), ms.level(L, h)
            assert got.shape == want.shape == (NY + (1 << h) - 1, NX + (1 << h) - 1) and got.dtype == np.uint8
            assert got.tobytes() == want.tobytes(), (h, np.argwhere(got != want)[:4])
        lib = cm._lib
        buf = np.full(NX * NY + 1, 7, np.uint8)
        dims = (C.c_uint32 * 2)()
        assert lib.cm_map_match_search_level_copy(cm._ctx, 0, buf.ctypes.data, NX * NY - 1, C.byref(dims)) == capi.CAPACITY and (buf == 7).all()
        assert tuple(dims) == (NX, NY)
        assert lib.cm_map_match_search_level_copy(cm._ctx, 0, buf.ctypes.data, NX * NY + 1, None) == capi.OK and buf[:-1].tobytes() == L.tobytes() and buf[-1] == 7
        assert lib.cm_map_match_search_level_copy(cm._ctx, 0, None, NX * NY, None) == capi.BAD_ARG
        assert lib.cm_map_match_search_level_copy(cm._ctx, 8, buf.ctypes.data, NX * NY, None) == capi.BAD_ARG
        configure_search(cm, dict(q, depth=2))
        cm.map_match_search(tmm.prior_of(sc, tmm.TAB()))
        tm.refused(cm, cm.map_match_search_level, 3, text=b"depth")        # above the configured depth


@pytest.mark.gpu
def test_with_ground_removal():
    """tests/test_map_match.py's ground scene: the plane's points are in G, not in A, and must not be counted."""
    from cloud_merger_amd.types import MergeParams
    parts = tg.ground_scene(31)
    n_cap = sum(len(p) for p in parts)
    q = ms.params(sigma=0.5, max_dist=1.5, n_a=2, a_stride=4, wx=9, wy=5, depth=2, max_cells=8192, flags=1)
    mq = mr.params(0.5, 320, 24)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=2, flags=capi.FLAG_OCCUPANCY) as cm:
        cm.set_ground_removal(capi.make_ground_params([tg.FRONT, tg.FRONT]))
        tm.configure(cm, mq)
        tg.run_frame(cm, tg.clouds_of(parts), MergeParams(leaf=(0.1,) * 3, min_points_per_voxel=1, **tg.ROI))
        A, G = tg.host_clouds(cm, n_cap, True)
        assert len(G) > n_cap // 2 and len(A) > 500
        minfo = cm.map_integrate(None)
        cm.map_cost_configure(0.0, 1.0, 3.0, False)
        cm.map_cost_update()
        configure_search(cm, q)
        prior = tm.pose_t(1.0, -0.5)                                       # two cells right, one down
        status, want, winfo, (L, Q, D) = ms.match(A, cm.map_cost()[1], mq, tuple(minfo.anchor), q, prior, tmm.TAB())
        _, with_g, _, _ = ms.match(np.concatenate([A, G]), cm.map_cost()[1], mq, tuple(minfo.anchor), q, prior, tmm.TAB())
        assert status == "ok" and with_g["n_cells"] != want["n_cells"]     # counting G would show
        res, info = cm.map_match_search(prior)
        assert tmm.same_result(tmm.result_dict(res), want) and info_dict(info) == winfo
        assert (res.k, res.i, res.j) == (0, -2, 1) and res.score == res.max_score


@pytest.mark.gpu
def test_with_deskew():
    """tests/test_map_match.py's moving vehicle through the wide search: k_match_mark reads the compensated records in place.
    Result, info and every level of the pyramid are the restatement's on the library's merged(), and the bytes of a context
    without motion fed the numpy-compensated clouds."""
    sc = tmm.scene("deskew", tmm.BASE, q=dict(n_a=2, a_stride=16, wx=20, wy=13, depth=3, max_nodes=1 << 16, max_cells=4096, flags=1))
    raws, stamps = tmm.deskew_raws(tmm.parts_of(sc["map_cells"], sc["nx"], sc["ny"]))
    with capi.CloudMerger(max_points_total=4096, max_sensors=2) as cm, capi.CloudMerger(max_points_total=4096, max_sensors=2) as plain:
        tmm.build_map(cm, sc)
        tmm.build_map(plain, sc)
        A, comp = tmm.run_deskewed(cm, raws, stamps)
        lo, hi = tmm.moved_by_cells(A, tmm.scan_of(sc)[1])
        assert lo > 3.0 and hi < 12.0, (lo, hi)
        res, info, (L, Q, D) = evaluate(cm, sc)
        tg.run_frame(plain, comp, tc.PARAMS)
        assert tg.host_clouds(plain, 4096, False)[0].tobytes() == A.tobytes()
        p_res, p_info, _ = evaluate(plain, sc)
        assert bytes(res) == bytes(p_res) and bytes(info) == bytes(p_info)
        for h in range(search_q(sc)["depth"] + 1):
            got = cm.map_match_search_level(h)
            assert got.tobytes() == ms.level(L, h).tobytes() == plain.map_match_search_level(h).tobytes(), h
        _, unmoved, _, _ = ms.match(tmm.scan_of(sc)[1], cm.map_cost()[1], sc["mq"], tmm.anchor_of(sc["nx"], sc["ny"]), search_q(sc), tmm.prior_of(sc, tmm.TAB()),
                                    tmm.TAB())
        assert not tmm.same_result(tmm.result_dict(res), unmoved)      # searching with the raw clouds would show


def small_stack(cm, nx=64, ny=48, cell=0.1, search=True):
    tm.configure(cm, tc.map_q(cell, nx, ny))
    cm.map_cost_configure(0.35, 1.05, 3.0, True)
    if search:
        cm.map_match_search_configure(0.1, 0.3, 1, 8, 20, 12, 2, 4096, 256)


@pytest.mark.gpu
def test_staleness_and_lifetime():
    nx, ny, cell = 64, 48, 0.1
    I = np.eye(3, 4, dtype=F32)
    frame = lambda cm: tg.run_frame(cm, tc.frame_of(tc.CORNERS_64_48, cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
    reads = lambda cm: (cm.map_match_search_result, lambda: cm.map_match_search_level(0))
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.refused(cm, cm.map_match_search_configure, 0.1, 0.3, text=b"cm_map_configure")
        tm.configure(cm, tc.map_q(cell, nx, ny))
        tm.refused(cm, cm.map_match_search_configure, 0.1, 0.3, text=b"cm_map_cost_configure")      # no cost layer
        cm.map_cost_configure(0.35, 1.05, 3.0, True)
        for call in reads(cm) + (lambda: cm.map_match_search(I),):
            tm.refused(cm, call, text=b"cm_map_match_search_configure")                              # no search layer
        small_stack(cm)
        for call in reads(cm):                                                                       # a read before the first evaluate
            tm.refused(cm, call, text=b"stale")
            tm.refused(cm, call, text=b"cm_map_match_search_configure")
        tm.refused(cm, cm.map_match_search, I, text=b"no result")                                    # no frame yet
        frame(cm)
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_integrate")                             # n_frames == 0
        cm.map_integrate(None)
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_cost_update")                           # dist2 is stale
        cm.map_cost_update()
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_cost_update")
        res, info = cm.map_match_search(tm.pose_t(0.2, -0.1))                                        # an integrated frame may be matched
        assert (res.k, res.i, res.j, res.score) == (0, -2, 1, 255 * 5) and info.overflow_level == -1
        frame(cm)                                                                                    # a merge
        for call in reads(cm):
            tm.refused(cm, call, text=b"merge")
        again, info2 = cm.map_match_search(tm.pose_t(0.2, -0.1))                                     # a frame that is not integrated
        assert bytes(again) == bytes(res) and bytes(info2) == bytes(info)
        cm.map_integrate(None)
        for call in reads(cm):
            tm.refused(cm, call, text=b"cm_map_integrate")
        tm.refused(cm, cm.map_match_search, I, text=b"stale")
        cm.map_cost_update()
        cm.map_match_search(I)
        cm.map_match_search_configure(0.1, 0.3, 1, 8, 20, 12, 2, 4096, 256)                          # configure again: stale again
        tm.refused(cm, cm.map_match_search_result, text=b"cm_map_match_search_configure")
        cm.map_match_search(I)
        cm.map_match_search_configure(None)                                                          # NULL frees
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_match_search_configure")
        small_stack(cm)
        cm.map_cost_configure(0.35, 1.05, 3.0, True)                                                 # the cost layer takes it along
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_match_search_configure")
        small_stack(cm)
        cm.map_cost_configure(None)
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_cost_configure")
        small_stack(cm)
        tm.configure(cm, tc.map_q(cell, nx, ny))                                                     # and so does the map
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_cost_configure")
        small_stack(cm)
        cm.map_configure(None)
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_configure")
        cm.map_match_search_configure(None)                                                          # freeing what is not there is fine


@pytest.mark.gpu
def test_refusals_and_a_frame_in_flight():
    nx, ny, cell = 64, 48, 0.1
    I = np.eye(3, 4, dtype=F32)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        lib = cm._lib
        small_stack(cm, search=False)
        ok = ms.params()
        for kw in REFUSED_PARAMS:                      # every refusal of the restatement's validator is the library's
            q = dict(ok, **kw)
            p = capi.MatchSearchParams(q["sigma"], q["max_dist"], q["n_a"], q["a_stride"], q["wx"], q["wy"], q["depth"], q["max_nodes"], q["max_cells"], q["flags"])
            assert lib.cm_map_match_search_configure(cm._ctx, C.byref(p)) == capi.BAD_ARG and lib.cm_last_error(cm._ctx), kw
        tm.refused(cm, cm.map_match_search, I, text=b"cm_map_match_search_configure")                # a refused call configured nothing
        for kw in ACCEPTED_PARAMS:
            configure_search(cm, dict(ok, **kw))
        small_stack(cm)
        tg.run_frame(cm, tc.frame_of([(3, 2), (40, 30)], cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
        cm.map_integrate(None)
        cm.map_cost_update()
        res, info = cm.map_match_search(I)
        assert res.score == 510 and lib.cm_map_match_search(cm._ctx, None, None, None) == capi.BAD_ARG
        assert lib.cm_map_match_search(cm._ctx, I.ctypes.data, None, None) == capi.OK                # both outputs may be NULL
        for bad in (np.nan, np.inf):
            for at in (0, 3, 7, 11):
                P = I.copy()
                P.reshape(-1)[at] = bad
                tm.refused(cm, cm.map_match_search, P, text=b"finite")
        far = I.copy()
        far[0, 3] = 3e38
        tm.refused(cm, cm.map_match_search, far, text=b"vehicle")
        kept, kinfo = cm.map_match_search_result()                                                   # a refused evaluate leaves the result
        assert bytes(kept) == bytes(res) and bytes(kinfo) == bytes(info)
        moved, _ = cm.map_match_search(tm.pose_t(1.1, 0.0))
        assert (moved.i, moved.j, moved.score) == (-11, 0, 510)
        cm.submit_all(tc.frame_of([(3, 2), (40, 30)], cell, nx, ny, tc.OUTSIDE))                     # a frame in flight
        cm.merge_voxelize_async(capi.make_params(tc.PARAMS))
        for c in (lambda: cm.map_match_search_configure(0.1, 0.3), cm.map_match_search_result, lambda: cm.map_match_search_level(0), lambda: cm.map_match_search(I)):
            tm.refused(cm, c, text=b"flight")
        assert cm.wait().status == capi.OK
        tm.refused(cm, cm.map_match_search_result, text=b"merge")


@pytest.mark.gpu
def test_an_evaluate_changes_no_other_layer():
    nx, ny, cell = 64, 48, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        small_stack(cm, nx, ny)
        cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
        cm.map_plan_configure(50, 205, True)
        cm.map_traj_configure(3, 3, 4, [(0.1, 0.0)], 1, 1, True)
        tg.run_frame(cm, tc.frame_of(tc.CORNERS_64_48, cell, nx, ny, tc.OUTSIDE), tc.PARAMS)
        cm.map_integrate(None)
        cm.map_cost_update()
        cm.map_plan_update(2.05, 1.05)
        cm.map_traj_evaluate(0.05, 0.05, 0.0, (0.0, 1.0), (-1.0, 1.0), 0.1)
        cm.map_match(tm.pose_t(0.2, -0.1))

        def state():
            table, info = cm.map()
            cost, dist2, _ = cm.map_cost()
            vol, mres = cm.map_match_scores()
            return (table.tobytes(), cm.map_occupancy()[0].tobytes(), tm.info_tuple(info), cost.tobytes(), dist2.tobytes(), cm.map_cost_table().tobytes(),
                    cm.map_plan()[0].tobytes(), cm.map_traj()[0].tobytes(), bytes(cm.map_traj()[1]), cm.merged(4096).tobytes(), vol.tobytes(), bytes(mres),
                    cm.map_match_table().tobytes())

        before = state()
        res, info = cm.map_match_search(tm.pose_t(0.2, -0.1))
        names = [n for n, _ in cm.stage_times()]
        assert names == ["msearch_clear", "k_match_field", "k_msearch_pyramid", "k_match_mark", "k_msearch_list", "k_msearch_score", "k_msearch_pick",
                         "k_msearch_select", "k_msearch_best"], names
        assert all(ms_ >= 0.0 for _, ms_ in cm.stage_times()) and (res.i, res.j, res.score) == (-2, 1, 255 * 5)
        assert state() == before                       # nothing went stale either: every read above still answers
        tg.run_frame(cm, tc.frame_of([(3, 2)], cell, nx, ny, tc.OUTSIDE), tc.PARAMS)      # a frame's own list never holds the call's stages
        assert not any("msearch" in n for n, _ in cm.stage_times())
