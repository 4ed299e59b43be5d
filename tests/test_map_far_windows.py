"""Every map layer on windows far from the world origin (include/cloudmerge.h: world_axis, the anchor strictly inside
+-2^30; tests/far_windows.py holds the placements, the scenes and their guards).

The placements, each the absolute cell of window cell (0, 0):

  origin     anchor_of(nx, ny): the control, what every other test of the map layers uses.
  km         (+120 000, -70 000) minus half the window: +12 km and -7 km, signs mixed, the window wholly off both axes; fp32
             still resolves a millimetre. A vehicle that has driven a while: the ordinary case of a rolling map.
  two24      (2^24 - nx/2, -2^24 - ny/2): the window straddles absolute cell +-2^24 on both axes, so (float)(ax + ix) of
             init_uniform rounds for odd cells; at 0.1 m cells that is 1.68e6 m, beyond the hypotheses mode's clamp at
             2^20 m; fp32 resolves 1.25 cells.
  limit_pos  (2^30 - nx/2, 2^30 - 1 - ny) on 2048 x 64: the largest anchor cm_map_load accepts on y, and on x a window whose
             right half has no existing absolute cell. fp32 names one row and thirteen columns of it.
  limit_neg  an anchor below -2^30. cm_map_load refuses it, so it is absent from every test of a loaded map by construction;
             cm_map_integrate reaches it (anchor = vehicle cell - n/2) with 0.5 m cells, 512 x 512 and x = -536 870 848, and
             the integration test is the one that runs there.

Part A is lockstep with the restatements, byte for byte, at every placement the load accepts (the integration at km, two24
and limit_neg). Part B compares the library with itself under a shift that is exact in fp32: no restatement is involved, so
a mistake that header, kernel and restatement shared would still show. The guards run on the restatements alone, unmarked."""
import math

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import xyzi_cloud
from tests import cast_ref as kr
from tests import far_windows as fw
from tests import front_ref as fr
from tests import match_ref as mf
from tests import match_search_ref as ms
from tests import mcl_beam_ref as br
from tests import mcl_hyp_ref as hr
from tests import mcl_ref as mr
from tests import plan_ref as pr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_map_cast as tcs
from tests import test_map_cost as tc
from tests import test_map_frontier as tf
from tests import test_map_match as tmm
from tests import test_map_match_search as tms
from tests import test_map_mcl as tml
from tests import test_map_mcl_beam as tmb
from tests import test_map_mcl_hyp as tmh
from tests import test_map_plan as tp
from tests import test_map_traj as ttj
from tests import test_occupancy_map as tm
from tests import traj_ref as jr

F32 = np.float32
PLACES = pytest.mark.parametrize("place", fw.LOADED, ids=repr)
BEAM = br.params()


# ---- CPU: the placements and the guards on the restatements alone --------------------------------------------------------------
def test_the_placements_are_what_the_docstring_says():
    assert fw.ORIGIN.anchor == (-48, -40) and fw.KM.anchor == (119952, -70040)
    assert fw.TWO24.anchor == (16777168, -16777256) and fw.LIMIT_POS.anchor == ((1 << 30) - 1024, (1 << 30) - 65)
    assert all(abs(a) < 1 << 30 for p in fw.LOADED for a in p.anchor)                  # what cm_map_load accepts
    # km: a coordinate at a cell's centre lands in that cell; two24: not always; limit_pos: one row, thirteen columns
    every = [(x, y) for x in range(0, 96, 5) for y in range(0, 80, 7)]
    assert all(fw.KM.landing(*c) == c for c in every) and all(fw.ORIGIN.landing(*c) == c for c in every)
    moved = [c for c in every if fw.TWO24.landing(*c) != c]
    assert 0 < len(moved) < len(every) and all(fw.TWO24.landing(*c) is not None for c in every if 2 <= c[0] < 94 and 2 <= c[1] < 78)
    landed = {fw.LIMIT_POS.landing(x, y) for x in range(0, 2048, 8) for y in range(64)}
    assert landed <= {(c, fw.WIDE_ROW) for c in fw.WIDE_COLS} | {None} and len(landed) > 8
    assert len(fw.WIDE_COLS) == 13 and all(c % 64 == 0 and c < 1024 for c in fw.WIDE_COLS) and fw.LIMIT_POS.anchor[1] + fw.WIDE_ROW == (1 << 30) - 64
    assert fw.LIMIT_POS.anchor[0] + 1023 == (1 << 30) - 1                              # columns from 1024 on do not exist
    assert fw.uniform_rounds(fw.TWO24, fw.image_of(fw.TWO24)) > 1000 and fw.uniform_rounds(fw.KM, fw.image_of(fw.KM)) == 0


@PLACES
def test_the_far_scenes_satisfy_the_guards(place):
    tab = jr.table()
    image, cost, dist2 = fw.tables_of(place)
    q, gxy, goal, starts, pot, walks = fw.plan_restated(place, cost)
    assert pr.window_cell(*gxy, place.cell, place.anchor, place.nx, place.ny) == goal
    want = fr.frontiers_propagate(image, cost, pot, fr.params(min_cells=2))
    assert want[2][2] >= 1                                                             # a frontier
    fw.traj_restated(place, cost, pot, tab)
    fw.match_restated(place, dist2, tab)
    fw.cast_restated(place, image, tab)
    pts, mq_, _ = fw.mcl_scene(place)
    A = fw.frame_cloud(pts)
    f = mr.Filter(mq_, tml.MQ, tab)
    fw.mcl_drive(place, f, lambda: f.update(A, dist2, place.anchor))
    b = br.Filter(mq_, place.mq, tab, BEAM)
    fw.mcl_drive(place, b, lambda: b.update(A, dist2, place.anchor, image), rounds=1)
    assert b.binfo["n_rays"] > b.binfo["n_skipped"]


def hyp_restated(place, image, dist2, tab):
    f = hr.Filter(tml.q_of(**fw.HYP_MCL), tml.MQ, tab, hr.params(**fw.HYP_Q))
    assert f.init_uniform(image, place.anchor)
    infos = []
    for k, pts in enumerate(fw.hyp_frames()):
        found = f.parts.copy()
        infos.append(f.update(fw.frame_cloud(pts), dist2, place.anchor, image=image)[3])
        if k == 0:
            bins = {(by, bx) for by, bx, _ in hr.bins_of(found, f.hq)}
            f.predict(*fw.PREDICT)
    fw.hyp_guard(place, infos[0], infos[1], bins, int((f.parts["parent"] == hr.NO_PARENT).sum()))
    return infos[0]["n_bins"]


def test_the_hypotheses_clamp_engages_at_two24_on_the_restatement():
    tab = jr.table()
    image, _, dist2 = fw.tables_of(fw.ORIGIN, sym=True)
    assert hyp_restated(fw.TWO24, image, dist2, tab) < hyp_restated(fw.ORIGIN, image, dist2, tab)


@pytest.mark.parametrize("name", ["km", "two24", "limit_neg"])
def test_the_far_sequences_satisfy_the_guards(name):
    q, frames, poses, guard = fw.far_sequences()[name]
    clouds = [tr.moved(parts, tm.TRANS) for parts in frames]
    h = tm.restate_sequence(q, [(A, tm.NO_G) for A in clouds], tm.TRANS[:3], poses)
    if guard:
        fw.mpr.guards(h)
        fw.mpr.scroll_guards(h)
    fw.sequence_guards(name, h, clouds, poses)


def b_inputs():
    vals = [np.asarray(fw.B_POSES).ravel(), np.asarray(fw.B_TRANS).ravel()]
    for (parts, A), (tx, ty) in zip(fw.b_frames(), fw.B_POSES):
        vals += [A[:, :3].ravel(), A[:, 0].astype(np.float64) + tx, A[:, 1].astype(np.float64) + ty]
    return np.concatenate(vals)


def test_the_shift_is_exact_for_every_input():
    v = b_inputs()
    assert len(v) > 10000 and np.abs(v).max() <= 64.0 and (v * 128.0 == np.rint(v * 128.0)).all()
    assert F32(1.0) / F32(fw.B_CELL) == 8.0 and fw.B_SHIFT == (8192.0, -8192.0)
    assert fw.exact_under_shift(v, fw.B_SHIFT[0]) and fw.exact_under_shift(v, fw.B_SHIFT[1])
    assert not fw.exact_under_shift([float(F32(0.1))], fw.B_SHIFT[0])                  # (the check can fail)


# ---- GPU: part A --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    with capi.CloudMerger(max_points_total=16384, max_sensors=2, flags=capi.FLAG_PROFILE) as cm:
        yield cm


def put(cm, place, sym=False):
    """The placement's map through cm_map_load on the shared context, the cost layer over it."""
    tm.configure(cm, place.mq)
    cm.map_cost_configure(fw.COST_Q["inscribed_radius"], fw.COST_Q["inflation_radius"], fw.COST_Q["cost_scaling"], False)
    tcs.load(cm, fw.image_of(place, sym), place.anchor, place.mq)
    return cm.map_occupancy()[0]


def plan_in_lockstep(cm, place, cost):
    q, gxy, goal, starts, want, walks = fw.plan_restated(place, cost)
    cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], False, q["max_path_cells"])
    info = cm.map_plan_update(*gxy)
    pot, i1 = cm.map_plan()
    assert tp.plan_tuple(info) == tp.plan_tuple(i1) == (goal, 0)
    assert pot.dtype == np.uint32 and pot.tobytes() == want.tobytes(), (place.name, np.argwhere(pot != want)[:4])
    for (sxy, start), (cells, status, ps) in zip(starts, walks):
        got, pinfo = cm.map_path(*sxy)
        assert tp.path_tuple(pinfo) == (start, goal, len(cells), status, ps, 0), (place.name, start, tp.path_tuple(pinfo))
        assert got.tobytes() == cells.tobytes(), (place.name, start)
    return pot


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["km", "two24", "limit_neg"])
def test_integration_far_away(name):
    q, frames, poses, guard = fw.far_sequences()[name]
    n_cap = tm.n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as cm:
        h = tm.run_sequence(cm, q, frames, poses, tm.TRANS[:3], n_cap, guard=guard, scrolls=guard)
        fw.sequence_guards(name, h, [tr.moved(parts, tm.TRANS) for parts in frames], poses)


@pytest.mark.gpu
@PLACES
def test_image_layers_after_a_load(ctx, place):
    """Cost and dist2, the potential and paths, the frontier labels and table."""
    put(ctx, place)
    image, (cost, dist2, _) = tc.check(ctx, place.cell, fw.COST_Q, place.name)
    pot = plan_in_lockstep(ctx, place, cost)
    want = tf.check(ctx, (image, cost, pot), fr.params(min_cells=2), label=place.name)
    assert want[2][2] >= 1


@pytest.mark.gpu
@PLACES
def test_rollout(ctx, place):
    put(ctx, place)
    cost = ctx.map_cost()[0]
    pot = plan_in_lockstep(ctx, place, cost)
    tq, foot, win, want, winfo = fw.traj_restated(place, cost, pot, tcs.TAB())
    ctx.map_traj_configure(tq["nv"], tq["nw"], tq["n_steps"], foot, tq["occ_scale"], tq["goal_scale"], bool(tq["flags"] & 1))
    info = ctx.map_traj_evaluate(win["x"], win["y"], win["yaw"], (win["v_lo"], win["v_hi"]), (win["w_lo"], win["w_hi"]), win["dt"])
    got, i1 = ctx.map_traj()
    assert ttj.same_info(ttj.info_dict(info), winfo) and bytes(info) == bytes(i1), (place.name, ttj.info_dict(info), winfo)
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, f"{place.name}: {len(bad)} of {len(want)} entries differ, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


@pytest.mark.gpu
@PLACES
def test_match_search_and_pyramid(ctx, place):
    """Correlative matching and branch and bound under a turned prior, then every level of the search's pyramid."""
    put(ctx, place)
    sc = fw.match_scene(place)
    assert tmm.prior_of(sc, tmm.TAB())[0, 1] != 0
    vol, res = tmm.evaluate(ctx, sc, n_cap=16384)
    fw.match_guard(vol, res.n_cells)
    sres, _, _ = tms.evaluate(ctx, sc, n_cap=16384)
    assert sres.score == res.score
    q = tms.search_q(sc)
    tms.configure_search(ctx, q)
    ctx.map_match_search(tmm.prior_of(sc, tmm.TAB()))
    L = mf.field(ctx.map_cost()[1], mf.table(place.cell, q["sigma"], q["max_dist"]))
    for h in range(q["depth"] + 1):
        got, want = ctx.map_match_search_level(h), ms.level(L, h)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (place.name, h)
    ctx.map_match_search_configure(None)
    ctx.map_match_configure(None)


@pytest.mark.gpu
@PLACES
def test_casting(ctx, place):
    image = put(ctx, place)
    poses, want = fw.cast_restated(place, image, tcs.TAB())
    got = tcs.check(ctx, fw.cast_q(poses), None, poses, place.cell)
    fw.cast_guard(place, poses, got)
    assert got.tobytes() == want.tobytes()                                             # (the library's heading table is the restatement's here)
    ctx.map_cast_configure(None)


def cast_from_the_particles(cm, place, image):
    """cm_map_cast_evaluate_mcl reads the particles in place: the same kernel, the other pose layout."""
    parts = cm.map_mcl_particles()
    poses = np.zeros(len(parts), kr.POSE)
    poses["x"], poses["y"], poses["h"] = parts["x"], parts["y"], parts["h"]
    q = dict(max_poses=len(parts), n_bearings=16, range_cells=200, flags=0)
    want, winfo = kr.cast(image, place.cell, place.anchor, q, None, poses, tcs.TAB())
    assert (want["status"] != kr.S_NO_ORIGIN).any() and (not place.wide or (want["status"] == kr.S_NO_ORIGIN).any())
    for plain in (False, True):
        cm.map_cast_configure(q["max_poses"], q["n_bearings"], q["range_cells"], plain)
        info = cm.map_cast_particles()
        assert cm.map_cast_rays()[0].tobytes() == want.tobytes() and [getattr(info, f) for f in tcs.INFO] == [winfo[f] for f in tcs.INFO]
    cm.map_cast_configure(None)


class Driven:
    """A lockstep pair behind the Filter interface tests/far_windows.py's mcl_drive wants."""

    def __init__(self, pair):
        self.p, self.init_pose, self.predict = pair, pair.init_pose, pair.predict

    parts = property(lambda self: self.p.f.parts)

    def update(self):
        w, info, _ = self.p.update()[:3]
        return w, info


@pytest.mark.gpu
@PLACES
def test_the_particle_filter(ctx, place):
    """init_pose, predict, two updates; then init_uniform (at two24 with the rounded (float)(ax + ix)) and an update."""
    image = put(ctx, place)
    pts, q, _ = fw.mcl_scene(place)
    tml.frame(ctx, pts)
    d = Driven(tml.Pair(ctx, q))
    fw.mcl_drive(place, d, d.update)
    cast_from_the_particles(ctx, place, image)
    parts = d.p.init_uniform()
    on, ix, iy = place.cells(parts["x"], parts["y"])
    assert len(set(zip(ix[on].tolist(), iy[on].tolist()))) > (4 if place.wide else 60)
    if place is fw.TWO24:
        assert fw.uniform_rounds(place, image) > 1000
    w, info, _ = d.p.update()
    assert info.n_beams > 0
    ctx.map_mcl_configure(None)


@pytest.mark.gpu
@PLACES
def test_the_beam_model(ctx, place):
    put(ctx, place)
    pts, q, _ = fw.mcl_scene(place)
    tml.frame(ctx, pts)
    for plain in (0, 1):
        d = Driven(tmb.BeamPair(ctx, q, dict(BEAM, flags=plain), place.mq))
        fw.mcl_drive(place, d, d.update, rounds=1)
        assert d.p.f.binfo["n_rays"] > d.p.f.binfo["n_skipped"]
    ctx.map_mcl_configure(None)


@pytest.mark.gpu
def test_the_hypotheses_at_two24_clamp(ctx):
    """bin_q = 64 and 256 heading bins from a uniform start: at the origin nearly every particle has a bin of its own; at two24
    every position clamps at 2^20 m, the bins differ by heading alone and the neighbour walk meets its bin bound. A second
    frame that fits badly makes the recovery inject: those particles are init_uniform's, with the rounded (float)(ax + ix)."""
    n_bins = {}
    for place in (fw.ORIGIN, fw.TWO24):
        put(ctx, place, sym=True)
        p = tmh.HypPair(ctx, tml.q_of(**fw.HYP_MCL), hr.params(**fw.HYP_Q))
        p.init_uniform()
        infos = []
        for k, pts in enumerate(fw.hyp_frames()):
            tml.frame(ctx, pts)
            found = p.f.parts.copy()
            p.update()
            infos.append(p.f.hinfo)
            if k == 0:
                bins = {(by, bx) for by, bx, _ in hr.bins_of(found, p.f.hq)}
                p.predict(*fw.PREDICT)
        fw.hyp_guard(place, infos[0], infos[1], bins, int((ctx.map_mcl_particles()["parent"] == capi.MCL_NO_PARENT).sum()))
        n_bins[place.name] = infos[0]["n_bins"]
    assert n_bins["two24"] < n_bins["origin"], n_bins
    ctx.map_mcl_configure(None)


# ---- GPU: part B, the exact shift ----------------------------------------------------------------------------------------------
AXIS_YAWS = (0.0, math.pi / 2, math.pi, -math.pi / 2)


def exact(v):
    assert float(F32(v)) == v, v
    return float(v)


def b_run(cm, k):
    """Everything part B compares, with the world shifted by k * B_SHIFT: a dictionary of bytes and tuples that must not depend
    on k, and the anchors and pose outputs with the shift taken off again."""
    sx, sy = k * fw.B_SHIFT[0], k * fw.B_SHIFT[1]
    nx, ny, cell = fw.B_NX, fw.B_NY, fw.B_CELL
    out = {}
    tm.configure(cm, fw.B_MQ)
    for f, ((parts, A), (tx, ty)) in enumerate(zip(fw.b_frames(), fw.B_POSES)):
        tg.run_frame(cm, [xyzi_cloud(p[:, :3], p[:, 3], t_xyz=fw.B_TRANS[s]) for s, p in enumerate(parts)], tc.PARAMS)
        assert tg.host_clouds(cm, 16384, False)[0][:, :3].tobytes() == A.tobytes()
        info = cm.map_integrate(tm.pose_t(exact(tx + sx), exact(ty + sy)))
        out[f"table {f}"], out[f"image {f}"] = cm.map()[0].tobytes(), cm.map_occupancy()[0].tobytes()
        out[f"anchor {f}"] = (info.anchor[0] - k * fw.B_SHIFT_CELLS, info.anchor[1] + k * fw.B_SHIFT_CELLS, info.sensors_cast)
    image = cm.map_occupancy()[0]
    ax, ay = cm.map()[1].anchor
    world = lambda ix, iy, ox=0.0, oy=0.0: (exact((ax + ix + 0.5) * cell + ox), exact((ay + iy + 0.5) * cell + oy))
    assert (image == 0).sum() > 500 and (image == 100).sum() > 100 and (image == -1).sum() > 100
    cm.map_cost_configure(0.0, 0.375, 3.0, False)
    cm.map_cost_update()
    cost, dist2, _ = cm.map_cost()
    out["cost"], out["dist2"] = cost.tobytes(), dist2.tobytes()
    # plan: the goal and the start are free cells of the image, named by their exact centres
    free = np.argwhere((image == 0) & (cost < 100))
    goal, start = tuple(int(v) for v in free[len(free) // 9][::-1]), tuple(int(v) for v in free[-(len(free) // 7)][::-1])
    cm.map_plan_configure(50, 205, True, nx * ny)
    pinfo = cm.map_plan_update(*world(*goal))
    assert tuple(pinfo.goal) == goal
    out["pot"] = cm.map_plan()[0].tobytes()
    path, pi = cm.map_path(*world(*start))
    out["path"], out["path info"] = path.tobytes(), tp.path_tuple(pi)
    assert tuple(pi.start) == start and len(path) > 5
    cm.map_frontier_configure(2)
    finfo = cm.map_frontier_update()
    out["labels"], out["frontiers"], out["frontier info"] = cm.map_frontier_labels()[0].tobytes(), cm.map_frontiers()[0].tobytes(), tf.info_tuple(finfo)
    assert finfo.n_frontiers >= 1
    # cast: poses on the 2^-7 lattice, inside and just outside the window
    rng = np.random.default_rng(8)
    rows = [world(ix, iy, ox * fw.B_LATTICE, oy * fw.B_LATTICE) + (int(h),)
            for ix, iy, ox, oy, h in zip(rng.integers(-2, nx + 2, 80), rng.integers(-2, ny + 2, 80), rng.integers(-8, 8, 80), rng.integers(-8, 8, 80),
                                         rng.integers(0, 1 << 32, 80))]
    cm.map_cast_configure(80, 32, 60, False, None)
    cinfo = cm.map_cast(kr.poses_of(rows))
    out["rays"] = cm.map_cast_rays()[0].tobytes()
    assert cinfo.n_hit > 0 and cinfo.n_no_origin > 0
    # match: the last frame under axis-aligned priors beside the pose it was integrated under
    tx, ty = fw.B_POSES[-1]
    cm.map_match_configure(0.1, 0.3, 0, 1, 4, 3, False)
    for name, lin in (("identity", [[1, 0, 0], [0, 1, 0]]), ("quarter turn", [[0, -1, 0], [1, 0, 0]])):
        P = tm.pose_t(exact(tx + 0.25 + sx), exact(ty - 0.125 + sy))
        P[:2, :3] = lin
        res = cm.map_match(P)
        out[f"volume {name}"] = cm.map_match_scores()[0].tobytes()
        out[f"match {name}"] = (res.best, res.k, res.i, res.j, res.score, res.n_cells, res.max_score, float(res.pose[3]) - sx, float(res.pose[7]) - sy)
        assert res.n_cells > 0 and (name != "identity" or (res.score > 0 and (res.i, res.j) == (-2, 1)))
    # the particle filter: every particle on one lattice pose, the four axis headings; then the same under the beam model
    cm.map_mcl_configure(64, 256, 64, 0.1, 0.5, 8.0, 0.5, False, 9)
    for mode in ("field", "beam"):
        if mode == "beam":
            cm.map_mcl_beam_configure(8, 0.1, 0.75, 0.125, 0.125, False)
        for yaw in AXIS_YAWS:
            cm.map_mcl_init_pose(exact(tx + 0.5 + sx), exact(ty - 0.25 + sy), yaw, 0.0, 0.0, 0.0)
            parts = cm.map_mcl_particles()
            assert jr.entry(int(parts["h"][0])) in (0, 1024, 2048, 3072) and len(set(parts["h"].tolist())) == 1
            info = cm.map_mcl_update()
            w, _ = cm.map_mcl_weights()
            assert info.n_beams > 0 and w["score"][0] > 0 and (w["score"] == w["score"][0]).all()
            out[f"{mode} weights {yaw:.2f}"] = w.tobytes()
            out[f"{mode} info {yaw:.2f}"] = (info.n_beams, info.n_cells, info.sum_w, info.best, float(parts["x"][0]) - sx, float(parts["y"][0]) - sy)
        if mode == "beam":
            b = cm.map_mcl_beam_info()
            out["beam counts"] = (b.n_rays,) + tuple(getattr(b, f) for f in br.COUNTS)
    assert len({out[f"field weights {yaw:.2f}"] for yaw in AXIS_YAWS}) > 1           # the heading matters
    return out


@pytest.mark.gpu
def test_an_exact_shift_changes_nothing():
    """A map of 0.125 m cells, every coordinate on a multiple of 2^-7 m within 64 m, the world moved by 65 536 cells on x and
    -65 536 on y: every sum of xf_row and every product with inv = 8 is exact in fp32 either way (asserted on the CPU above), so
    the two runs must agree in every byte, and the anchors and pose outputs once the shift is taken off."""
    with capi.CloudMerger(max_points_total=16384, max_sensors=2) as cm:
        a = b_run(cm, 0)
    with capi.CloudMerger(max_points_total=16384, max_sensors=2) as cm:
        b = b_run(cm, 1)
    assert a.keys() == b.keys()
    assert [k for k in a if a[k] != b[k]] == []
