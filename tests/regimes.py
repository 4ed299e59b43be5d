"""Helpers of tests/test_regimes.py: the scenes with their references, the collections of by-product and layer calls, a stream
that is kept busy, and the published pipeline. Nothing in here is a test.

The collections are those of the suites: tests/test_byproduct_layouts.py's by_products() against restated(), the four layers it
leaves out (layers() against layers_restated()), tests/test_byproduct_reuse.py's five_calls() with its suites' checkers, and
tests/test_ctx_memory.py's map_calls() with tests/test_boxes.py's check and the grid and ray restatements. Every expected value
is a restatement's; every comparison is of bytes."""
import ast
import ctypes as C
import threading

import numpy as np

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from oracle import oracle
from tests import cast_ref as kr
from tests import cost_ref as cr
from tests import frame_host as fh
from tests import front_ref as fr
from tests import grid_ref as gr
from tests import match_ref as mf
from tests import match_search_ref as ms
from tests import mcl_ref as mr
from tests import plan_ref as pr
from tests import rays_ref as rr
from tests import test_boxes as tb
from tests import test_byproduct_layouts as bl
from tests import test_byproduct_reuse as bu
from tests import test_ctx_memory as cmem
from tests import test_map_cast as tcs
from tests import test_map_frontier as tf
from tests import test_map_match as tmm
from tests import test_map_match_search as tms
from tests import test_map_plan as tp
from tests import test_map_traj as ttj
from tests import traj_ref as jr
from tests.test_gpu_parity import BUCKET, SPLIT
from tests.util import SEQ_EXACT_MAX, assert_centroids_close_or_exact, same_bits, xyzi_of

F32 = np.float32
SEEDS = (41, 42, 44, 47)
# The small scene: no sensor above 300 points (two of them above 100, so the hand-placed values are in it), the seed the first
# from 60 on (60 has no counted point with the NaN intensity) for which restated() and layers_restated() pass every guard.
SMALL_COUNTS = [300, 0, 1, 257, 130, 63]
SMALL_SEED = 61
N_CAP = bl.N_CAP
LEAF3 = (bu.LATTICE_LEAF,) * 3
NO_G = np.zeros((0, 4), F32)
FOOT = np.array([[0.3, 0.0], [-0.3, 0.2]], F32)


def layer_set(plan=pr.params(50, 205, pr.ALLOW_UNKNOWN), traj=jr.params(4, 5, 8, 1, 1, jr.ALLOW_UNKNOWN), window=((0.0, 30.0), (-1.5, 1.5), 0.1),
              front=fr.params(min_cells=2), n_bearings=32, range_cells=60, n_poses=40):
    """What layers() configures and layers_restated() restates."""
    return dict(plan=plan, traj=traj, window=window, front=front, n_bearings=n_bearings, range_cells=range_cells, n_poses=n_poses)


# The second parameter set: every host-built table differs from the first one's (the cost table by the radii and the scaling,
# the match, search and localisation tables by sigma and max_dist, the cast layer's directions by range_cells), and so do the
# sizes of the volumes, the beams, the particles and their seed.
PSET_B = bl.parameter_set(match=mf.params(sigma=0.35, max_dist=1.5, n_a=3, a_stride=6, wx=2, wy=3),
                          search=ms.params(sigma=0.35, max_dist=1.5, n_a=3, a_stride=6, wx=2, wy=3, depth=1),
                          mcl=mr.params(n_particles=80, max_beams=96, range_cells=24, sigma=0.35, max_dist=1.5, tau=6.0, resample_frac=0.5, flags=0, seed=11),
                          cost=(0.25, 1.5, 2.0, False))
LSET_B = layer_set(plan=pr.params(40, 128, pr.ALLOW_UNKNOWN), traj=jr.params(5, 4, 7, 2, 1, jr.ALLOW_UNKNOWN), window=((0.0, 24.0), (-1.0, 1.0), 0.125),
                   front=fr.params(min_cells=3), n_bearings=48, range_cells=40, n_poses=33)


# ---- the four layers by_products() leaves out ------------------------------------------------------------------------------------
def traj_info_bytes(d):
    return repr((d["best"], d["n_valid"], tuple(d["start"]), F32(d["best_v"]).tobytes(), F32(d["best_w"]).tobytes())).encode()


def layers_restated(want, pset, lset):
    """The plan layer with one path, the rollout, the frontiers and a cast over restated()'s map image and dist2. Returns
    ({name: bytes}, the calls' arguments). Goal, start, window and poses are chosen from the reference, and the guards are
    conditions on it: a finite potential at the start and a path that is found, samples that survive and samples that do not,
    at least two frontiers, rays that hit, rays that leave and poses without an origin cell."""
    mq = pset["mq"]
    nx, ny, cell = mq["nx"], mq["ny"], mq["cell"]
    image = np.frombuffer(want["map_image"], np.int8).reshape(ny, nx)
    anchor = tuple(ast.literal_eval(want["map_info"].decode())[0])
    c = pset["cost"]
    cost, d2, _ = cr.cost_separable(image, cell, cr.params(c[0], c[1], c[2], int(c[3])))
    assert d2.astype(np.uint32).tobytes() == want["dist2"]
    out, args = {"cost": cost.tobytes()}, {}
    tab = bl.TAB()
    # plan: the goal a free cell near the window's lower edge, the start the reachable free cell farthest from it
    q = dict(lset["plan"], max_path_cells=nx * ny)
    assert pr.refusal(q, nx, ny) is None
    free = np.argwhere((image == 0) & (cost < 253))
    assert len(free) > 100
    goal = tuple(int(v) for v in free[len(free) // 9][::-1])
    pot = pr.potential_dijkstra(cost, q, goal)
    reach = np.where((pot != pr.UNREACHABLE) & (image == 0) & (cost < 253), pot.astype(np.int64), -1)
    start = tuple(int(v) for v in np.unravel_index(int(reach.argmax()), reach.shape)[::-1])
    cells, status, pot_start = pr.walk(pot, cost, q, goal, start, q["max_path_cells"])
    assert pot_start != pr.UNREACHABLE and status == pr.FOUND and len(cells) > 5 and (pot == pr.UNREACHABLE).any()
    pr.check_path(cells, status, pot, cost, q, goal)
    args["goal"], args["start"] = pr.cell_centre(*goal, cell, anchor), pr.cell_centre(*start, cell, anchor)
    assert pr.window_cell(*args["goal"], cell, anchor, nx, ny) == goal and pr.window_cell(*args["start"], cell, anchor, nx, ny) == start
    out["pot"], out["plan_info"] = pot.tobytes(), repr((goal, 0)).encode()
    out["path"], out["path_info"] = cells.tobytes(), repr((start, goal, len(cells), status, pot_start, 0)).encode()
    # rollout: from the start, heading along the path's first step
    nxt = (int(cells[1]) % nx - start[0], int(cells[1]) // nx - start[1])
    yaw = float(np.arctan2(nxt[1], nxt[0]))
    v, w, dt = lset["window"]
    win = jr.window(args["start"][0], args["start"][1], yaw, v, w, dt)
    tq = lset["traj"]
    assert jr.refusal(tq, FOOT) is None and jr.refusal(tq, FOOT, win, cell, anchor, nx, ny) is None
    scores, tinfo = jr.rollout(cost, pot, anchor, cell, tq, FOOT, win, tab)
    jr.guards(scores, ("some_valid",))
    assert (scores["status"] != jr.VALID).any() and tinfo["start"] == start
    args["win"] = win
    out["traj"], out["traj_info"] = scores.tobytes(), traj_info_bytes(tinfo)
    # frontiers
    fq = lset["front"]
    labels, table, finfo = fr.frontiers_propagate(image, cost, pot, fq)
    assert finfo[2] >= 2 and finfo[3] == finfo[2], finfo
    out["front_labels"], out["front_table"], out["front_info"] = labels.tobytes(), table.tobytes(), repr(tuple(finfo)).encode()
    # cast: poses at the centres of free cells and four outside the window
    rng = np.random.default_rng(17)
    pick = free[rng.choice(len(free), lset["n_poses"] - 4, replace=False)]
    at = [(int(ix), int(iy)) for iy, ix in pick] + [(-2, 10), (nx + 1, 5), (10, -3), (10, ny + 2)]
    poses = kr.poses_of([pr.cell_centre(ix, iy, cell, anchor) + (int(h),) for (ix, iy), h in zip(at, rng.integers(0, 1 << 32, len(at)))])
    cq = dict(max_poses=len(poses), n_bearings=lset["n_bearings"], range_cells=lset["range_cells"], flags=0)
    rays, cinfo = kr.cast(image, cell, anchor, cq, None, poses, tab)
    assert cinfo["n_hit"] > 0 and cinfo["n_off_map"] > 0 and cinfo["n_no_origin"] == 4 * cq["n_bearings"], cinfo
    args["poses"], args["cast_q"] = poses, cq
    out["cast_rays"], out["cast_info"] = rays.tobytes(), repr(tuple(cinfo[f] for f in tcs.INFO)).encode()
    return out, args


def layers(cm, args, lset, configure=True):
    """The same calls on the map by_products() integrated: {name: bytes}. configure False: the producers alone, on the layers
    as they stand."""
    out = {"cost": cm.map_cost()[0].tobytes()}
    q = lset["plan"]
    if configure:
        cm.map_plan_configure(q["neutral"], q["cost_factor_q8"], bool(q["flags"] & 1))
    info = cm.map_plan_update(*args["goal"])
    pot, i1 = cm.map_plan()
    assert tp.plan_tuple(info) == tp.plan_tuple(i1)
    out["pot"], out["plan_info"] = pot.tobytes(), repr(tp.plan_tuple(info)).encode()
    path, pinfo = cm.map_path(*args["start"])
    out["path"], out["path_info"] = path.tobytes(), repr(tp.path_tuple(pinfo)).encode()
    tq, w = lset["traj"], args["win"]
    if configure:
        cm.map_traj_configure(tq["nv"], tq["nw"], tq["n_steps"], FOOT, tq["occ_scale"], tq["goal_scale"], bool(tq["flags"] & 1))
    info = cm.map_traj_evaluate(w["x"], w["y"], w["yaw"], (w["v_lo"], w["v_hi"]), (w["w_lo"], w["w_hi"]), w["dt"])
    got, i1 = cm.map_traj()
    assert bytes(info) == bytes(i1)
    out["traj"], out["traj_info"] = got.tobytes(), traj_info_bytes(ttj.info_dict(info))
    fq = lset["front"]
    if configure:
        cm.map_frontier_configure(fq["min_cells"], fq["max_frontiers"], fq["max_cost"], fq["pot_scale"], fq["gain_scale"])
    info = cm.map_frontier_update()
    table, i1 = cm.map_frontiers()
    labels, i2 = cm.map_frontier_labels()
    assert tf.info_tuple(info) == tf.info_tuple(i1) == tf.info_tuple(i2)
    out["front_labels"], out["front_table"], out["front_info"] = labels.tobytes(), table.tobytes(), repr(tf.info_tuple(info)).encode()
    cq = args["cast_q"]
    if configure:
        cm.map_cast_configure(cq["max_poses"], cq["n_bearings"], cq["range_cells"], False)
    info = cm.map_cast(args["poses"])
    rays, i1 = cm.map_cast_rays()
    assert bytes(info) == bytes(i1)
    out["cast_rays"], out["cast_info"] = rays.tobytes(), repr(tuple(getattr(info, f) for f in tcs.INFO)).encode()
    return out


# ---- the scenes and their references ---------------------------------------------------------------------------------------------
class SceneRef:
    """A base_scene as XYZI16 clouds with everything the regimes compare against: restated() and layers_restated() under a
    parameter set (their guards run here, before any device output exists) and the oracle's voxel grid."""

    def __init__(self, seed, counts=bl.COUNTS, pset=None, lset=None):
        self.seed, self.counts = seed, list(counts)
        self.pset, self.lset = pset or bl.parameter_set(), lset or layer_set()
        self.parts, self.dropped = bl.base_scene(seed, counts=counts)
        self.clouds = bl.clouds_in(self.parts, ["xyzi16"] * len(counts))
        self.frame = fh.fuse(self.clouds, bl.PARAMS.crop_min, bl.PARAMS.crop_max)
        self.want, self.structs = bl.restated(self.frame, self.dropped, pset=self.pset, counts=self.counts)
        self.want_layers, self.args = layers_restated(self.want, self.pset, self.lset)
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle.merge_voxelize(self.clouds, bl.PARAMS, threads=4, stable=True)
            assert self._oracle[0] == oracle.OK
        return self._oracle

    def raw(self, s):
        return np.ascontiguousarray(self.clouds[s].data).view(np.uint8).reshape(-1)


_REFS = {}


def scene_ref(seed, which="a"):
    """The cached reference of base_scene(seed) under the first ("a") or the second ("b") parameter set; seed "small": the
    small scene."""
    key = (seed, which)
    if key not in _REFS:
        pset, lset = (None, None) if which == "a" else (PSET_B, LSET_B)
        _REFS[key] = SceneRef(SMALL_SEED, SMALL_COUNTS, pset, lset) if seed == "small" else SceneRef(seed, pset=pset, lset=lset)
    return _REFS[key]


def check_scene(cm, ref, label, n_cap=N_CAP):
    """Both collections of the map side on the context's last frame, which must be ref's."""
    got = bl.by_products(cm, n_cap, ref.pset)
    bl.against_restatement(got, ref.want, label)
    bl.check_structs(bl.structs_of(got), ref.structs)
    bl.against_restatement(layers(cm, ref.args, ref.lset), ref.want_layers, label + ", layers")


def check_settled(cm, ref, label):
    """The producers once more, with no configure call in between: what the tables a context keeps must still give."""
    cm.map_cost_update()
    cost, dist2, _ = cm.map_cost()
    assert cost.tobytes() == ref.want_layers["cost"] and dist2.tobytes() == ref.want["dist2"], f"{label}: the cost tables"
    res = cm.map_match(bl.PRIOR)
    assert cm.map_match_scores()[0].tobytes() == ref.want["match_volume"], f"{label}: the match volume"
    assert tmm.same_result(tmm.result_dict(res), ref.structs["match_result"]), label
    sres, sinfo = cm.map_match_search(bl.PRIOR)
    assert tmm.same_result(tmm.result_dict(sres), ref.structs["search_result"]) and tms.info_dict(sinfo) == ref.structs["search_info"], label
    bl.against_restatement(layers(cm, ref.args, ref.lset, configure=False), ref.want_layers, label + ", layers as they stand")


def storm_ref(ref):
    """The references of table_storm for a scene: the largest tables the two layers take (a radius of 200 cells for the cost
    table, of 64 for the match table, so that building one takes a while), the shape of each still the parameter set's own."""
    mq = ref.pset["mq"]
    nx, ny, cell = mq["nx"], mq["ny"], mq["cell"]
    image = np.frombuffer(ref.want["map_image"], np.int8).reshape(ny, nx)
    dist2 = np.frombuffer(ref.want["dist2"], np.uint32).reshape(ny, nx)
    anchor = tuple(ast.literal_eval(ref.want["map_info"].decode())[0])
    c = (ref.pset["cost"][0], 100.0, ref.pset["cost"][2] / 20.0, False)
    cost, _, cost_lut = cr.cost_separable(image, cell, cr.params(c[0], c[1], c[2], 0))
    q = dict(ref.pset["match"], max_dist=32.0)
    assert cr.refusal(cr.params(c[0], c[1], c[2], 0), cell, nx, ny) is None and mf.refusal(q, cell) is None
    vol, _ = mf.match(ref.frame.A, dist2, mq, anchor, q, bl.PRIOR, bl.TAB())
    match_lut = mf.table(cell, q["sigma"], q["max_dist"])
    assert len(cost_lut) == 200 * 200 + 1 and len(match_lut) == 64 * 64 + 1 and len(set(cost.ravel().tolist())) > 8 and vol.max() > 0
    return dict(cost_args=c, cost_lut=cost_lut.tobytes(), cost=cost.tobytes(), match_q=q, match_lut=match_lut.tobytes(), volume=vol.tobytes())


def table_storm(cm, want, label, rounds=100):
    """The cost layer and the matching layer configured again and again with storm_ref's large tables, each time the table
    read back and the producer run: two threads doing this at once with different parameters build their host tables at the
    same moments, over and over."""
    for k in range(rounds):
        cm.map_cost_configure(*want["cost_args"])
        assert cm.map_cost_table().tobytes() == want["cost_lut"], f"{label}: the cost table, configure call {k}"
        cm.map_cost_update()
        assert cm.map_cost()[0].tobytes() == want["cost"], f"{label}: the cost bytes, configure call {k}"
        tmm.configure_match(cm, want["match_q"])
        assert cm.map_match_table().tobytes() == want["match_lut"], f"{label}: the match table, configure call {k}"
        cm.map_match(bl.PRIOR)
        assert cm.map_match_scores()[0].tobytes() == want["volume"], f"{label}: the match volume, configure call {k}"


def blocking_frame(cm, ref):
    res = bl.run_frame(cm, ref.clouds)
    assert res.n_in == sum(ref.counts)
    return res


# ---- the centroid side: five_calls, the boxes, map_calls -----------------------------------------------------------------------------
_LATTICE = {}


def lattice_ref(step):
    """The lattice of tests/test_byproduct_reuse.py's step with the grid maps and ray tables of map_calls' grids, restated."""
    if step not in _LATTICE:
        xyz = bu.sparse_lattice(*bu.LATTICES[step])
        A = np.concatenate([xyz, np.ones((len(xyz), 1), F32)], axis=1)
        tag, none = np.zeros(len(A), np.int64), np.zeros(0, np.int64)
        tables = []
        for origin, cell, nx, ny in cmem.GRIDS:
            grid, image = gr.grid_vectorised(A, NO_G, origin, cell, nx, ny, (-np.inf, np.inf), 0.3, 1)
            rays, cleared, _ = rr.rays_vectorised(A, NO_G, tag, none, [(0.0, 0.0)], origin, cell, nx, ny, (-np.inf, np.inf), 0.3, 1, 1, 0)
            assert (grid["n"] > 0).sum() > 20 and (rays["n_pass"] > 0).sum() > 20
            tables.append((grid.tobytes(), image.tobytes(), rays.tobytes(), cleared.tobytes()))
        _LATTICE[step] = (xyz, tables)
    return _LATTICE[step]


def same_points(rec, xyz):
    """The result's centroids are the lattice's points bit for bit (every point its own voxel)."""
    got = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).view(np.uint32)
    key = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    return np.array_equal(key(got), key(np.ascontiguousarray(xyz, F32).view(np.uint32)))


def check_lattice(cm, res, step, label):
    """five_calls with its suites' checkers, the boxes through tests/test_boxes.py's check, map_calls, and map_calls' tables
    against the restatements. The context's last frame must be the lattice of `step`."""
    xyz, tables = lattice_ref(step)
    assert res.status == capi.OK and res.n_out == len(xyz) and same_points(cm.result(res.n_out), xyz), label
    bu.five_calls(cm, res, xyz, LEAF3, bu.TOL, checked=True)
    tb.check(cm, res, bu.TOL, vacuous_ok=True)             # (a lattice's boxes all lie along the axes: check_shapes has the turned ones)
    cmem.map_calls(cm)
    for (origin, cell, nx, ny), (grid, image, rays, cleared) in zip(cmem.GRIDS, tables):
        assert cm.grid_map(origin, cell, nx, ny).tobytes() == grid and cm.grid_occupancy().tobytes() == image, f"{label}: grid map {nx} x {ny}"
        assert cm.grid_rays(origin, cell, nx, ny).tobytes() == rays and cm.grid_ray_occupancy().tobytes() == cleared, f"{label}: rays {nx} x {ny}"


SHAPES_LEAF = 0.04
_SHAPES = []


def shapes_ref():
    """tests/test_boxes.py's turned L-shapes and rectangles, ten of each, every point the centre of its own voxel."""
    if not _SHAPES:
        _SHAPES.append(tb.snap(tb.shapes_for_gpu(0.0) * [1, 1, 0], SHAPES_LEAF))
        assert 4096 < len(_SHAPES[0]) <= bu.CAP
    return _SHAPES[0]


def shapes_frame(cm):
    return tb.submit_as_voxels(cm, shapes_ref(), SHAPES_LEAF)


def check_shapes(cm, res, label):
    """The boxes of the turned shapes through tests/test_boxes.py's check, its guards on (two boxes, two headings) and its
    suite's own: twenty clusters at eight headings or more."""
    xyz = shapes_ref()
    assert res.status == capi.OK and res.n_out == len(xyz) and same_points(cm.result(res.n_out), xyz), label
    want, table = tb.check(cm, res, 1.0, 5, tb.NONE)
    assert len(table) == 20 and len(set(want["angle"].tolist())) >= 8, label


def lattice_context():
    return capi.CloudMerger(max_points_total=bu.CAP, max_sensors=1, flags=bu.FLAGS)


def scene_context():
    return capi.CloudMerger(max_points_total=N_CAP, max_sensors=6, flags=capi.FLAG_OCCUPANCY)


# ---- the voxel grid against the oracle -----------------------------------------------------------------------------------------------
def check_result(cm, res, ref, rec16, label):
    """The frame's counts, fused cloud and occupancy bit for bit, its centroids as tests/test_gpu_parity.py holds them: bit for
    bit where the route adds in the oracle's order (SEQ_EXACT_MAX), assert_centroids_close_or_exact everywhere. A voxel that holds the NaN
    intensity has a NaN intensity on both sides; its xyz is compared like any other."""
    st, merged, out, rep = ref.oracle
    assert res.status == capi.OK and res.n_merged == rep.n_merged and res.n_out == rep.n_out, label
    got_merged = cm.merged(N_CAP)
    assert same_bits(np.stack([got_merged[k] for k in ("x", "y", "z", "intensity")], axis=1), xyzi_of(merged)), label
    cells, counts = cm.cells(res.n_out)
    assert np.array_equal(cells, rep.cells) and np.array_equal(counts, rep.counts), label
    got = np.stack([rec16[k] for k in ("x", "y", "z", "intensity")], axis=1)
    want = xyzi_of(out)
    # (tests/test_layouts.py's check_oracle: which voxels the frame's route adds in the oracle's order)
    if res.path_flags & BUCKET:
        small = np.ones(len(counts), bool) if not res.path_flags & SPLIT else counts <= SEQ_EXACT_MAX
    else:
        small = counts <= 2
    assert small.any() and same_bits(got[small], want[small]), f"{label}: the centroids the route adds in the oracle's order"
    nan = np.isnan(want[:, 3])
    assert np.array_equal(np.isnan(got[:, 3]), nan) and np.isfinite(want[:, :3]).all(), label
    g, w = got.copy(), want.copy()
    g[nan, 3] = w[nan, 3] = 0
    assert_centroids_close_or_exact(g, w, counts, rep.cells, merged, bl.PARAMS.leaf, sequential=False)


# ---- a caller's stream that always has work queued --------------------------------------------------------------------------------------
class BusyStream:
    """Keeps a few milliseconds of matrix products queued on a stream from a thread of its own, so that whatever the library
    launches on that stream starts late, while a launch that went to another stream starts at once and finds its inputs not yet
    written. At most two batches are queued at a time."""

    def __init__(self, stream, batch=6, n=2048):
        import torch
        self.torch, self.stream, self.batch = torch, stream, batch
        with torch.cuda.stream(stream):
            self.a = torch.full((n, n), 1.0 / n, device="cuda")
            self.b = torch.full((n, n), 1.0, device="cuda")
        stream.synchronize()
        self.stop, self.error, self.batches = threading.Event(), None, 0
        self.thread = threading.Thread(target=self.run, daemon=True)

    def run(self):
        torch = self.torch
        try:
            last = None
            while not self.stop.is_set():
                with torch.cuda.stream(self.stream):
                    for _ in range(self.batch):
                        self.b = self.a @ self.b
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                if last is not None:
                    last.synchronize()
                last = ev
                self.batches += 1
        except Exception as e:                               # pragma: no cover
            self.error = e

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *a):
        self.stop.set()
        self.thread.join(60)
        assert not self.thread.is_alive(), "the busy stream's thread did not end"
        self.stream.synchronize()
        if a[0] is None:
            assert self.error is None, self.error
            assert self.batches > 2, "the stream was never busy"


def backlog(torch, stream, n=2048, products=24):
    """A few milliseconds of work on the stream, queued without waiting."""
    with torch.cuda.stream(stream):
        a = torch.full((n, n), 1.0 / n, device="cuda")
        b = torch.full((n, n), 1.0, device="cuda")
        for _ in range(products):
            b = a @ b
    return b


def hip():
    h = tb.hip_rt()
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    return h


# ---- the published pipeline ------------------------------------------------------------------------------------------------------------
class Pinned:
    """Pinned copies of the scenes' clouds, and pinned destinations for the published results."""

    def __init__(self):
        self.holders = []

    def of(self, raw):
        h = capi.pinned_array(max(len(raw), 16))
        h.array[:len(raw)] = raw
        self.holders.append(h)
        return h

    def zeros(self, nbytes):
        h = capi.pinned_array(max(nbytes, 16))
        h.array[:] = 0
        self.holders.append(h)
        return h

    def free(self):
        for h in self.holders:
            h.free()
        self.holders = []


def device_bytes(ptr, nbytes):
    out = np.zeros(nbytes, np.uint8)
    if nbytes:
        assert hip().hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out.tobytes()


def scene_pipeline(cm, refs, pinned, label, first_step=16):
    """The node shell's order of calls over the scenes `refs` on one context: asynchronous submits from pinned memory,
    merge_voxelize_async + wait, the result read, publish_async with no publish_wait, the NEXT frame's clouds submitted at once,
    then every collection on the frame at rest. step_out alternates. After the last frame: publish_wait, and every destination
    holds the bytes cm_result_copy gave for its frame. A frame's device buffer still holds it while its successor is at rest (it
    is the buffer the copy-out reads), and the successor lives in the other one."""
    clouds = [[pinned.of(ref.raw(s)) for s in range(len(ref.clouds))] for ref in refs]
    dsts = [pinned.zeros(32 * sum(ref.counts)) for ref in refs]
    for s, c in enumerate(refs[0].clouds):
        cm.set_transform(s, c.q_xyzw, c.t_xyz)                  # (every scene has the poses of pose_of)

    def submit(n):
        for s, c in enumerate(refs[n].clouds):
            assert cm.submit_async(s, c, host_ptr=clouds[n][s].ptr.value) == capi.OK, (label, n, s)

    submit(0)
    published, last = [], None
    for n, ref in enumerate(refs):
        what = f"{label}, frame {n} (scene {ref.seed})"
        assert cm.merge_voxelize_async(capi.make_params(bl.PARAMS)) == capi.OK
        res = cm.wait()
        step = first_step if n % 2 == 0 else 48 - first_step
        rec16 = cm.result(res.n_out, 16)
        shown = rec16.tobytes() if step == 16 else cm.result(res.n_out, 32).tobytes()
        ptr, n_dev = cm.result_device()
        assert n_dev == res.n_out and len(shown) == res.n_out * step
        if last is not None:
            assert ptr != last[0], f"{what}: the frame wrote the buffer its predecessor's copy-out reads"
            assert device_bytes(*last[:2]) == last[2], f"{what}: the predecessor's result did not stay in its buffer"
        cm.publish_async(dsts[n].ptr.value, res.n_out, step)
        if n + 1 < len(refs):
            submit(n + 1)
        published.append(shown)
        last = (ptr, 16 * res.n_out, rec16.tobytes())
        check_result(cm, res, ref, rec16, what)
        check_scene(cm, ref, what)
    cm.publish_wait()
    for n, shown in enumerate(published):
        assert dsts[n].array[:len(shown)].tobytes() == shown, f"{label}: the published bytes of frame {n} are not its result's"
        assert not dsts[n].array[len(shown):].any(), f"{label}: frame {n}'s copy-out wrote beyond its result"


def lattice_pipeline(cm, steps, pinned, label):
    """The same order of calls over the lattices of tests/test_byproduct_reuse.py (steps 0..2) and the turned shapes
    ("shapes"): five_calls, the boxes and map_calls run between publish_async and the next frame."""
    points = [shapes_ref() if k == "shapes" else lattice_ref(k)[0] for k in steps]
    clouds = [xyzi_cloud(xyz, np.ones(len(xyz), F32)) for xyz in points]
    raws = [pinned.of(np.ascontiguousarray(c.data).view(np.uint8).reshape(-1)) for c in clouds]
    dsts = [pinned.zeros(32 * len(xyz)) for xyz in points]
    assert cm.submit_async(0, clouds[0], host_ptr=raws[0].ptr.value) == capi.OK
    published = []
    for n, k in enumerate(steps):
        what = f"{label}, frame {n} ({k})"
        leaf = SHAPES_LEAF if k == "shapes" else bu.LATTICE_LEAF
        assert cm.merge_voxelize_async(capi.make_params(MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=1 if k == "shapes" else 0))) == capi.OK
        res = cm.wait()
        step = 16 if n % 2 == 0 else 32
        shown = cm.result(res.n_out, step).tobytes()
        cm.publish_async(dsts[n].ptr.value, res.n_out, step)
        if n + 1 < len(steps):
            assert cm.submit_async(0, clouds[n + 1], host_ptr=raws[n + 1].ptr.value) == capi.OK
        published.append(shown)
        if k == "shapes":
            check_shapes(cm, res, what)
        else:
            check_lattice(cm, res, k, what)
    cm.publish_wait()
    for n, shown in enumerate(published):
        assert dsts[n].array[:len(shown)].tobytes() == shown, f"{label}: the published bytes of frame {n} are not its result's"
