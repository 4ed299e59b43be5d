"""The calls that read the last frame's raw clouds in place, long after the frame has finished (cm_result_grid_map, cm_result_grid_rays,
cm_map_integrate, cm_map_match_evaluate, cm_map_match_search, cm_map_mcl_update; cm_merged_copy reads the same descriptor), on
every wire layout of tests/layouts.py and after calls that build a descriptor without producing a frame.

Every comparison is of bytes: all outputs are integers or exact fp32 images. The expected values come from the restatements
(grid_ref, rays_ref, map_ref, cost_ref, match_ref, match_search_ref, mcl_ref) fed with tests/frame_host.py's fused cloud, which
tests/test_frame_host.py holds against the oracle; cm.merged() is itself compared with it and is never an expected value's
source. Every other layout, the mixed frames, the frames with a stage on and the device-submitted clouds must then give the
bytes the XYZI16 frame gives.

The frame: six sensors of 4096 + 37, 0, 1, 4096, 2 * 4096 + 1 and 63 points (CM_TILE is 4096: a tile edge, an empty sensor in
the middle, a single point, a sub-wave sensor and a sensor over three tiles), each with its own rotation and translation, a room
of walls, poles and flat patches within 12 m, and by hand NaN and infinite coordinates, a NaN intensity, -0.0 coordinates and
points outside the crop box beside counted cells. The grid and the map window are 64 x 48 cells of 0.5 m: one and a half
CM_MATCH_TILE (32) in y, two bitmap words per row."""
import ctypes as C

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from tests import cost_ref as cr
from tests import frame_host as fh
from tests import grid_ref as gr
from tests import layouts as wl
from tests import map_ref as mpr
from tests import match_ref as mf
from tests import match_search_ref as ms
from tests import mcl_ref as mr
from tests import motion_ref as mo
from tests import rays_ref as rr
from tests import test_grid_map as tg
from tests import test_layouts as tl
from tests import test_map_match as tmm
from tests import test_map_match_search as tms
from tests import test_map_mcl as tmc
from tests import test_occupancy_map as tm

pytestmark = pytest.mark.gpu

F32 = np.float32
COUNTS = [4096 + 37, 0, 1, 4096, 2 * 4096 + 1, 63]
N_CAP = sum(COUNTS)
CROP = dict(crop_min=(-12.0, -11.0, -1.0), crop_max=(12.0, 11.0, 3.0))
PARAMS = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, **CROP)
CELL, NX, NY = 0.5, 64, 48
ORIGIN = (-16.0, -12.0)
BAND = (-0.5, 1.9)                                     # (some points of every kind lie above it)
GRID = (ORIGIN, CELL, NX, NY, BAND, 0.3, 2)            # obstacle_height 0.3, min_points 2
MQ = mpr.params(CELL, NX, NY, z_band=BAND)
MATCH_Q = mf.params(sigma=0.5, max_dist=1.0, n_a=2, a_stride=8, wx=3, wy=2)
SEARCH_Q = ms.params(sigma=0.5, max_dist=1.0, n_a=2, a_stride=8, wx=3, wy=2, depth=1)
MCL_Q = mr.params(n_particles=48, max_beams=64, range_cells=30, sigma=0.5, max_dist=1.0, tau=8.0, resample_frac=0.5, flags=0, seed=5)
MCL_INIT = (0.25, -0.25, 0.05, 0.3, 0.3, 0.1)
MCL_MOVE = (0.1, -0.05, 0.02, 0.05, 0.05, 0.01)
PRIOR = np.eye(3, 4, dtype=F32)
# translations: five inside the grid (rays are cast from them), the single point's sensor outside it
TRANSLATIONS = [(1.5, -0.25, 0.5), (-3.0, 2.0, 0.2), (20.0, 1.0, 0.3), (-5.5, -4.0, 0.0), (4.25, 5.5, 0.75), (0.0, 0.0, -0.0)]
YAWS = [0.0, 0.6, -1.1, 2.3, -2.9, 0.2]
TILTS = [(0.0, 0.0), (0.02, -0.01), (0.0, 0.03), (-0.015, 0.0), (0.01, 0.01), (0.0, 0.0)]
NAN_PAYLOAD = 0x7FC00ABC
# hand-placed world points outside the crop box, inside the grid, beside wall cells that are counted
OUTSIDE = [(12.1, 1.0, 0.5), (-12.2, -2.0, 0.4), (3.0, 11.2, 0.6), (2.0, 2.0, 3.2)]
COST_ARGS = (0.0, 1.0, 3.0, False)                     # cm_map_cost_configure's arguments


def parameter_set(grid=GRID, mq=MQ, match=MATCH_Q, search=SEARCH_Q, mcl=MCL_Q, cost=COST_ARGS):
    """What by_products() configures and restated() restates; the defaults are the module's constants."""
    return dict(grid=grid, mq=mq, match=match, search=search, mcl=mcl, cost=cost)


def pose_of(s):
    rx, ry = TILTS[s]
    q = np.array([rx, ry, np.sin(YAWS[s] / 2), np.cos(YAWS[s] / 2)])
    return tuple((q / np.linalg.norm(q)).tolist()), TRANSLATIONS[s]


def world_points(rng, n):
    """n points of the room: walls on an outline with gaps and an inner L, poles, flat patches."""
    kind = rng.choice(3, n, p=[0.6, 0.2, 0.2])
    t = rng.uniform(0.0, 1.0, n)
    side = rng.integers(0, 6, n)
    wx = np.select([side == 0, side == 1, side == 2, side == 3, side == 4], [-11.0 + 22.0 * t, 11.8 + 0 * t, -11.0 + 17.0 * t, -11.8 + 0 * t, -4.0 + 6.0 * t],
                   default=2.0 + 0 * t)
    wy = np.select([side == 0, side == 1, side == 2, side == 3, side == 4], [-10.8 + 0 * t, -9.0 + 18.0 * t, 10.8 + 0 * t, -7.0 + 12.0 * t, 3.3 + 0 * t],
                   default=-6.0 + 9.3 * t)
    poles = np.random.default_rng(99).uniform(-10.0, 10.0, (30, 2))
    pk = rng.integers(0, 30, n)
    patch = np.array([(-7.0, -5.0), (6.0, -3.0), (7.5, 7.0), (-6.0, 6.5)])[rng.integers(0, 4, n)] + rng.uniform(0.0, 2.0, (n, 2))
    x = np.select([kind == 0, kind == 1], [wx + rng.uniform(0, 0.05, n), poles[pk, 0] + rng.uniform(0, 0.04, n)], default=patch[:, 0])
    y = np.select([kind == 0, kind == 1], [wy + rng.uniform(0, 0.05, n), poles[pk, 1] + rng.uniform(0, 0.04, n)], default=patch[:, 1])
    z = np.where(kind == 2, rng.uniform(0.0, 0.05, n), rng.uniform(0.1, 2.2, n))
    return np.stack([x, y, z], axis=1)


def base_scene(seed, shift=(0.0, 0.0, 0.0), counts=COUNTS):
    """Per sensor (xyz, intensity) in the sensor's own frame, float32, the hand-placed values in it; and what was placed:
    per sensor the indices that must be dropped."""
    rng = np.random.default_rng(seed)
    parts, dropped = [], []
    for s, n in enumerate(counts):
        q, t = pose_of(s)
        m = fh.matrix_of(q, t).astype(np.float64)
        w = world_points(rng, n) + np.asarray(shift)
        drop = []
        if n > 100:
            w[20:20 + len(OUTSIDE)] = OUTSIDE
            drop += list(range(20, 20 + len(OUTSIDE)))
        local = ((w - m[:, 3]) @ m[:, :3]).astype(F32)             # R^T (w - t)
        inten = rng.uniform(0.0, 255.0, n).astype(F32)
        if n > 100:
            local[3, 0] = np.nan
            local[5, 1] = np.inf
            local[7, 2] = -np.inf
            local[4097 % n] = (np.nan, np.nan, np.nan)             # (the first point of the second tile where there is one)
            drop += [3, 5, 7, 4097 % n]
            local[9] = (-0.0, -0.0, -0.0)                          # a valid point: the sensor's own position
            local[11, 1] = -0.0
            inten[13] = np.uint32(NAN_PAYLOAD).view(F32)
            inten[15] = -0.0
        elif n > 10:
            local[n - 1, 2] = np.nan                               # the last point of the sub-wave sensor
            drop += [n - 1]
        parts.append((local, inten))
        dropped.append(sorted(set(drop)))
    return parts, dropped


def clouds_in(parts, names, seed=0, taus=None):
    """The parts as SensorClouds, sensor s in layout names[s] (decoys in every byte that is no field)."""
    out = []
    for s, ((xyz, inten), name) in enumerate(zip(parts, names)):
        rng = np.random.default_rng(1000 * seed + 31 * s + sum(map(ord, name)))
        q, t = pose_of(s)
        out.append(wl.repack(xyz, inten, name, rng, tau=None if taus is None else taus[s], q_xyzw=q, t_xyz=t))
    return out


def zeroed(parts, which):
    """The parts with intensity 0 on the sensors `which` marks: what layouts without the field must give."""
    return [(xyz, np.zeros_like(inten) if z else inten) for (xyz, inten), z in zip(parts, which)]


# ---- everything the wrapper can copy out, in the order of the calls ------------------------------------------------------------
def struct_bytes(s):
    return bytes(s)


def by_products(cm, n_cap=N_CAP, pset=None):
    """grid_map, grid_rays, map_configure + map_integrate, map_cost_update, map_match, map_match_search and a seeded
    map_mcl_init_pose / predict / update on the context's last frame. Returns {name: bytes}. pset: a parameter_set()."""
    pset = pset or parameter_set()
    GRID, MQ, MATCH_Q, SEARCH_Q, MCL_Q = (pset[k] for k in ("grid", "mq", "match", "search", "mcl"))
    out = {}
    out["merged"] = cm.merged(n_cap).tobytes()
    out["grid"] = cm.grid_map(*GRID).tobytes()
    out["grid_image"] = cm.grid_occupancy().tobytes()
    out["rays"] = cm.grid_rays(*GRID, 1, 0).tobytes()
    out["rays_image"] = cm.grid_ray_occupancy().tobytes()
    out["rays_grid_image"] = cm.grid_occupancy().tobytes()
    tm.configure(cm, MQ)
    info = cm.map_integrate(None)
    table, image, dev = tm.read_map(cm, info)
    assert dev.tobytes() == table.tobytes()
    out["map"], out["map_image"], out["map_info"] = table.tobytes(), image.tobytes(), repr(tm.info_tuple(info)).encode()
    cm.map_cost_configure(*pset["cost"])
    cm.map_cost_update()
    cost, dist2, _ = cm.map_cost()
    out["cost"], out["dist2"] = cost.tobytes(), dist2.tobytes()
    tmm.configure_match(cm, MATCH_Q)
    res = cm.map_match(PRIOR)
    vol, r1 = cm.map_match_scores()
    assert bytes(res) == bytes(r1)
    out["match_volume"], out["match_result"] = vol.tobytes(), struct_bytes(res)
    tms.configure_search(cm, SEARCH_Q)
    sres, sinfo = cm.map_match_search(PRIOR)
    out["search_result"], out["search_info"] = struct_bytes(sres), struct_bytes(sinfo)
    q = MCL_Q
    cm.map_mcl_configure(q["n_particles"], q["max_beams"], q["range_cells"], q["sigma"], q["max_dist"], q["tau"], q["resample_frac"],
                         bool(q["flags"] & 1), q["seed"])
    cm.map_mcl_init_pose(*MCL_INIT)
    out["mcl_init"] = cm.map_mcl_particles().tobytes()
    cm.map_mcl_predict(*MCL_MOVE)
    out["mcl_predict"] = cm.map_mcl_particles().tobytes()
    minfo = cm.map_mcl_update()
    w, i1 = cm.map_mcl_weights()
    assert bytes(minfo) == bytes(i1)
    out["mcl_particles"], out["mcl_weights"], out["mcl_info"] = cm.map_mcl_particles().tobytes(), w.tobytes(), struct_bytes(minfo)
    return out


def same_outputs(got, want, label):
    assert list(got) == list(want)
    bad = [k for k in want if got[k] != want[k]]
    if bad:
        k = bad[0]
        a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
        where = np.flatnonzero(a != b) if len(a) == len(b) else []
        raise AssertionError(f"{label}: {bad} differ; {k}: {len(a)} bytes against {len(b)}, {len(where)} differ, first at byte "
                             f"{where[0] if len(where) else '-'}: got {a[where[:8]].tolist() if len(where) else ''} want {b[where[:8]].tolist() if len(where) else ''}")


def run_frame(cm, clouds, params=PARAMS):
    cm.submit_all(clouds)
    res = cm.merge_voxelize(params)
    assert res.status == capi.OK, capi.status_string(res.status)
    return res


def frame_outputs(clouds, params=PARAMS, prepare=None, n_cap=N_CAP):
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=len(clouds)) as cm:
        if prepare:
            prepare(cm)
        res = run_frame(cm, clouds, params)
        out = by_products(cm, n_cap)
        out["result"] = cm.result(res.n_out).tobytes()
        return out, res


# ---- the restatements, fed from frame_host -----------------------------------------------------------------------------------
_tab = []


def TAB():
    if not _tab:
        _tab.append(capi.traj_directions())
    return _tab[0]


def restated(frame, dropped=None, guard=True, pset=None, counts=COUNTS):
    """{name: bytes} of by_products()' outputs that a restatement defines, from a frame_host frame alone. The vacuity guards are
    conditions on this reference: they are checked here, before any device output is looked at. pset: a parameter_set();
    counts: the points per sensor the scene was made with."""
    pset = pset or parameter_set()
    GRID, MQ, MATCH_Q, SEARCH_Q, MCL_Q = (pset[k] for k in ("grid", "mq", "match", "search", "mcl"))
    A, tag = frame.A, frame.sensor
    NO_G = np.zeros((0, 4), F32)
    origin, cell, nx, ny, band, height, min_points = GRID
    want = {"merged": A.view(np.uint32).tobytes()}
    grid, image = gr.grid_vectorised(A, NO_G, origin, cell, nx, ny, band, height, min_points)
    want["grid"], want["grid_image"] = grid.tobytes(), image.tobytes()
    rays, cleared, rinfo = rr.rays_vectorised(A, NO_G, tag, np.zeros(0, np.int64), [t[:2] for t in frame.translations], origin, cell, nx, ny,
                                              band, height, min_points, 1, 0)
    want["rays"], want["rays_image"], want["rays_grid_image"] = rays.tobytes(), cleared.tobytes(), rinfo["base_image"].tobytes()
    table, mimage, minfo = mpr.MapVectorised(MQ).integrate(A, NO_G, tag, np.zeros(0, np.int64), frame.translations, PRIOR)
    want["map"], want["map_image"], want["map_info"] = table.tobytes(), mimage.tobytes(), repr(tm.want_info(minfo)).encode()
    dist2 = cr.dist2_separable(mimage)
    want["dist2"] = dist2.astype(np.uint32).tobytes()
    anchor = minfo["anchor"]
    vol, mres = mf.match(A, dist2, MQ, anchor, MATCH_Q, PRIOR, TAB())
    want["match_volume"] = vol.tobytes()
    status, sres, sinfo, _ = ms.match(A, dist2, MQ, anchor, SEARCH_Q, PRIOR, TAB())
    assert status == "ok"
    f = mr.Filter(MCL_Q, MQ, TAB())
    f.init_pose(*MCL_INIT)
    want["mcl_init"] = f.parts.tobytes()
    f.predict(*MCL_MOVE)
    want["mcl_predict"] = f.parts.tobytes()
    wtable, winfo = f.update(A, dist2, anchor)
    want["mcl_particles"], want["mcl_weights"] = f.parts.tobytes(), wtable.tobytes()
    structs = dict(match_result=mres, search_result=sres, search_info=sinfo, mcl_info=winfo)
    if guard:
        ends = rr.ray_set(A, NO_G, tag, np.zeros(0, np.int64), len(frame.translations), origin, cell, nx, ny, band)
        for s, e in enumerate(ends):
            assert (len(e) > 0) == ((tag == s).any()), f"sensor {s} contributes no counted cell"
        assert set(grid["state"].ravel().tolist()) == {gr.UNKNOWN, gr.FREE, gr.OCCUPIED}
        assert set(cleared.ravel().tolist()) == {-1, 0, 100} and rinfo["two_sensors"] > 0 and rinfo["n_rays"] > 100
        assert set(mimage.ravel().tolist()) == {-1, 0, 100} and minfo["sensors_cast"] not in (0, (1 << len(frame.translations)) - 1)
        assert (vol == vol.max()).sum() == 1 and vol.max() > 0, "the match volume has no unique maximum"
        assert winfo["n_beams"] > 8 and len(set(wtable["score"].tolist())) > 8
        # (i_max is the largest finite intensity of a cell: a NaN beside finite values must not show in it)
        nan_i = A[:, 3].view(np.uint32) == NAN_PAYLOAD
        nan_cells, nan_ok = gr.cells_of(A[nan_i], origin, cell, nx, ny, *band)
        assert nan_i.sum() >= 3 and nan_ok.any() and not np.isnan(grid["i_max"].ravel()[nan_cells]).any(), "no counted point has the NaN intensity"
    if guard and dropped is not None:
        # a hand-placed point outside the crop box: inside the grid, its 3 x 3 neighbourhood holds counted points, and it is
        # not in the frame (its own cell would count one point more)
        near = 0
        for p in OUTSIDE[:3]:
            idx, ok = gr.cells_of(F32([list(p) + [0.0]]), origin, cell, nx, ny, -np.inf, np.inf)
            assert ok.all()
            ix, iy = int(idx[0]) % nx, int(idx[0]) // nx
            near += int(grid["n"][max(iy - 1, 0):iy + 2, max(ix - 1, 0):ix + 2].sum() > 0)
        assert near >= 1, "no dropped point lies beside a counted cell"
        for s, d in enumerate(dropped):
            assert not set(d) & set(frame.index[tag == s].tolist()), f"sensor {s}: a hand-placed value was not dropped"
            assert d == [] or (tag == s).sum() == counts[s] - len(d)
    return want, structs


def check_structs(out_structs, structs):
    res, sres, sinfo, minfo = out_structs
    assert tmm.same_result(tmm.result_dict(res), structs["match_result"]), (tmm.result_dict(res), structs["match_result"])
    assert tmm.same_result(tmm.result_dict(sres), structs["search_result"])
    assert tms.info_dict(sinfo) == structs["search_info"], (tms.info_dict(sinfo), structs["search_info"])
    tmc.same_info(minfo, structs["mcl_info"])


def against_restatement(out, want, label):
    for k, v in want.items():
        if out[k] != v:
            a, b = np.frombuffer(out[k], np.uint8), np.frombuffer(v, np.uint8)
            n = int((a != b).sum()) if len(a) == len(b) else -1
            raise AssertionError(f"{label}: {k} differs from the restatement: {len(a)} bytes against {len(b)}, {n} differ")


def structs_of(out):
    return (capi.MatchResult.from_buffer_copy(out["match_result"]), capi.MatchResult.from_buffer_copy(out["search_result"]),
            capi.MatchSearchInfo.from_buffer_copy(out["search_info"]), capi.MclInfo.from_buffer_copy(out["mcl_info"]))


# ---- the XYZI16 baseline ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    parts, dropped = base_scene(41)
    return parts, dropped


@pytest.fixture(scope="module")
def baseline(scene):
    """The XYZI16 frame's outputs, with the intensities and with zeros."""
    parts, _ = scene
    full, _ = frame_outputs(clouds_in(parts, ["xyzi16"] * 6))
    zero, _ = frame_outputs(clouds_in(zeroed(parts, [True] * 6), ["xyzi16"] * 6))
    assert full["grid"] != zero["grid"] and full["rays"] == zero["rays"]
    return full, zero


def test_xyzi16_baseline_against_the_restatements(scene, baseline):
    parts, dropped = scene
    frame = fh.fuse(clouds_in(parts, ["xyzi16"] * 6), PARAMS.crop_min, PARAMS.crop_max)
    want, structs = restated(frame, dropped)
    print(f"frame: {frame.n_in} points, {len(frame.A)} valid; grid states {np.bincount(np.frombuffer(want['grid_image'], np.int8).astype(int) + 1, minlength=102)[[0, 1, 101]].tolist()}; "
          f"match best {structs['match_result']['best']} score {structs['match_result']['score']}; mcl beams {structs['mcl_info']['n_beams']}")
    against_restatement(baseline[0], want, "xyzi16")
    check_structs(structs_of(baseline[0]), structs)


# ---- every layout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [k for k in wl.ALL if k != "xyzi16"])
def test_uniform_layouts(scene, baseline, layout):
    parts, _ = scene
    clouds = clouds_in(parts, [layout] * 6, seed=1)
    assert all(c.point_step == wl.ALL[layout].step for c in clouds)
    got, _ = frame_outputs(clouds)
    same_outputs(got, baseline[1 if layout in wl.NO_INTENSITY else 0], layout)


# MIXED of tests/test_layouts.py, six of its entries in the order of the sensors, and one of its 16-byte layouts beside XYZI16:
# PCL32 and the generic 32-byte pcl32_i12 on the two large one-tile sensors, two 16-byte layouts with different offsets.
MIXED6 = [tl.MIXED[0], tl.MIXED[1], tl.MIXED[6], tl.MIXED[7], tl.MIXED[4], tl.STEP16[1]]


def test_mixed_names_are_what_the_comment_says():
    assert MIXED6 == ["pcl32", "velo22", "tail", "pcl32_i12", "xyzi16", "zyx_i16"]
    L = wl.ALL
    assert L["pcl32"].fast == "PCL32" and L["pcl32_i12"].fast == "GENERIC" and L["pcl32_i12"].step == 32
    assert L["xyzi16"].step == L["zyx_i16"].step == 16 and L["xyzi16"].off != L["zyx_i16"].off


def test_mixed_layouts(scene, baseline):
    parts, _ = scene
    got, _ = frame_outputs(clouds_in(parts, MIXED6, seed=2))
    same_outputs(got, baseline[0], "mixed")


FRONT = [(4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]


def test_mixed_layouts_with_ground_removal(scene):
    """The ground mask and the ground points' sensors (sensor_g) behind mixed layouts: the bytes of the XYZI16 frame."""
    parts, _ = scene

    def prepare(cm):
        cm.set_ground_removal(capi.make_ground_params([FRONT] * 6))

    want, _ = frame_outputs(clouds_in(parts, ["xyzi16"] * 6), prepare=prepare)
    got, _ = frame_outputs(clouds_in(parts, MIXED6, seed=3), prepare=prepare)
    with capi.CloudMerger(max_points_total=N_CAP, max_sensors=6) as cm:
        prepare(cm)
        run_frame(cm, clouds_in(parts, MIXED6, seed=3))
        n_ground = len(cm.ground(N_CAP))
        grid = cm.grid_map(*GRID)
    assert n_ground > 100 and (grid["n_ground"] > 0).any(), "the frame has no ground points"
    same_outputs(got, want, "mixed + ground")


def test_mixed_layouts_with_the_outlier_stage(scene, baseline):
    """The keep mask behind mixed layouts."""
    parts, _ = scene

    def prepare(cm):
        cm.set_statistical_outlier(8, 0.5)

    want, res = frame_outputs(clouds_in(parts, ["xyzi16"] * 6), prepare=prepare)
    got, _ = frame_outputs(clouds_in(parts, MIXED6, seed=4), prepare=prepare)
    assert res.path_flags & capi.PATH_SOR and len(want["merged"]) < len(baseline[0]["merged"]), "the stage removed nothing"
    assert want["grid"] != baseline[0]["grid"]
    same_outputs(got, want, "mixed + outlier stage")


# ---- deskew: the descriptor points at the motion buffer ---------------------------------------------------------------------------
T_REF = 1_700_000_000_000_000_000
V, W = (6.0, -4.0, 0.0), (0.0, 0.0, 0.05)
TIMED6 = ["odd17_t", "livox18_t"] * 3


def test_deskew_with_timed_layouts(scene):
    parts, _ = scene
    rng = np.random.default_rng(8)
    stamps = [T_REF + int(d) for d in rng.integers(-40_000_000, 40_000_001, 6)]
    taus = [rng.uniform(0.0, 0.1, n).astype(F32) if wl.TIMED[name].time[1] == wl.TIME_F32_S else rng.integers(0, 100_000_000, n).astype(np.uint32)
            for n, name in zip(COUNTS, TIMED6)]
    clouds = clouds_in(parts, TIMED6, seed=5, taus=taus)
    motions = [(mo.time_of(tau, wl.TIMED[name].time[1]), mo.dt0_s(stamp, T_REF), V, W) for tau, name, stamp in zip(taus, TIMED6, stamps)]
    frame = fh.fuse(clouds, PARAMS.crop_min, PARAMS.crop_max, motions)
    plain = fh.fuse(clouds, PARAMS.crop_min, PARAMS.crop_max)
    # (the points move by up to 0.8 m: some leave the crop box, others stay only because they moved)
    assert 12000 < len(frame.A) < len(plain.A) and not np.array_equal(frame.A[:100, :3], plain.A[:100, :3])
    want, structs = restated(frame, guard=False)

    def prepare(cm):
        for s, name in enumerate(TIMED6):
            cm.set_time_field(s, *wl.TIMED[name].time)
        cm.set_ego_motion(capi.make_motion(V, W, T_REF, stamps))

    got, res = frame_outputs(clouds, prepare=prepare)
    assert res.path_flags & capi.PATH_MOTION
    against_restatement(got, want, "deskew")
    check_structs(structs_of(got), structs)


# ---- device-submitted clouds at addresses that are not 16-byte aligned -----------------------------------------------------------
@pytest.mark.parametrize("layout", ["xyzi16", "pcl32"])
def test_device_clouds_at_4_byte_alignment(scene, baseline, layout):
    """XYZI16 or PCL32 bytes at byte offsets 4, 8, 12 and 0 of 256-byte slots of one device buffer: only the last may take the
    fast loader. The by-products are those of the host-submitted frame."""
    parts, _ = scene
    clouds = clouds_in(parts, [layout] * 6, seed=6)
    hip = tg.hip_rt()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    offsets = [4, 8, 12, 12, 8, 0]
    spans = [(c.n * c.point_step + 511) // 256 * 256 for c in clouds]
    starts = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(int)
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), int(sum(spans))) == 0
    try:
        for s, c in enumerate(clouds):
            data = np.ascontiguousarray(c.data)
            assert int(starts[s]) + offsets[s] + data.nbytes <= int(starts[s]) + spans[s]
            if data.nbytes:
                assert hip.hipMemcpy(buf.value + int(starts[s]) + offsets[s], data.ctypes.data, data.nbytes, 1) == 0
        with capi.CloudMerger(max_points_total=N_CAP, max_sensors=6) as cm:
            for s, c in enumerate(clouds):
                cm.set_transform(s, c.q_xyzw, c.t_xyz)
                ptr = buf.value + int(starts[s]) + offsets[s]
                assert ptr % 4 == 0 and (ptr % 16 == 0) == (offsets[s] == 0)
                cm.submit_device(s, ptr, c.n, c.point_step, c.off_x, c.off_y, c.off_z, c.off_i)
            res = cm.merge_voxelize(PARAMS)
            assert res.status == capi.OK
            got = by_products(cm)
            got["result"] = cm.result(res.n_out).tobytes()
    finally:
        hip.hipFree(buf)
    same_outputs(got, baseline[0], f"{layout} on the device")


# ---- the descriptor survives calls that produce no frame ----------------------------------------------------------------------------
# Two sensors, PCL32 and odd17, with the radius outlier stage on (cm_local_bounds refuses the statistical one), so the keep mask
# is not all ones. 8130 + 63 = 8193 points is also the context's max_points_total: each of two clouds of 8193 points fits it, and
# together they need 2 * 12288 padded slots, more than the 12288 + 2 * 4096 the context has: the merge is refused in build_frame.
# Every mask and bitmap the calls index is sized by the capacity (ensure_mask: cap_padded bytes; the ray, map, match and mcl
# bitmaps: max_sensors or the layer's own grid), and cloud N + 1 has frame N's counts and layouts: whichever clouds a call reads,
# every index stays inside what frame N allocated.
C_COUNTS = [8130, 63]
C_CAP = sum(C_COUNTS)
C_LAYOUTS = ["pcl32", "odd17"]
C_PARAMS = MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0, outlier_radius=0.3, outlier_min_neighbors=3, **CROP)


def c_clouds(seed, shift=(0.0, 0.0, 0.0), counts=C_COUNTS):
    parts, _ = base_scene(seed, shift, counts)
    return clouds_in(parts, C_LAYOUTS, seed=seed)


def frame_n_outputs(cm):
    """by_products() and what cm_result_copy serves."""
    out = by_products(cm, C_CAP)
    _, n = cm.result_device()
    out["result"] = cm.result(n).tobytes()
    return out


@pytest.fixture(scope="module")
def frames_n():
    """Frame N and frame N + 1 on a context that makes no other call: what every sequence below must reproduce."""
    with capi.CloudMerger(max_points_total=C_CAP, max_sensors=2) as cm:
        res = run_frame(cm, c_clouds(51), C_PARAMS)
        n = frame_n_outputs(cm)
        kept = len(n["merged"]) // 16
        assert 0 < kept < res.n_in - 8, "the outlier stage removed nothing: the keep mask is all ones"
        run_frame(cm, c_clouds(52, (1.5, -1.0, 0.0)), C_PARAMS)
        n1 = frame_n_outputs(cm)
    assert n["grid"] != n1["grid"] and n["map"] != n1["map"] and n["merged"] != n1["merged"]
    return n, n1


def test_a_peek_with_a_fresh_cloud_leaves_the_frame(frames_n):
    want_n, want_n1 = frames_n
    nxt = c_clouds(52, (1.5, -1.0, 0.0))
    with capi.CloudMerger(max_points_total=C_CAP, max_sensors=2) as cm:
        res = run_frame(cm, c_clouds(51), C_PARAMS)
        cm.submit_all(nxt)
        lo, hi, n_valid = cm.local_bounds(C_PARAMS)
        # the peek's own answer: the bounds of cloud N + 1
        mn, mx, cnt = fh.bounds(fh.fuse(nxt, C_PARAMS.crop_min, C_PARAMS.crop_max))
        assert lo.tobytes() == mn.tobytes() and hi.tobytes() == mx.tobytes() and n_valid == cnt
        # every by-product, the fused cloud and the result are frame N's
        same_outputs(frame_n_outputs(cm), want_n, "after the peek")
        assert cm.frame_stats()["n_in"] == C_COUNTS and res.n_in == C_CAP
        # a second peek straight after a by-product call, then the merge: frame N + 1, whatever HBM held in between
        assert cm.local_bounds(C_PARAMS)[2] == cnt
        res = cm.merge_voxelize(C_PARAMS)
        assert res.status == capi.OK
        same_outputs(frame_n_outputs(cm), want_n1, "frame N + 1 after the peeks")


def test_a_peek_then_a_merge_with_no_call_in_between(frames_n):
    """The descriptor cache: the peek uploaded cloud N + 1's descriptor, the merge builds its own."""
    _, want_n1 = frames_n
    with capi.CloudMerger(max_points_total=C_CAP, max_sensors=2) as cm:
        run_frame(cm, c_clouds(51), C_PARAMS)
        cm.submit_all(c_clouds(52, (1.5, -1.0, 0.0)))
        cm.local_bounds(C_PARAMS)
        assert cm.merge_voxelize(C_PARAMS).status == capi.OK
        same_outputs(frame_n_outputs(cm), want_n1, "frame N + 1 straight after the peek")


def test_a_peek_that_finds_nothing_new_or_only_empty_clouds(frames_n):
    want_n, _ = frames_n
    empty = c_clouds(53, counts=[0, 0])
    with capi.CloudMerger(max_points_total=C_CAP, max_sensors=2) as cm:
        run_frame(cm, c_clouds(51), C_PARAMS)
        with pytest.raises(capi.CloudMergeError) as e:
            cm.local_bounds(C_PARAMS)
        assert e.value.status == capi.NOT_READY
        same_outputs(frame_n_outputs(cm), want_n, "after a peek that was not ready")
        cm.submit_all(empty)
        lo, hi, n_valid = cm.local_bounds(C_PARAMS)
        assert n_valid == 0 and np.isinf(lo).all() and np.isinf(hi).all()
        same_outputs(frame_n_outputs(cm), want_n, "after a peek over empty clouds")
        assert cm.merge_voxelize(C_PARAMS).status == capi.EMPTY_INPUT


def test_a_merge_refused_for_capacity_leaves_the_frame(frames_n):
    want_n, want_n1 = frames_n
    with capi.CloudMerger(max_points_total=C_CAP, max_sensors=2) as cm:
        run_frame(cm, c_clouds(51), C_PARAMS)
        # (cm_submit_cloud takes each cloud: 8193 points are the context's limit. The frame of both is what does not fit.)
        cm.submit_all(c_clouds(54, counts=[C_CAP, C_CAP]))
        with pytest.raises(capi.CloudMergeError) as e:
            cm.merge_voxelize(C_PARAMS)
        assert e.value.status == capi.CAPACITY
        same_outputs(frame_n_outputs(cm), want_n, "after the refused merge")
        assert cm.frame_stats()["n_in"] == C_COUNTS
        # the context goes on: clear the clouds that do not fit, then frame N + 1
        cm.clear(0)
        cm.clear(1)
        run_frame(cm, c_clouds(52, (1.5, -1.0, 0.0)), C_PARAMS)
        same_outputs(frame_n_outputs(cm), want_n1, "frame N + 1 after the refused merge")
