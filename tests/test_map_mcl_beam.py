"""The beam model of the localisation layer: cm_map_mcl_beam_configure, cm_map_mcl_beam_info_copy, cm_mcl_beam_table
(include/cloudmerge.h, k_mcl_beam in cm_kernels_mcl.hip).

The bar on the GPU is the localisation layer's: every byte of the particles, of the weight table, of the device-pointer variant
and every field of both infos equal to the restatement (tests/mcl_beam_ref.py, which walks cell by cell through the image), in
both walk modes. There is no tolerance. What the model is for, a pose whose beams pass through a wall, is shown on the
restatement on the CPU first; the byte equality on the GPU carries it over."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from cloud_merger_amd import capi
from tests import cast_ref as kr
from tests import cost_ref as cr
from tests import mcl_beam_ref as br
from tests import mcl_ref as mr
from tests import map_ref as mpr
from tests import match_ref as mf
from tests import test_grid_map as tg
from tests import test_map_cast as tcs
from tests import test_map_match as tmm
from tests import test_map_mcl as tml
from tests import test_occupancy_map as tm
from tests import traj_ref as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
NAMES = ("cm_map_mcl_beam_configure", "cm_map_mcl_beam_info_copy", "cm_mcl_beam_table")
BEAM_TYPES = (capi.MclBeamParams, capi.MclBeamInfo)  # (a library without the mode fails every test here, at import)
F32 = np.float32
CELL, NX, NY, MQ, ANCHOR = tml.CELL, tml.NX, tml.NY, tml.MQ, tml.ANCHOR
TAB = tml.TAB


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_beam_structs_and_constants_match_header(tmp_path):
    structs = {"cm_mcl_beam_params": capi.MclBeamParams, "cm_mcl_beam_info": capi.MclBeamInfo}
    names = ["CM_MCL_BEAM_MAX_OVER", "CM_MCL_BEAM_MAX_D", "CM_MCL_BEAM_PLAIN"]
    items, want = [], []
    for s, T in structs.items():
        fields = [f for f, _ in T._fields_]
        items += [f"sizeof({s})"] + [f"offsetof({s},{f})" for f in fields]
        want += [C.sizeof(T)] + [getattr(T, f).offset for f in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%llu ",(unsigned long long)({it}));' for it in items + names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:len(want)] == want == [24, 0, 4, 8, 12, 16, 20, 56, 0, 8, 16, 24, 32, 40, 48]
    assert got[len(want):] == [capi.MCL_BEAM_MAX_OVER, capi.MCL_BEAM_MAX_D, capi.MCL_BEAM_PLAIN] == [br.MAX_OVER, br.MAX_D, br.PLAIN] == [64, 1450, 1]
    assert tuple(f for f, _ in capi.MclBeamInfo._fields_[1:]) == br.COUNTS
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)
    # the layer's own structs and the layer table are what they were
    assert C.sizeof(capi.MclParams) == 40 and C.sizeof(capi.MclInfo) == 176


def test_null_context_calls_leave_their_outputs_untouched():
    L = capi.load()
    p = capi.MclBeamParams(8, 0.1, 0.75, 0.125, 0.125, 0)
    info = capi.MclBeamInfo(7, 7, 7, 7, 7, 7, 7)
    before = bytes(info)
    assert L.cm_map_mcl_beam_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_mcl_beam_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_mcl_beam_info_copy(None, C.byref(info)) == capi.BAD_ARG and bytes(info) == before


def b_of(**kw):
    return dict(br.params(), **kw)


def lib_table(b, cell=CELL):
    return capi.mcl_beam_table(cell, b["over_cells"], b["sigma"], b["z_hit"], b["z_short"], b["z_rand"], bool(b["flags"] & 1))


TABLES = [b_of(), b_of(over_cells=0), b_of(over_cells=64), b_of(over_cells=64, sigma=0.7), b_of(z_hit=1.0, z_short=0.0, z_rand=0.0),
          b_of(z_hit=0.5, z_short=0.25, z_rand=0.25), b_of(z_hit=0.75, z_short=0.125, z_rand=0.125, over_cells=3), b_of(sigma=1e-3),
          b_of(sigma=1e-30, over_cells=5), b_of(sigma=0.05, z_hit=0.3, z_short=0.0, z_rand=0.01), b_of(sigma=3.0, z_hit=0.001, over_cells=64),
          b_of(z_hit=0.5, z_short=0.5, z_rand=0.0, flags=1), b_of(sigma=1e30, over_cells=64)]


@pytest.mark.parametrize("k", range(len(TABLES)))
def test_the_table_against_the_restatement(k):
    b = TABLES[k]
    for cell in (CELL, 0.05, 1.0):
        got, want = lib_table(b, cell), br.table(b, cell)
        assert got.dtype == np.uint8 and len(got) == 2 * b["over_cells"] + 3 and got.tobytes() == want.tobytes(), (b, cell, got, want)
        E = b["over_cells"]
        assert got[E] == got[:E + 1].max()             # among the early entries the hit term peaks at the measured end
        assert got[2 * E + 1] == round(255 * (float(F32(b["z_short"])) + float(F32(b["z_rand"])))) and got[2 * E + 2] == round(255 * float(F32(b["z_rand"])))


def test_the_table_by_hand_and_its_refusals():
    # sums of exactly 1: the end byte is 255 * (z_hit + z_rand) early, and saturates at 255 late
    assert lib_table(b_of(over_cells=1, sigma=1e-3, z_hit=0.5, z_short=0.25, z_rand=0.25)).tolist() == [64, 191, 128, 128, 64]
    assert lib_table(b_of(over_cells=0, z_hit=1.0, z_short=0.0, z_rand=0.0)).tolist() == [255, 0, 0]
    # a sigma so small that only e == 0 is above the floor
    t = lib_table(b_of(over_cells=5, sigma=1e-30, z_hit=0.5, z_short=0.125, z_rand=0.125))
    assert t.tolist() == [32] * 5 + [159] + [64] * 5 + [64, 32]          # 31.875 -> 32, 159.375 -> 159, 63.75 -> 64
    # ties go to even: 255 * 0.5 = 127.5 -> 128, 255 * 0.1 (as fp32) is above 25.5
    assert lib_table(b_of(over_cells=0, z_hit=0.5, z_short=0.5, z_rand=0.0))[1] == 128
    L = capi.load()
    buf = np.full(8, 7, np.uint8)
    ok = capi.MclBeamParams(1, 0.1, 0.75, 0.125, 0.125, 0)
    assert L.cm_mcl_beam_table(C.byref(ok), CELL, buf.ctypes.data, 4) == capi.CAPACITY and (buf == 7).all()
    assert L.cm_mcl_beam_table(C.byref(ok), CELL, None, 8) == capi.BAD_ARG and L.cm_mcl_beam_table(None, CELL, buf.ctypes.data, 8) == capi.BAD_ARG
    for cell in (0.0, -1.0, np.nan, np.inf):
        assert L.cm_mcl_beam_table(C.byref(ok), cell, buf.ctypes.data, 8) == capi.BAD_ARG and (buf == 7).all()
    for kw in REFUSED_BEAMS:
        b = b_of(**kw)
        p = capi.MclBeamParams(b["over_cells"], b["sigma"], b["z_hit"], b["z_short"], b["z_rand"], b["flags"])
        assert L.cm_mcl_beam_table(C.byref(p), CELL, buf.ctypes.data, 8) == capi.BAD_ARG and (buf == 7).all(), kw
    assert L.cm_mcl_beam_table(C.byref(ok), CELL, buf.ctypes.data, 5) == capi.OK and (buf[5:] == 7).all()


REFUSED_BEAMS = [dict(over_cells=65), dict(over_cells=2 ** 31), dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=np.nan), dict(sigma=np.inf),
                 dict(z_hit=0.0), dict(z_hit=-0.5), dict(z_hit=np.nan), dict(z_hit=np.inf), dict(z_short=-0.01), dict(z_short=np.nan),
                 dict(z_rand=-0.01), dict(z_rand=np.inf), dict(z_hit=0.9, z_short=0.1, z_rand=0.1), dict(z_hit=1.0, z_short=0.0, z_rand=1e-6),
                 dict(flags=2), dict(flags=1 << 31)]
ACCEPTED_BEAMS = [dict(over_cells=0), dict(over_cells=64), dict(sigma=1e-30), dict(sigma=1e30), dict(z_hit=1.0, z_short=0.0, z_rand=0.0),
                  dict(z_hit=0.5, z_short=0.25, z_rand=0.25), dict(z_hit=1e-6, z_short=0.0, z_rand=0.0), dict(flags=1)]


def test_refusals_of_the_restatement():
    assert br.refusal(b_of(), CELL) is None
    for kw in REFUSED_BEAMS:
        assert br.refusal(b_of(**kw), CELL) is not None, kw
    for kw in ACCEPTED_BEAMS:
        assert br.refusal(b_of(**kw), CELL) is None, kw


# ---- CPU: the walks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tcs.small_windows()))
@pytest.mark.parametrize("E", [0, 1, 5])
def test_the_jump_walk_against_the_plain_walk_exhaustively(name, E):
    """Every origin of the window and every (dx, dy) with |d| <= 12, followed E steps past its end: the skip rule of §30 holds
    for arbitrary lines and past their end. The scalar walks on Python integers ride along on a sample."""
    image = tcs.small_windows()[name]
    ny, nx = image.shape
    steps = br.steps_of(kr.dist2_of(image))
    assert ((steps == 0) == (image == 100)).all()
    oy, ox, dy, dx = (v.reshape(-1) for v in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(-12, 13), np.arange(-12, 13), indexing="ij"))
    cls, idx, _ = br.walk_plain_many(image, ox, oy, dx, dy, E)              # (_: the cells the plain walk read)
    cls2, idx2, reads2 = br.walk_skip_many(steps, ox, oy, dx, dy, E)
    assert (cls == cls2).all() and (idx == idx2).all() and (reads2 <= np.maximum(_, 1)).all()
    zero = (dx == 0) & (dy == 0)
    assert (cls[zero] == np.where(image[oy[zero], ox[zero]] == 100, br.AT, br.BEYOND)).all()
    for i in np.random.default_rng(E).integers(0, len(ox), 300):
        a = br.walk_plain(image, int(ox[i]), int(oy[i]), int(dx[i]), int(dy[i]), E)
        b = br.walk_skip(steps, int(ox[i]), int(oy[i]), int(dx[i]), int(dy[i]), E)
        assert a[:2] == b[:2] == (int(cls[i]), int(idx[i])) and b[2] <= a[2]


@pytest.mark.parametrize("ulps", [-1, 0, 1])
def test_the_quotient_without_a_division_at_the_beam_bound(ulps):
    """cm_cast_math.hpp's quotient at the beam model's operands: lines of |d| <= 1450 followed 64 steps past their end, the
    largest operand 2 * 1514 * 1450 + 1450 = 4 392 050 < 2^24, with the reciprocal as rounded and one unit either side."""
    assert 2 * (br.MAX_D + br.MAX_OVER) * br.MAX_D + br.MAX_D == 4392050 < 1 << 24
    for L in list(range(1025, 1451, 5)) + [1447, 1448, 1449, 1450]:
        d = np.unique(np.concatenate([np.arange(0, L + 1, 29), [1, L - 1, L]]))
        k = np.unique(np.concatenate([np.arange(0, L + 65, 7), np.arange(L - 2, L + 65)]))
        K, D = np.meshgrid(k, d)
        assert (kr.minor_cell(K, D, L, ulps) == (2 * K * D + L) // (2 * L)).all(), L
    for L in (1450, 1031, 7, 1):                       # next to every multiple, where a rounding error could change the floor
        K, D = np.meshgrid(np.arange(L + 65), np.arange(L + 1))
        m = (2 * K * D + L) % (2 * L)
        near = (m <= 2) | (m >= 2 * L - 2)
        assert (kr.minor_cell(K[near], D[near], L, ulps) == (2 * K[near] * D[near] + L) // (2 * L)).all()
    # the last step inside: k <= ((2 m + 1) L - 1) div 2 am for m < am + 64
    rng = np.random.default_rng(ulps + 2)
    L = rng.integers(1, 1451, 20000)
    am = np.minimum(rng.integers(1, 1451, 20000), L)
    m = np.minimum(rng.integers(0, 1514, 20000), am + 63)
    n, d = (2 * m + 1) * L - 1, 2 * am
    rd = (F32(1.0) / d.astype(F32)).astype(F32)
    for _ in range(abs(ulps)):
        rd = np.nextafter(rd, F32(np.inf if ulps > 0 else -np.inf))
    assert n.max() < 1 << 24 and (kr.quot(n, d, rd) == n // d).all()


# ---- CPU: what the model is for ------------------------------------------------------------------------------------------------
def two_walls():
    """A corridor of 64 x 9 cells with walls at columns 25 and 45, everything else free."""
    img = np.zeros((9, 64), np.int8)
    img[:, 25] = img[:, 45] = 100
    return img


WALLS_MQ = mpr.params(CELL, 64, 9)
WALLS_ANCHOR = tmm.anchor_of(64, 9)
WALLS_BEAMS = [(25, -1), (25, 0), (25, 1)]            # three beams 25 cells ahead
WALLS_Q = dict(mr.params(), n_particles=2, max_beams=64, range_cells=64, sigma=0.1, max_dist=0.5, tau=8.0, resample_frac=0.0)
WALLS_B = b_of(over_cells=4, sigma=0.1)


def pose_in(ix, iy, anchor):
    """A point a quarter of a cell inside window cell (ix, iy): with heading 0 a beam of body cell b ends in cell (ix, iy) + b."""
    return ((anchor[0] + ix + 0.25) * CELL, (anchor[1] + iy + 0.25) * CELL)


def walls_particles(cols):
    parts = np.zeros(len(cols), mr.PARTICLE)
    for i, col in enumerate(cols):
        parts[i]["x"], parts[i]["y"] = pose_in(col, 4, WALLS_ANCHOR)
    parts["parent"] = np.arange(len(cols))
    return parts


def test_two_walls_by_hand():
    """The pose at column 0 sees the wall at column 25 where its beams end. The pose at column 20 also ends on a wall, the one at
    column 45, but its beams pass through the wall at column 25 on the way: the field gives both the same byte, the beam model
    does not, and after one update the through-the-wall pose weighs less."""
    image = two_walls()
    dist2 = cr.dist2_separable(image)
    tab = tj.table()
    parts = walls_particles([0, 20])
    bm = dict(n_cells=3, stride=1, n_beams=3, bx=np.array([b[0] for b in WALLS_BEAMS]), by=np.array([b[1] for b in WALLS_BEAMS]))
    bm["fx"] = (bm["bx"].astype(F32) + F32(0.5)) * F32(CELL)
    bm["fy"] = (bm["by"].astype(F32) + F32(0.5)) * F32(CELL)
    field = mf.field(dist2, mf.table(CELL, WALLS_Q["sigma"], WALLS_Q["max_dist"]))
    S_field = mr.scores(parts, bm, field, WALLS_MQ, WALLS_ANCHOR, tab)
    S_beam, counts, _ = br.scores(parts, bm, image, WALLS_MQ, WALLS_ANCHOR, tab, WALLS_B)
    T = br.table(WALLS_B, CELL)
    print(f"field scores {S_field.tolist()} beam scores {S_beam.tolist()} counts {counts} table {T.tolist()}")
    assert S_field[0] == S_field[1] == 3 * 255          # both poses' beams end on wall cells
    assert S_beam[0] == 3 * int(T[4]) and S_beam[1] == 3 * int(T[0]) and S_beam[1] < S_beam[0]
    assert counts == [3, 3, 0, 0, 0, 0]                # the first occupied cell of the second pose lies 20 steps early: e = -4
    assert br.walk_plain(image, 0, 4, 25, 0, 4)[:2] == (br.AT, 4) and br.walk_plain(image, 20, 4, 25, 0, 4)[:2] == (br.EARLY, 0)
    # one update of a filter with a cluster at the true pose and one particle through the wall
    q = dict(WALLS_Q, n_particles=4, seed=1)
    parts = walls_particles([0, 0, 0, 20])
    A = tmm.clouds_of(tml.split(tml.body_points(WALLS_BEAMS)))[1]
    _, wt, info, binfo = br.update(parts, A, dist2, image, WALLS_MQ, WALLS_ANCHOR, q, WALLS_B, 0, tab)
    assert info["n_beams"] == 3 and binfo["n_rays"] == 12 and wt["weight"][3] < wt["weight"][:3].sum() and wt["weight"][3] < wt["weight"][0]
    _, wt_f, _ = mr.update(parts, A, dist2, WALLS_MQ, WALLS_ANCHOR, q, 0, tab)
    assert (wt_f["weight"] == 65536).all()             # the field cannot tell them apart


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_room_is_tracked_on_the_restatement_alone(seed):
    """§29's room and its bound (one cell, 0.05 rad at the last update) with the beam model on: occlusion costs the filter
    nothing where the field already works."""
    image = tmm.image_of([tml.ROOM], NX, NY)
    dist2 = cr.dist2_separable(image)
    T = tml.truths()
    frames = lambda k: (tmm.clouds_of(tml.split(tml.body_points(tml.scan_of(T[k]))))[1], dist2, ANCHOR, image)
    f = br.Filter(dict(tml.TRACK_Q, seed=seed), MQ, tj.table(), b_of(over_cells=4, sigma=0.1))
    infos = tml.track(f, frames, (tml.TRUTH0[0] + 0.25, tml.TRUTH0[1] - 0.2, tml.TRUTH0[2] + 0.08))
    for k, info in enumerate(infos):
        print(f"seed {seed} round {k}: off {tml.off_truth(info, T[k])} n_eff {info['n_eff']:.1f} resampled {info['resampled']}")
    d, a = tml.off_truth(infos[-1], T[-1])
    assert d <= 0.1 and a <= 0.05


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def beam_configure(cm, b):
    if b is None:
        cm.map_mcl_beam_configure(None)
    else:
        cm.map_mcl_beam_configure(b["over_cells"], b["sigma"], b["z_hit"], b["z_short"], b["z_rand"], bool(b["flags"] & 1))


class BeamPair(tml.Pair):
    """tests/test_map_mcl.py's Pair with the mode: the library's layer and the restatement in lockstep."""

    def __init__(self, cm, q, beam, mq=MQ, n_cap=16384):
        self.cm, self.q, self.n_cap = cm, q, n_cap
        cm.map_mcl_configure(q["n_particles"], q["max_beams"], q["range_cells"], q["sigma"], q["max_dist"], q["tau"], q["resample_frac"],
                             bool(q["flags"] & 1), q["seed"])
        self.f = br.Filter(q, mq, TAB(), None)
        if beam is not None:
            self.beam(beam)

    def beam(self, b):
        beam_configure(self.cm, b)
        self.f.beam_configure(b)

    def update(self):
        cm = self.cm
        A = tg.host_clouds(cm, self.n_cap, False)[0]
        _, dist2, minfo = cm.map_cost()
        image = cm.map_occupancy()[0]
        want_w, want = self.f.update(A, dist2, tuple(minfo.anchor), image)
        info = cm.map_mcl_update()
        w, i1 = cm.map_mcl_weights()
        p_ptr, w_ptr, i2 = cm.map_mcl_device()
        assert bytes(info) == bytes(i1) == bytes(i2)
        tml.same_info(info, want)
        if w.tobytes() != want_w.tobytes():
            bad = np.flatnonzero(w != want_w)
            raise AssertionError(f"{len(bad)} of {len(w)} weights differ, first {bad[0]}: got {w[bad[0]]} want {want_w[bad[0]]}")
        parts = self.particles()
        dp, dw = np.zeros_like(parts), np.zeros_like(w)
        rt = tg.hip_rt()
        assert p_ptr and w_ptr and rt.hipMemcpy(C.c_void_p(dp.ctypes.data), C.c_void_p(p_ptr), C.c_size_t(dp.nbytes), 2) == 0
        assert rt.hipMemcpy(C.c_void_p(dw.ctypes.data), C.c_void_p(w_ptr), C.c_size_t(dw.nbytes), 2) == 0
        assert dp.tobytes() == parts.tobytes() and dw.tobytes() == want_w.tobytes()
        if self.f.beam is None:
            tm.refused(cm, cm.map_mcl_beam_info, text=b"without the beam model")
            return w, info, None
        bi = cm.map_mcl_beam_info()
        for f in ("n_rays",) + br.COUNTS:
            assert getattr(bi, f) == self.f.binfo[f], (f, getattr(bi, f), self.f.binfo)
        assert sum(getattr(bi, f) for f in br.COUNTS) == bi.n_rays == info.n_particles * info.n_beams
        return w, info, self.f.binfo


def both_modes(cm, q, b, drive, mq=MQ):
    """drive(pair) for the jump walk and for the plain walk on the same input; the weight tables of the two must be the same
    bytes (each was compared with the restatement already)."""
    out = []
    for plain in (0, 1):
        p = BeamPair(cm, q, dict(b, flags=plain), mq)
        out.append(drive(p))
    return out


@pytest.fixture(scope="module")
def room():
    with capi.CloudMerger(max_points_total=16384, max_sensors=2, flags=capi.FLAG_PROFILE) as cm:
        tml.build_room(cm)
        yield cm


@pytest.fixture(scope="module")
def lab():
    """A context whose map is loaded per test (cm_map_load), with no cast layer."""
    with capi.CloudMerger(max_points_total=16384, max_sensors=2, flags=capi.FLAG_PROFILE) as cm:
        yield cm


def lab_load(cm, image, mq, anchor):
    tm.configure(cm, mq)
    cm.map_cost_configure(0.0, 0.3, 3.0, False)
    tcs.load(cm, image, anchor, mq)


def one_update(start, sd=(0.3, 0.3, 0.1)):
    def drive(p):
        p.init_pose(*start, *sd)
        return p.update()
    return drive


COUNTS_N = [1, 3, 4, 5, 63, 64, 65, 257, 300]
COUNTS_B = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_beams,over", [(n, COUNTS_B[(3 * i + 2) % 8], (0, 1, 64)[i % 3]) for i, n in enumerate(COUNTS_N)]
                         + [(COUNTS_N[(2 * i + 1) % 9], b, (64, 0, 1)[i % 3]) for i, b in enumerate(COUNTS_B)])
def test_particle_and_beam_counts(room, n, n_beams, over):
    cells = tml.some_body_cells(n_beams, reach=30)
    tml.frame(room, tml.body_points(cells))
    (w, info, bi), _ = both_modes(room, tml.q_of(n_particles=n, max_beams=512, seed=n + n_beams), b_of(over_cells=over),
                                  one_update((tml.TRUTH0[0], tml.TRUTH0[1], tml.TRUTH0[2])))
    assert (info.n_particles, info.n_beams, bi["n_rays"]) == (n, n_beams, n * n_beams)
    if n_beams == 0:
        assert (w["score"] == 0).all() and (w["weight"] == 65536).all()


@pytest.mark.gpu
def test_with_deskew():
    """The beams are the body cells of the frame's clouds, which under motion are the compensated records. Two updates with a
    predict between them in both walks: weights, info, particles and the outcome counts are the restatement's on the library's
    merged(), and the same bytes with and without motion."""
    def drive(p):
        p.init_pose(tml.TRUTH0[0] + 0.25, tml.TRUTH0[1] - 0.2, tml.TRUTH0[2] + 0.08, 0.3, 0.3, 0.1)
        w1, i1, b1 = p.update()
        p.predict(0.1, 0.0, 0.05, 0.03, 0.03, 0.02)
        w2, i2, b2 = p.update()
        assert i1.n_beams > 32 and b1["n_rays"] == i1.n_particles * i1.n_beams
        return w1.tobytes(), bytes(i1), sorted(b1.items()), w2.tobytes(), bytes(i2), sorted(b2.items()), p.particles().tobytes()

    q = tml.q_of(n_particles=300, max_beams=256, range_cells=64, seed=6)
    walks = []
    for plain_walk in (0, 1):
        a, b = tml.deskew_pair(lambda cm: BeamPair(cm, q, b_of(over_cells=4, flags=plain_walk)), drive)
        assert a == b
        walks.append(a)
    assert walks[0][0] == walks[1][0] and walks[0][3] == walks[1][3]      # the jump walk and the plain walk: the same weights


@pytest.mark.gpu
def test_the_two_walls_on_the_device(lab):
    lab_load(lab, two_walls(), WALLS_MQ, WALLS_ANCHOR)
    tml.frame(lab, tml.body_points(WALLS_BEAMS))
    T = br.table(WALLS_B, CELL)
    for col, want, cls in ((0, 3 * int(T[4]), "n_at"), (20, 3 * int(T[0]), "n_early")):
        x, y = pose_in(col, 4, WALLS_ANCHOR)
        for (w, info, bi) in both_modes(lab, dict(WALLS_Q, seed=1), WALLS_B, one_update((x, y, 0.0), (0.0, 0.0, 0.0)), WALLS_MQ):
            assert (w["score"] == want).all() and bi[cls] == 6 == bi["n_rays"]
        p = BeamPair(lab, dict(WALLS_Q, seed=1), None, WALLS_MQ)     # the field score of the same poses
        p.init_pose(x, y, 0.0)
        assert (p.update()[0]["score"] == 3 * 255).all()


RAYS = [(10, 0), (9, 9), (-11, 4)]                     # an axis ray, a diagonal ray, a skew ray


@pytest.mark.gpu
@pytest.mark.parametrize("over", [0, 1, 64])
def test_wall_positions(lab, over):
    """A lone occupied cell at steps L - E - 1, L - E, L - 1, L, L + 1, L + E and L + E + 1 of each ray: the line is the same
    from every origin, so the pose is moved instead of the wall."""
    nx, ny = 200, 180
    mq, anchor = mpr.params(CELL, nx, ny), tmm.anchor_of(nx, ny)
    wall = (100, 90)
    img = np.zeros((ny, nx), np.int8)
    img[wall[1], wall[0]] = 100
    lab_load(lab, img, mq, anchor)
    tml.frame(lab, tml.body_points(RAYS))
    E = over
    for plain in (0, 1):
        p = BeamPair(lab, tml.q_of(n_particles=3, max_beams=64, range_cells=16, seed=2), b_of(over_cells=E, flags=plain), mq)
        for r, (dx, dy) in enumerate(RAYS):
            L = max(abs(dx), abs(dy))
            for k in sorted({L - E - 1, L - E, L - 1, L, L + 1, L + E, L + E + 1}):
                if k < 0:
                    continue
                jx, jy = br.cell_at(k, dx, dy, L)
                ox, oy = wall[0] - jx, wall[1] - jy
                want = br.walk_plain(img, ox, oy, dx, dy, E)
                assert want[:2] == ((br.BEYOND, 2 * E + 1) if k > L + E else br.outcome(k, L, E))
                p.init_pose(*pose_in(ox, oy, anchor), 0.0)
                _, info, bi = p.update()
                hits = bi["n_early"] + bi["n_at"] + bi["n_late"]
                assert info.n_beams == 3 and hits >= 3 * (k <= L + E), (dx, dy, k, bi)
                assert bi[br.COUNTS[want[0]]] >= 3


@pytest.mark.gpu
def test_skip_ties_on_the_diagonal(lab):
    """A lone occupied cell at (j, j) from the origin on the exact diagonal: dist2 at the origin is exactly 2 j^2 and the
    smallest j with 2 j^2 >= dist2 lands on it."""
    for j in (1, 2, 3, 11):
        img = np.zeros((NY, NX), np.int8)
        img[20 + j, 30 + j] = 100
        lab_load(lab, img, MQ, ANCHOR)
        assert lab.map_cost()[1][20, 30] == 2 * j * j
        tml.frame(lab, tml.body_points([(12, 12), (-12, -12)]))
        x, y = pose_in(30, 20, ANCHOR)
        for (w, info, bi) in both_modes(lab, tml.q_of(n_particles=2, seed=3), b_of(over_cells=2), one_update((x, y, 0.0), (0.0, 0.0, 0.0))):
            # the beam of 12 steps meets the cell at step j, early; the opposite one ends 14 steps away on free cells
            assert (bi["n_early"], bi["n_beyond"], bi["n_rays"]) == (2, 2, 4) and (w["score"] == w["score"][0]).all()


EDGE_X, EDGE_Y = tml.EDGE_X, tml.EDGE_Y
PLACES = tml.PLACES + [("first_corner", (ANCHOR[0] + 0.5) * CELL, (ANCHOR[1] + 0.5) * CELL, 0.0), ("far_corner", EDGE_X, (ANCHOR[1] + 0.5) * CELL, 0.0),
                       ("near_corner", (ANCHOR[0] + 0.5) * CELL, EDGE_Y, 0.0), ("outside_left", (ANCHOR[0] - 1.5) * CELL, 0.05, 0.0),
                       ("outside_above", 0.05, EDGE_Y + 0.2, 0.0), ("on_a_wall",) + pose_in(30, 10, ANCHOR) + (0.0,),
                       ("no_cell_y", 0.05, -1e30, 0.0)]


@pytest.mark.gpu
def test_particle_and_beam_placements(room):
    """All particles on one pose: on the window's edges and corners, outside each edge, where no cell exists, on an occupied
    cell, at the headings around the table's rounding and wrap. The beams: the particle's own cell (L = 0), neighbours, and
    some far enough to leave the window through every edge and corner from a pose near it."""
    far = [(60, 0), (-60, 0), (0, 60), (0, -60), (60, 60), (-60, 60), (60, -60), (-60, -60)]
    tml.frame(room, tml.body_points([(0, 0), (-1, 0), (0, -1), (-3, -3), (1, 0), (0, 1), (12, 5), (-20, 9)] + far))
    for name, x, y, yaw in PLACES:
        (w, info, bi), _ = both_modes(room, tml.q_of(n_particles=66, max_beams=64, seed=6), b_of(over_cells=3), one_update((x, y, yaw), (0.0, 0.0, 0.0)))
        print(f"{name}: score {int(w['score'][0])} {bi}")
        assert (w["score"] == w["score"][0]).all() and info.n_beams == 16
        if name in ("outside", "outside_below", "outside_left", "outside_above", "no_cell", "no_cell_y"):
            assert bi["n_skipped"] == bi["n_rays"] and w["score"][0] == 0
        else:
            assert bi["n_skipped"] == 0
        if name == "on_a_wall":
            assert bi["n_early"] == 66 * 15 and bi["n_at"] == 66      # every ray but the L = 0 beam hits at step 0: e = max(-L, -3)
    image = room.map_occupancy()[0]
    assert image[10, 30] == 100
    # positions that are not finite or beyond every cell come from a predict, which may overflow; the update must not mind
    for big in (3e38, 1e30):
        def drive(p, big=big):
            p.init_pose(big, 0.05, 0.0)
            p.predict(big, 0.0, 0.0)
            return p.update()
        for (w, info, bi) in both_modes(room, tml.q_of(n_particles=5, max_beams=64, seed=6), b_of(over_cells=3), drive):
            assert bi["n_skipped"] == bi["n_rays"] == 5 * 16
    # an inf and then a NaN position: x + c a overflows, then inf - inf
    def drive(p):
        p.init_pose(3e38, 0.05, math.pi)
        p.predict(3e38, 0.0, 0.0)                      # x = 3e38 + (-1) * 3e38 - ... stays finite or not: whatever it is, both sides agree
        p.predict(-3e38, 3e38, 0.0)
        return p.update()
    both_modes(room, tml.q_of(n_particles=5, max_beams=64, seed=6), b_of(over_cells=3), drive)


@pytest.mark.gpu
def test_the_largest_reach(lab):
    """One particle in a 2048 x 8 window with range_cells 1024 and over_cells 64: L + E = 1088 along the row, and the diagonal
    beams of |d| = 1024 whose end cells lie far outside."""
    nx, ny = 2048, 8
    mq, anchor = mpr.params(CELL, nx, ny), tmm.anchor_of(nx, ny)
    for wall in (None, 1090, 1030):
        img = np.zeros((ny, nx), np.int8)
        if wall is not None:
            img[:, wall] = 100
        lab_load(lab, img, mq, anchor)
        tml.frame(lab, tml.body_points([(1024, 0), (1024, 3), (-1024, -2), (1024, 1024), (-1024, 1024), (1000, -1)]))
        x, y = pose_in(10, 4, anchor)
        for (w, info, bi) in both_modes(lab, tml.q_of(n_particles=1, max_beams=64, range_cells=1024, seed=4), b_of(over_cells=64),
                                        one_update((x, y, 0.0), (0.0, 0.0, 0.0)), mq):
            assert info.n_beams == 6 and bi["n_off"] == 3 and bi["n_skipped"] == 0
            assert (bi["n_beyond"], bi["n_late"], bi["n_early"]) == {None: (3, 0, 0), 1090: (1, 2, 0), 1030: (0, 1, 2)}[wall]


@pytest.mark.gpu
@pytest.mark.parametrize("pct", [0, 1, 5, 20])
def test_random_maps(lab, pct):
    lab_load(lab, tcs.random_image(pct, 60 + pct) if pct else np.full((NY, NX), -1, np.int8), MQ, ANCHOR)
    tml.frame(lab, tml.body_points(tml.some_body_cells(200, reach=45, seed=pct)))
    (w, info, bi), _ = both_modes(lab, tml.q_of(n_particles=300, max_beams=256, seed=10 + pct), b_of(over_cells=6), one_update((0.3, -0.2, 0.7), (2.5, 2.0, 3.0)))
    assert info.n_beams == 200 and bi["n_rays"] == 60000 and bi["n_off"] > 0
    assert (bi["n_early"] + bi["n_at"] + bi["n_late"] > 0) == (pct > 0)


@pytest.mark.gpu
def test_a_dense_frame_at_the_largest_beam_capacity(room):
    """max_beams 8192: the staged beams alone fill 64 KiB of LDS, and the counts and the table lie behind them."""
    cells = [(x, y) for x in range(-50, 50) for y in range(-50, 50)]
    tml.frame(room, tml.body_points(cells))
    (w, info, bi), _ = both_modes(room, tml.q_of(n_particles=5, max_beams=8192, range_cells=64, seed=4), b_of(over_cells=64), one_update((0.0, 0.0, 0.0), (1.0, 1.0, 0.5)))
    assert (info.n_cells, info.stride, info.n_beams, bi["n_rays"]) == (10000, 2, 5000, 25000)


@pytest.mark.gpu
def test_an_empty_map_is_refused_as_before(lab):
    tm.configure(lab, MQ)
    lab.map_cost_configure(0.0, 0.3, 3.0, False)
    tml.frame(lab, tml.body_points([(1, 1)]))
    lab.map_mcl_configure(8)
    beam_configure(lab, b_of())
    lab.map_mcl_init_pose(0.0, 0.0, 0.0)
    tm.refused(lab, lab.map_mcl_update, text=b"cm_map_integrate")    # n_frames == 0
    beam_configure(lab, None)
    tm.refused(lab, lab.map_mcl_update, text=b"cm_map_integrate")


@pytest.mark.gpu
@pytest.mark.parametrize("always", [0, 1])
def test_accumulation_over_three_updates(room, always):
    tml.frame(room, tml.body_points(tml.scan_of(tml.TRUTH0)))

    def drive(p):
        p.init_pose(tml.TRUTH0[0] + 0.1, tml.TRUTH0[1], tml.TRUTH0[2], 0.3, 0.3, 0.1)
        acc = np.zeros(400, np.int64)
        for k in range(3):
            w, info, _ = p.update()
            assert info.resampled == always and info.gen == 1 + 2 * k
            acc = np.zeros(400, np.int64) if always else acc + w["score"]
            assert (p.particles()["acc"] == acc).all()
            p.predict(0.02, 0.0, 0.01, 0.01, 0.01, 0.01)
        return w

    a, b = both_modes(room, tml.q_of(n_particles=400, max_beams=256, resample_frac=float(always), flags=always, seed=12), b_of(over_cells=4), drive)
    assert a.tobytes() == b.tobytes() and a["score"].max() > 0


@pytest.mark.gpu
def test_switching_the_mode_and_staleness(room):
    cm = room
    tml.frame(cm, tml.body_points(tml.scan_of(tml.TRUTH0)))
    q = tml.q_of(n_particles=300, max_beams=256, seed=13)
    tm.refused(cm, lambda: (cm.map_mcl_configure(None), beam_configure(cm, b_of()))[1], text=b"cm_map_mcl_configure")   # no layer: the table's text
    ref = tml.Pair(cm, q)                               # the parent commit's field score, never touched by the mode
    ref.init_pose(tml.TRUTH0[0], tml.TRUTH0[1], tml.TRUTH0[2], 0.3, 0.3, 0.1)
    w_field = ref.update()[0]
    p = BeamPair(cm, q, None)
    start = p.init_pose(tml.TRUTH0[0], tml.TRUTH0[1], tml.TRUTH0[2], 0.3, 0.3, 0.1)
    stale = lambda text: [tm.refused(cm, call, text=text) for call in (cm.map_mcl_weights, cm.map_mcl_device, cm.map_mcl_beam_info)]
    p.beam(b_of(over_cells=4))                         # on: gen and the particles stay
    assert p.particles().tobytes() == start.tobytes()
    stale(b"since cm_map_mcl_beam_configure")
    w_on, info, _ = p.update()
    assert info.gen == 1
    names = [n for n, _ in cm.stage_times()]
    assert names == ["mcl_clear", "k_match_field", "k_mcl_mark", "k_mcl_compact", "k_mcl_steps", "k_mcl_beam", "k_mcl_best", "k_mcl_weights", "k_mcl_spread",
                     "k_mcl_resample"]
    p.update()
    assert "k_mcl_steps" not in [n for n, _ in cm.stage_times()] and "k_mcl_beam" in [n for n, _ in cm.stage_times()]
    cm.map_cost_update()                               # dist2 anew: the skip bytes are rebuilt once
    p.update()
    assert "k_mcl_steps" in [n for n, _ in cm.stage_times()]
    p.beam(None)                                       # off: the field score, and no beam info
    stale(b"since cm_map_mcl_beam_configure")
    p.update()
    assert [n for n, _ in cm.stage_times()][4] == "k_mcl_score"
    p.beam(b_of(over_cells=4, flags=1))                # on again, plain: never a steps pass
    p.update()
    assert "k_mcl_steps" not in [n for n, _ in cm.stage_times()] and "k_mcl_beam" in [n for n, _ in cm.stage_times()]
    # the off state from the start gives the field score's bytes
    p = BeamPair(cm, q, b_of())
    p.beam(None)
    p.init_pose(tml.TRUTH0[0], tml.TRUTH0[1], tml.TRUTH0[2], 0.3, 0.3, 0.1)
    assert p.update()[0].tobytes() == w_field.tobytes() and w_on.tobytes() != w_field.tobytes()
    # cm_map_mcl_configure in either form frees the mode
    beam_configure(cm, b_of())
    cm.map_mcl_configure(300, 256, 64, seed=13)
    cm.map_mcl_init_pose(0.0, 0.0, 0.0)
    cm.map_mcl_update()
    assert [n for n, _ in cm.stage_times()][4] == "k_mcl_score"
    tm.refused(cm, cm.map_mcl_beam_info, text=b"without the beam model")
    # every refusal of the restatement's validator is the library's, and a refused call changes nothing
    L = cm._lib
    beam_configure(cm, b_of(over_cells=2))
    cm.map_mcl_update()
    keep = bytes(cm.map_mcl_beam_info())
    for kw in REFUSED_BEAMS:
        b = b_of(**kw)
        pp = capi.MclBeamParams(b["over_cells"], b["sigma"], b["z_hit"], b["z_short"], b["z_rand"], b["flags"])
        assert L.cm_map_mcl_beam_configure(cm._ctx, C.byref(pp)) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
    assert bytes(cm.map_mcl_beam_info()) == keep
    for kw in ACCEPTED_BEAMS:
        beam_configure(cm, b_of(**kw))
    # a frame in flight
    sensors = tmm.clouds_of(tml.split(tml.body_points(tml.scan_of(tml.TRUTH0))))[0]
    cm.submit_all(sensors)
    cm.merge_voxelize_async(capi.make_params(tml.tc.PARAMS))
    for call in (lambda: beam_configure(cm, b_of()), lambda: beam_configure(cm, None), cm.map_mcl_beam_info):
        tm.refused(cm, call, text=b"flight")
    assert cm.wait().status == capi.OK
    cm.map_mcl_configure(None)


@pytest.mark.gpu
def test_a_beam_update_changes_no_other_layer(room):
    cm = room
    cm.map_plan_configure(50, 205, True)
    cm.map_traj_configure(3, 3, 4, [(0.1, 0.0)], 1, 1, True)
    cm.map_frontier_configure()
    cm.map_match_configure(0.1, 0.3, 1, 8, 2, 2)
    cm.map_cast_configure(16, 8, 30)
    tml.frame(cm, tml.body_points(tml.scan_of(tml.TRUTH0)))
    cm.map_plan_update(2.05, 1.05)
    cm.map_traj_evaluate(0.05, 0.05, 0.0, (0.0, 1.0), (-1.0, 1.0), 0.1)
    cm.map_frontier_update()
    cm.map_match(tm.pose_t(0.1, 0.0))
    cm.map_cast(tcs.random_poses(16, 1))

    def state():
        table, info = cm.map()
        cost, dist2, _ = cm.map_cost()
        return (table.tobytes(), cm.map_occupancy()[0].tobytes(), tm.info_tuple(info), cost.tobytes(), dist2.tobytes(), cm.map_cost_table().tobytes(),
                cm.map_plan()[0].tobytes(), cm.map_traj()[0].tobytes(), bytes(cm.map_traj()[1]), cm.map_frontier_labels()[0].tobytes(),
                cm.map_match_scores()[0].tobytes(), bytes(cm.map_match_scores()[1]), cm.map_cast_rays()[0].tobytes(), bytes(cm.map_cast_rays()[1]),
                cm.merged(16384).tobytes())

    before = state()
    both_modes(cm, tml.q_of(n_particles=300, max_beams=256, seed=11), b_of(over_cells=5), one_update(tml.TRUTH0))
    assert state() == before                           # nothing went stale either: every read above still answers
    cm.map_cast(tcs.random_poses(16, 1))
    assert "k_cast_steps" not in [n for n, _ in cm.stage_times()]     # the cast layer's skip bytes are its own and still fresh
    for call in (cm.map_plan_configure, cm.map_match_configure, cm.map_cast_configure, cm.map_mcl_configure):
        call(None)
