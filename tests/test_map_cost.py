"""The cost layer over the occupancy map: cm_map_cost_configure, cm_map_cost_update, cm_map_cost_copy, cm_map_dist_copy,
cm_map_cost_device, cm_map_cost_table_copy (include/cloudmerge.h, cm_kernels_cost.hip, cm_cost_table.hpp).

The bar on the GPU: every byte of cost, of dist2, of the table, of the info and of the device-pointer variants equal to the
restatement (tests/cost_ref.py) fed with the library's own image (map_occupancy()) and the map's cell. There is no tolerance:
a squared distance in cells is an integer and the table is built from an exponential that is spelled out. The images are
designed: one point of A at the centre of each wanted cell makes it 100 in one frame (l_occ <= l_hit); a sensor outside the
window casts no rays (an image of 100 and -1 only), one inside gives free cells too. The named cases assert
cost_ref.guards on the restatement's output before the device's bytes are looked at."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import cost_ref as cr
from tests import map_ref as mr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_occupancy_map as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cloudmerge.h")
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")
F32 = np.float32
INF = float("inf")
NAMES = ("cm_map_cost_configure", "cm_map_cost_update", "cm_map_cost_copy", "cm_map_dist_copy", "cm_map_cost_device",
         "cm_map_cost_table_copy")
COST_TYPES = (capi.CostParams,)                    # (a library without the cost layer fails every test here, at import)
ROWS = tr.device_define("CM_COST_ROWS")            # rows of one block of k_cost_colmask / k_cost_colcarry: one 32-bit word
STRIP = tr.device_define("CM_COST_BLOCK")          # cells of one strip of k_cost_rows' workgroup along x
Q = cr.params(0.35, 1.05, 3.0)                     # the radii of a small robot on 10 cm cells


# ---- CPU: the interface -------------------------------------------------------------------------------------------------
def test_cost_struct_and_constants_match_header(tmp_path):
    fields = ["inscribed_radius", "inflation_radius", "cost_scaling", "flags"]
    names = ["CM_MAP_DIST_NONE", "CM_COST_LETHAL", "CM_COST_INSCRIBED", "CM_COST_NO_INFORMATION", "CM_COST_INFLATE_UNKNOWN",
             "CM_COST_MAX_RADIUS_CELLS", "CM_COST_MAX_AXIS"]
    items = ["sizeof(cm_cost_params)"] + [f"offsetof(cm_cost_params,{f})" for f in fields] + names
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cloudmerge.h"\nint main(void){'
                   + "".join(f'printf("%llu ",(unsigned long long)({it}));' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = capi.CostParams
    assert got[:5] == [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == [16, 0, 4, 8, 12]
    assert got[5:] == [capi.MAP_DIST_NONE, capi.COST_LETHAL, capi.COST_INSCRIBED, capi.COST_NO_INFORMATION, capi.COST_INFLATE_UNKNOWN,
                       capi.COST_MAX_RADIUS_CELLS, capi.COST_MAX_AXIS]
    assert got[5:] == [cr.DIST_NONE, cr.LETHAL, cr.INSCRIBED, cr.NO_INFORMATION, cr.INFLATE_UNKNOWN, cr.MAX_RADIUS_CELLS, cr.MAX_AXIS]
    assert got[5:] == [0xFFFFFFFF, 254, 253, 255, 1, 256, 2048]
    assert tr.device_define("CM_COST_MAX_AXIS_DEV") == 2048 and ROWS == 32 and STRIP == 256
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and re.search(r"CM_API\s+int\s+" + name + r"\(", text)


def test_null_context_calls_are_bad_args():
    L = capi.load()
    p = capi.CostParams(0.35, 1.05, 3.0, 0)
    info = capi.MapInfo()
    before = bytes(info)
    cost = np.full(16, 7, np.uint8)
    dist = np.full(16, 7, np.uint32)
    a, b, n = C.c_void_p(5), C.c_void_p(6), C.c_uint64(9)
    assert L.cm_map_cost_configure(None, C.byref(p)) == capi.BAD_ARG and L.cm_map_cost_configure(None, None) == capi.BAD_ARG
    assert L.cm_map_cost_update(None, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cost_copy(None, cost.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_dist_copy(None, dist.ctypes.data, 16, C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cost_device(None, C.byref(a), C.byref(b), C.byref(info)) == capi.BAD_ARG
    assert L.cm_map_cost_table_copy(None, cost.ctypes.data, 16, C.byref(n)) == capi.BAD_ARG
    assert (cost == 7).all() and (dist == 7).all() and bytes(info) == before and (a.value, b.value, n.value) == (5, 6, 9)


# ---- CPU: the two restatements --------------------------------------------------------------------------------------------
def random_image(rng, ny, nx, share):
    image = rng.choice(np.array([-1, 0], np.int8), size=(ny, nx))
    image[rng.random((ny, nx)) < share] = 100
    return image


def test_the_two_restatements_agree():
    rng = np.random.default_rng(11)
    some = 0
    for ny, nx in ((1, 1), (1, 70), (70, 1), (33, 65), (67, 129)):
        for share in (0.0, 0.02, 1.0):
            image = random_image(rng, ny, nx, share)
            for q in (Q, dict(Q, flags=cr.INFLATE_UNKNOWN)):
                a, b = cr.cost_brute(image, 0.1, q), cr.cost_separable(image, 0.1, q)
                assert all(u.tobytes() == v.tobytes() and u.dtype == v.dtype and u.shape == v.shape for u, v in zip(a, b))
                assert a[0].dtype == np.uint8 and a[1].dtype == np.uint32 and a[0].shape == a[1].shape == (ny, nx)
            if share == 0.0:
                assert (a[1] == cr.DIST_NONE).all() and set(np.unique(a[0]).tolist()) <= {0, 255}
            if share == 1.0:
                assert not a[1].any() and (a[0] == 254).all()
            some += int(((a[1] > 0) & (a[1] != cr.DIST_NONE)).sum())
    assert some > 5000


# cell 1, inscribed radius 1, inflation radius 3, scaling 1: R = 3 and the table by hand is
#   d2 0: 254;  1: m = 1 <= 1, 253;  2: 252 e^-0.4142 = 166.5;  3: 252 e^-0.7321 = 121.2;  4: 252 e^-1 = 92.7;
#   5: 252 e^-1.2361 = 73.2;  6: 252 e^-1.4495 = 59.2;  7: 252 e^-1.6458 = 48.6;  8: 252 e^-1.8284 = 40.5 (40.49);
#   9: m = 3 <= 3, 252 e^-2 = 34.1.
HAND_TABLE = [254, 253, 166, 121, 92, 73, 59, 48, 40, 34]
# x ->      the obstacle in the corner (0, 0); an unknown cell at distance 1 (inside the inscribed radius), one at
# y |       d2 = 5 (inside the inflation radius only) and one at d2 = 18 (beyond it); the free cell (4, 0) at d2 = 16 > 9.
HAND_IMAGE = [[100, -1, 0, 0, 0],
              [0, 0, -1, 0, 0],
              [0, 0, 0, 0, 0],
              [0, 0, 0, -1, 0]]
HAND_DIST2 = [[0, 1, 4, 9, 16], [1, 2, 5, 10, 17], [4, 5, 8, 13, 20], [9, 10, 13, 18, 25]]       # x^2 + y^2
HAND_COST = [[254, 253, 92, 34, 0],                # (1, 0): unknown, 253 >= 253 stays 253
             [253, 166, 255, 0, 0],                # (2, 1): unknown, 73 < 253 is NO_INFORMATION; with inflate_unknown 73
             [92, 73, 40, 0, 0],
             [34, 0, 0, 255, 0]]                   # (3, 3): unknown, 0 either way is NO_INFORMATION


def test_known_answers_on_a_5_by_4_image():
    q = cr.params(1.0, 3.0, 1.0)
    image = np.array(HAND_IMAGE, np.int8)
    for f in (cr.cost_brute, cr.cost_separable):
        cost, dist2, lut = f(image, 1.0, q)
        assert lut.tolist() == HAND_TABLE and dist2.tolist() == HAND_DIST2 and cost.tolist() == HAND_COST
        cost, dist2, lut = f(image, 1.0, dict(q, flags=cr.INFLATE_UNKNOWN))
        want = [row[:] for row in HAND_COST]
        want[1][2] = 73
        assert lut.tolist() == HAND_TABLE and dist2.tolist() == HAND_DIST2 and cost.tolist() == want


def test_known_table():
    lut = cr.table(0.1, Q)
    assert cr.radius_cells(0.1, 1.05) == 11 and len(lut) == 122 and lut.dtype == np.uint8
    assert lut[0] == 254 and (lut[1:13] == 253).all()
    assert lut[13:20].tolist() == [244, 234, 225, 216, 209, 201, 194]
    assert (np.diff(lut.astype(int)) <= 0).all()
    assert cr.table(0.1, cr.params(0.0, 0.0, 3.0)).tolist() == [254]                          # R = 0: one entry
    flat = cr.table(0.1, cr.params(0.35, 1.05, 0.0))
    assert set(flat[13:111].tolist()) == {252} and flat[111] == 0                             # no decay; sqrt(111) * 0.1 > 1.05
    assert len(cr.table(0.1, cr.params(0.0, 25.6, 0.1))) == 256 * 256 + 1


TABLE_CASES = [(0.1, Q), (0.1, cr.params(0.0, 0.0, 3.0)), (0.1, cr.params(0.3, 25.6, 0.25)), (0.05, cr.params(0.0, 1.0, 10.0)),
               (1.0, cr.params(1.0, 3.0, 1.0)), (0.25, cr.params(2.0, 2.0, 1.0)), (0.1, cr.params(0.35, 1.05, 0.0))]


def test_table_against_libm():
    """At most 1 per entry: floor(252 e) moves by one where libm's e and cm_exp_neg's differ in the last bits across an integer."""
    worst = 0
    for cell, q in TABLE_CASES:
        a, b = cr.table(cell, q).astype(int), cr.table(cell, q, cr.libm_exp_neg).astype(int)
        worst = max(worst, int(np.abs(a - b).max()))
    print(f"table against math.exp: largest difference {worst}")
    assert worst <= 1


TABLE_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cm_cost_table.hpp"
// argv: cell inscribed inflation scaling max_radius, each float as 8 hex digits of its bits -> "R" then the table in hex, or "refused: <why>"
static float bits(const char* s) { union { unsigned u; float f; } v; v.u = (unsigned)std::strtoul(s, nullptr, 16); return v.f; }
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    uint32_t R = 0;
    const float cell = bits(argv[1]), ri = bits(argv[2]), ro = bits(argv[3]), k = bits(argv[4]);
    if (const char* why = cm_cost_refusal(cell, ri, ro, k, (uint32_t)std::atoi(argv[5]), &R)) { std::printf("refused: %s\n", why); return 0; }
    std::vector<uint8_t> lut((size_t)R * R + 1);
    cm_cost_table(cell, ri, ro, k, R, lut.data());
    std::printf("%u\n", R);
    for (uint8_t v : lut) std::printf("%02x", v);
    std::printf("\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def table_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler")
    d = tmp_path_factory.mktemp("cost_table")
    (d / "driver.cpp").write_text(TABLE_DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(d / "driver.cpp"), "-o", str(exe)], check=True)

    def run(cell, q):
        args = ["%08x" % int(F32(v).view(np.uint32)) for v in (cell, q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"])]
        r = subprocess.run([str(exe)] + args + [str(cr.MAX_RADIUS_CELLS)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    return run


def test_table_builder_on_the_cpu_is_the_restatement_byte_for_byte(table_driver):
    """cm_cost_table.hpp in a program of its own, under the address and undefined-behaviour sanitizers."""
    radii = []
    for cell, q in TABLE_CASES:
        head, body = table_driver(cell, q).split()
        want = cr.table(cell, q)
        assert int(head) ** 2 + 1 == len(want) and bytes.fromhex(body) == want.tobytes()
        radii.append(int(head))
    assert 0 in radii and 256 in radii and 11 in radii
    ok = cr.params(0.35, 1.05, 3.0)
    for kw in REFUSED_PARAMS:
        if "flags" not in kw:
            assert table_driver(0.5, dict(ok, **kw)).startswith("refused"), kw


REFUSED_PARAMS = ([dict(inscribed_radius=v) for v in (np.nan, INF, -0.1)] + [dict(inflation_radius=v) for v in (np.nan, INF, -1.0)] +
                  [dict(cost_scaling=v) for v in (np.nan, INF, -INF, -3.0)] + [dict(inscribed_radius=1.06), dict(inflation_radius=0.3),
                   dict(inflation_radius=128.01), dict(inflation_radius=1e30), dict(flags=2), dict(flags=3), dict(flags=1 << 31)])


def test_every_refusal_of_the_restatement():
    ok = cr.params(0.35, 1.05, 3.0)
    assert cr.refusal(ok) is None and cr.refusal(dict(ok, flags=1)) is None
    bad = lambda **kw: cr.refusal(dict(ok, **kw))
    assert bad(inscribed_radius=np.nan) == bad(inscribed_radius=INF) == bad(inscribed_radius=-0.1) == "inscribed_radius"
    assert bad(inflation_radius=np.nan) == bad(inflation_radius=INF) == bad(inflation_radius=-1.0) == "inflation_radius"
    assert bad(cost_scaling=np.nan) == bad(cost_scaling=INF) == bad(cost_scaling=-3.0) == "cost_scaling"
    assert bad(inscribed_radius=1.06) == bad(inflation_radius=0.3) == "order"
    assert bad(inflation_radius=128.01) == bad(inflation_radius=1e30) == "radius" and bad(inflation_radius=128.0) is None      # R = 256 at cell 0.5
    assert bad(flags=2) == bad(flags=3) == bad(flags=1 << 31) == "flags"
    assert all(cr.refusal(dict(ok, **kw)) is not None for kw in REFUSED_PARAMS)
    assert cr.refusal(ok, have_map=False) == "map" and cr.refusal(ok, in_flight=True) == "flight"
    assert cr.refusal(ok, nx=2049, ny=1) == cr.refusal(ok, nx=1, ny=2049) == "axis" and cr.refusal(ok, nx=2048, ny=2048) is None
    for q in (cr.params(0.0, 0.0, 0.0), cr.params(1.05, 1.05, 3.0), cr.params(0.0, 1.05, 0.0), cr.params(-0.0, 0.0, 3.0)):
        assert cr.refusal(q) is None


# ---- designed images ------------------------------------------------------------------------------------------------------
OUTSIDE = (200.0, 0.0, 0.0)                        # a sensor there casts no rays into any window below
PARAMS = MergeParams(**tg.COARSE)


def map_q(cell, nx, ny):
    return mr.params(cell, nx, ny)


def frame_of(cells, cell, nx, ny, trans, pose_xy=(0.0, 0.0)):
    """One sensor's cloud with a point at the centre of every wanted window cell (ix, iy), for a vehicle at pose_xy: the
    anchor is the vehicle cell minus (nx // 2, ny // 2). No wanted cell: one point far outside the window (a frame needs one)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    vx, vy = (math.floor(float(F32(p) * (F32(1.0) / F32(cell)))) for p in pose_xy)
    ax, ay = vx - nx // 2, vy - ny // 2
    w = np.stack([(ax + cells[:, 0] + 0.5) * cell, (ay + cells[:, 1] + 0.5) * cell, np.zeros(len(cells))], axis=1)
    if len(cells) == 0:
        w = np.array([[(ax + nx + 40.5) * cell, 0.0, 0.0]])
    # in the vehicle frame the world point is w - pose, in the sensor's frame that minus the translation
    p = (w - np.array([pose_xy[0], pose_xy[1], 0.0]) - np.asarray(trans, np.float64)).astype(F32)
    return [xyzi_cloud(p, np.zeros(len(p), F32), t_xyz=tuple(trans))]


def read_cost(cm, info):
    """What the context holds after an update: the info of every call, both tables, both device tables, the cost table."""
    cost, dist2, i1 = cm.map_cost()
    pc, pd, i2 = cm.map_cost_device()
    assert pc and pd and tm.info_tuple(i1) == tm.info_tuple(i2) == tm.info_tuple(info) == tm.info_tuple(cm.map()[1])
    dc, dd = np.zeros_like(cost), np.zeros_like(dist2)
    assert tg.hip_rt().hipMemcpy(C.c_void_p(dc.ctypes.data), C.c_void_p(pc), C.c_size_t(cost.nbytes), 2) == 0
    assert tg.hip_rt().hipMemcpy(C.c_void_p(dd.ctypes.data), C.c_void_p(pd), C.c_size_t(dist2.nbytes), 2) == 0
    return cost, dist2, dc, dd, cm.map_cost_table()


def restate(image, cell, q):
    ny, nx = image.shape
    n_obs = int((image == 100).sum())
    return (cr.cost_separable if ny * nx * nx <= n_obs * ny * nx or ny * nx * nx <= 1 << 26 else cr.cost_brute)(image, cell, q)


def compare(got, want, label):
    (cost, dist2, dc, dd, lut), (c, d, t) = got, want
    assert lut.dtype == np.uint8 and lut.tobytes() == t.tobytes(), label
    assert dist2.dtype == np.uint32 and dist2.shape == d.shape
    if dist2.tobytes() != d.tobytes():
        bad = np.argwhere(dist2 != d)
        iy, ix = bad[0]
        raise AssertionError(f"{label}: dist2 differs in {len(bad)} of {d.size} cells, first ({ix}, {iy}): got {dist2[iy, ix]} want {d[iy, ix]}")
    assert cost.dtype == np.uint8 and cost.shape == c.shape
    if cost.tobytes() != c.tobytes():
        bad = np.argwhere(cost != c)
        iy, ix = bad[0]
        raise AssertionError(f"{label}: cost differs in {len(bad)} of {c.size} cells, first ({ix}, {iy}): got {cost[iy, ix]} want {c[iy, ix]}")
    assert dc.tobytes() == c.tobytes() and dd.tobytes() == d.tobytes(), label


def check(cm, cell, q, label, cells=None, guard=False):
    """Update, read everything back, restate from the library's own image; with both flag settings where guard is set."""
    image, _ = cm.map_occupancy()
    if cells is not None:                           # the designed obstacles are the image's, and nothing else is
        want = np.zeros(image.shape, bool)
        want[np.asarray(cells, np.int64).reshape(-1, 2)[:, 1], np.asarray(cells, np.int64).reshape(-1, 2)[:, 0]] = True
        assert ((image == 100) == want).all(), label
    wants = {f: restate(image, cell, dict(q, flags=f)) for f in ((q["flags"], q["flags"] ^ 1) if guard else (q["flags"],))}
    d = wants[q["flags"]][1]
    print(f"{label}: {image.shape[1]} x {image.shape[0]} image {np.bincount(image.ravel().astype(int) + 1, minlength=102)[[0, 1, 101]].tolist()} "
          f"table {len(wants[q['flags']][2])} largest dist2 {int(d[d != cr.DIST_NONE].max()) if (d != cr.DIST_NONE).any() else None}")
    if guard:
        plain, unknown = wants[q["flags"] & ~1], wants[q["flags"] | 1]
        cr.guards(image, plain[0], unknown[0], plain[1], plain[2])
    for f, want in wants.items():
        cm.map_cost_configure(q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"], bool(f & 1))
        info = cm.map_cost_update()
        compare(read_cost(cm, info), want, f"{label} flags {f}")
    return image, wants[q["flags"]]


def one_frame(cm, cell, nx, ny, cells, trans, q=Q, label="", guard=False, exact=True):
    tm.configure(cm, map_q(cell, nx, ny))
    tg.run_frame(cm, frame_of(cells, cell, nx, ny, trans), PARAMS)
    cm.map_integrate(None)
    return check(cm, cell, q, label or f"{nx} x {ny}", cells if exact else None, guard)


def edge_cells(nx, ny):
    """Obstacles one below, on and one above every internal block edge of the two kernels: rows around the multiples of ROWS
    (the column pass's words), columns around the multiples of STRIP (the row pass's strips), on a diagonal so that no two
    share a row or a column, and the four corners."""
    ys = [y for e in range(ROWS, ny, ROWS) for y in (e - 1, e, e + 1) if y < ny]
    xs = [x for e in range(STRIP, nx, STRIP) for x in (e - 1, e, e + 1) if x < nx]
    out = {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)}
    out |= {((7 * k + 3) % nx, y) for k, y in enumerate(ys)}
    out |= {(x, (5 * k + 2) % ny) for k, x in enumerate(xs)}
    return sorted(out)


def border_cells(nx, ny):
    return sorted({(x, y) for x in range(nx) for y in (0, ny - 1)} | {(x, y) for y in range(ny) for x in (0, nx - 1)})


def scattered(seed, nx, ny, n):
    rng = np.random.default_rng(seed)
    return sorted(set(zip(rng.integers(0, nx, n).tolist(), rng.integers(0, ny, n).tolist())))


CORNERS_64_48 = [(2, 2), (61, 3), (5, 44), (60, 45), (30, 2)]               # far from the sensor's cell (32, 24): rays through open space
SEQ = (96, 64, 0.1, [(0.0, 0.0), (1.25, -0.35), (3.05, 0.95)])              # the three-frame sequence: window, cell, poses


def seq_cells(k):
    """The obstacles stay where they are in the world (the first frame's window cells) while the vehicle moves."""
    nx, ny, cell, poses = SEQ
    sx, sy = (math.floor(float(F32(p) * (F32(1.0) / F32(cell)))) for p in poses[k])
    return [(x - sx, y - sy) for x, y in scattered(17, nx, ny, 25) if 0 <= x - sx < nx and 0 <= y - sy < ny], (sx, sy)


def named_cases():
    """(label, cell, nx, ny, [(cells, pose_xy) per frame]): the cases that assert the guards on the GPU, all with the sensor inside."""
    out = [("257 x 255", 0.1, 257, 255, [(sorted(set(edge_cells(257, 255)) | set(scattered(5, 257, 255, 40))), (0.0, 0.0))]),
           ("515 x 70", 0.1, 515, 70, [(edge_cells(515, 70), (0.0, 0.0))]), ("70 x 515", 0.1, 70, 515, [(edge_cells(70, 515), (0.0, 0.0))]),
           ("64 x 48", 0.1, 64, 48, [(CORNERS_64_48, (0.0, 0.0))])]
    nx, ny, cell, poses = SEQ
    out.append(("sequence", cell, nx, ny, [(seq_cells(k)[0], xy) for k, xy in enumerate(poses)]))
    return out


def test_the_named_cases_satisfy_the_guards():
    """On the CPU, with the image of tests/map_ref.py's restatement of the map in place of the library's."""
    trans = (0.0, 0.0, 0.0)
    for label, cell, nx, ny, frames in named_cases():
        ref = mr.MapVectorised(map_q(cell, nx, ny))
        for cells, xy in frames:
            d = frame_of(cells, cell, nx, ny, trans, xy)[0].data
            A = np.stack([d["x"], d["y"], d["z"], d["intensity"]], axis=1).astype(F32)          # (the translation is zero)
            none = np.zeros(0, np.int64)
            _, image, _ = ref.integrate(A, tm.NO_G, np.zeros(len(A), np.int64), none, [trans], tm.pose_t(*xy))
            want = np.zeros(image.shape, bool)
            want[[y for _, y in cells], [x for x, _ in cells]] = True
            assert ((image == 100) == want).all(), label
            plain, unknown = restate(image, cell, Q), restate(image, cell, dict(Q, flags=1))
            cr.guards(image, plain[0], unknown[0], plain[1], plain[2])


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_by_one_with_and_without_an_obstacle():
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        image, (cost, dist2, _) = one_frame(cm, 0.1, 1, 1, [(0, 0)], OUTSIDE)
        assert cost.tolist() == [[254]] and dist2.tolist() == [[0]]
        image, (cost, dist2, _) = one_frame(cm, 0.1, 1, 1, [], OUTSIDE)
        assert cost.tolist() == [[255]] and dist2.tolist() == [[cr.DIST_NONE]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(70, 1), (1, 70), (65, 33)])
def test_small_shapes_and_placements(shape):
    nx, ny = shape
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        for name, cells in (("none", []), ("all", [(x, y) for y in range(ny) for x in range(nx)]), ("border", border_cells(nx, ny)),
                            ("edges", edge_cells(nx, ny)), ("scattered", scattered(3, nx, ny, 6))):
            for trans in (OUTSIDE, (0.0, 0.0, 0.0)):
                one_frame(cm, 0.1, nx, ny, cells, trans, label=f"{nx} x {ny} {name} {'outside' if trans is OUTSIDE else 'inside'}")


@pytest.mark.gpu
def test_257_by_255_named_case_holds_every_guard():
    """Odd, and wider than one strip of the row pass. The sensor inside the window gives free cells; both flag settings."""
    nx, ny = 257, 255
    cells = sorted(set(edge_cells(nx, ny)) | set(scattered(5, nx, ny, 40)))
    with capi.CloudMerger(max_points_total=nx * ny, max_sensors=1) as cm:
        one_frame(cm, 0.1, nx, ny, cells, (0.0, 0.0, 0.0), label="257 x 255 inside", guard=True)
        one_frame(cm, 0.1, nx, ny, border_cells(nx, ny), OUTSIDE, label="257 x 255 border")
        one_frame(cm, 0.1, nx, ny, [(x, y) for y in range(ny) for x in range(nx)], OUTSIDE, label="257 x 255 all")
        one_frame(cm, 0.1, nx, ny, [], OUTSIDE, label="257 x 255 none")


@pytest.mark.gpu
def test_block_edges_of_both_kernels():
    """515 x 70: two internal strip edges along x (256, 512), two internal word edges along y (32, 64); then the transpose."""
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        for nx, ny in ((515, 70), (70, 515)):
            cells = edge_cells(nx, ny)
            assert {x for x, _ in cells} >= {e + d for e in range(STRIP, nx, STRIP) for d in (-1, 0, 1) if e + d < nx}
            assert {y for _, y in cells} >= {e + d for e in range(ROWS, ny, ROWS) for d in (-1, 0, 1) if e + d < ny}
            one_frame(cm, 0.1, nx, ny, cells, OUTSIDE, label=f"{nx} x {ny} edges outside")
            one_frame(cm, 0.1, nx, ny, cells, (0.0, 0.0, 0.0), label=f"{nx} x {ny} edges inside", guard=True)
            # a single obstacle at a time just beside an edge: every other cell's nearest obstacle is across it
            for cell_xy in ((STRIP, ROWS), (STRIP - 1, ROWS - 1)) if nx > ny else ((ROWS, STRIP), (ROWS - 1, STRIP - 1)):
                one_frame(cm, 0.1, nx, ny, [cell_xy], OUTSIDE, label=f"{nx} x {ny} single {cell_xy}")


@pytest.mark.gpu
def test_2048_by_2048_with_a_single_obstacle_in_one_corner():
    n = 2048
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, map_q(0.02, n, n))
        tg.run_frame(cm, frame_of([(n - 1, 0)], 0.02, n, n, OUTSIDE), PARAMS)
        cm.map_integrate(None)
        image, _ = cm.map_occupancy()
        assert (image == 100).sum() == 1 and image[0, n - 1] == 100
        q = cr.params(0.1, 0.5, 2.0)
        xs, ys = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
        d = ((xs[None, :] - (n - 1)) ** 2 + ys[:, None] ** 2).astype(np.uint32)               # the whole transform in closed form
        assert d[n - 1, 0] == 2 * 2047 ** 2 == d.max()
        lut = cr.table(0.02, q)
        for f in (0, 1):
            cm.map_cost_configure(q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"], bool(f))
            info = cm.map_cost_update()
            compare(read_cost(cm, info), (cr.cost_of(image, d, lut, f), d, lut), f"corner flags {f}")


@pytest.mark.gpu
def test_2048_by_2048_with_a_few_hundred_obstacles():
    n = 2048
    cells = sorted(set(scattered(9, n, n, 150)) | set(edge_cells(n, n)[:60]))
    assert 150 < len(cells) < 400
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, map_q(0.02, n, n))
        tg.run_frame(cm, frame_of(cells, 0.02, n, n, (0.0, 0.0, 0.0)), PARAMS)
        cm.map_integrate(None)
        check(cm, 0.02, cr.params(0.1, 0.5, 2.0), "2048 x 2048", cells)


@pytest.mark.gpu
def test_parameter_cases():
    nx, ny = 129, 67
    cells = sorted(set(scattered(13, nx, ny, 12)) | {(0, 0), (nx - 1, ny - 1)})
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, map_q(0.1, nx, ny))
        tg.run_frame(cm, frame_of(cells, 0.1, nx, ny, (0.0, 0.0, 0.0)), PARAMS)
        cm.map_integrate(None)
        for name, q in (("R = 0", cr.params(0.0, 0.0, 3.0)), ("R = 256", cr.params(0.3, 25.6, 0.25)), ("no decay", cr.params(0.35, 1.05, 0.0)),
                        ("no inscribed radius", cr.params(0.0, 1.05, 3.0)), ("inscribed = inflation", cr.params(0.7, 0.7, 3.0))):
            for f in (0, 1):
                image, (cost, dist2, lut) = check(cm, 0.1, dict(q, flags=f), f"{name} flags {f}", cells)
            if name == "R = 0":
                assert len(lut) == 1 and set(np.unique(cost).tolist()) == {0, 254, 255}
            if name == "R = 256":
                assert len(lut) == 65537 and (dist2 <= 65536).all()
            if name == "no decay":
                assert set(np.unique(cost[image == 0]).tolist()) <= {0, 252, 253} and (cost == 252).any()
            if name == "no inscribed radius":
                assert not (cost == 253).any()


@pytest.mark.gpu
def test_a_three_frame_sequence_with_a_scroll():
    """The obstacles stay where they are in the world while the vehicle moves: the window scrolls and forgets what leaves it."""
    nx, ny, cell, poses = SEQ
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm, capi.CloudMerger(max_points_total=4096, max_sensors=1) as never:
        for c in (cm, never):
            tm.configure(c, map_q(cell, nx, ny))
        cm.map_cost_configure(Q["inscribed_radius"], Q["inflation_radius"], Q["cost_scaling"])
        counts = []
        for k, xy in enumerate(poses):
            cells, (sx, sy) = seq_cells(k)
            outs = []
            for c in (cm, never):
                res = tg.run_frame(c, frame_of(cells, cell, nx, ny, (0.0, 0.0, 0.0), xy), PARAMS)
                outs.append((res.n_out, res.path_flags, c.result(res.n_out).tobytes(), c.merged(4096).tobytes()))
            assert outs[0] == outs[1]                  # the frame behind an update: that of a context that never had a layer
            P = tm.pose_t(xy[0], xy[1])
            infos = [tm.info_tuple(c.map_integrate(P)) for c in (cm, never)]
            assert infos[0] == infos[1] and infos[0][0] == (sx - nx // 2, sy - ny // 2)
            check(cm, cell, Q, f"frame {k}", cells, guard=True)
            # state table, image and info of the map: those of the context without a cost layer
            assert cm.map()[0].tobytes() == never.map()[0].tobytes() and cm.map_occupancy()[0].tobytes() == never.map_occupancy()[0].tobytes()
            assert tm.info_tuple(cm.map()[1]) == tm.info_tuple(never.map()[1])
            counts.append(len(cells))
        assert counts[0] > counts[2] > 0               # the scroll dropped obstacles


@pytest.mark.gpu
def test_staleness_lifetime_and_an_update_before_any_integration():
    nx, ny, cell = 64, 48, 0.1
    cells = CORNERS_64_48
    grid = ((-3.2, -2.4), 0.1, 64, 48)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        tm.configure(cm, map_q(cell, nx, ny))
        cm.map_cost_configure(0.35, 1.05, 3.0)
        assert cm.map_cost_table().tobytes() == cr.table(cell, Q).tobytes()                   # the table needs no update
        tm.refused(cm, cm.map_cost, text=b"stale")
        tm.refused(cm, cm.map_cost_device, text=b"cm_map_cost_configure")                      # ... which names the reason
        info = cm.map_cost_update()                    # before any integration: the image is all -1
        cost, dist2, _ = cm.map_cost()
        assert tm.info_tuple(info) == ((0, 0), nx, ny, 0, 0, 0) and (cost == 255).all() and (dist2 == cr.DIST_NONE).all()
        tg.run_frame(cm, frame_of(cells, cell, nx, ny, (0.0, 0.0, 0.0)), PARAMS)
        cost, dist2, _ = cm.map_cost()                 # a merge leaves the layer alone
        assert (cost == 255).all()
        cm.map_integrate(None)
        tm.refused(cm, cm.map_cost, text=b"cm_map_integrate")
        tm.refused(cm, cm.map_cost_device, text=b"stale")
        L = cm._lib
        buf = np.full(nx * ny, 7, np.uint32)
        assert L.cm_map_dist_copy(cm._ctx, buf.ctypes.data, nx * ny, None) == capi.BAD_ARG and (buf == 7).all()
        image, want = check(cm, cell, Q, "after the first integration", cells, guard=True)
        before = read_cost(cm, cm.map_cost_update())
        # merges, grid and ray calls: the tables stay, and stay readable
        tg.run_frame(cm, frame_of(cells[:2], cell, nx, ny, (0.0, 0.0, 0.0)), PARAMS)
        cm.grid_map(*grid)
        cm.grid_rays(*grid)
        after = read_cost(cm, cm.map()[1])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # cm_map_configure, in either form, frees the layer
        tm.configure(cm, map_q(cell, nx, ny))
        tm.refused(cm, cm.map_cost_update, text=b"cm_map_cost_configure")
        tm.refused(cm, cm.map_cost_table, text=b"cm_map_cost_configure")
        cm.map_cost_configure(0.35, 1.05, 3.0)
        cm.map_configure(None)
        tm.refused(cm, cm.map_cost_update, text=b"cm_map_configure")
        tm.refused(cm, cm.map_cost_configure, 0.35, 1.05, 3.0, text=b"cm_map_configure")
        cm.map_cost_configure(None)                    # freeing what is not there is fine


@pytest.mark.gpu
def test_refusals_and_capacity():
    nx, ny, cell = 16, 8, 0.5
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        ok = cr.params(0.35, 1.05, 3.0)
        configure = lambda q: cm.map_cost_configure(q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"], False)
        tm.refused(cm, configure, ok, text=b"cm_map_configure")                                # no map
        tm.refused(cm, cm.map_cost_update, text=b"cm_map_configure")
        tm.refused(cm, cm.map_cost)
        tm.refused(cm, cm.map_cost_device)
        tm.refused(cm, cm.map_cost_table)
        tm.configure(cm, map_q(cell, nx, ny))
        tm.refused(cm, cm.map_cost_update, text=b"cm_map_cost_configure")                      # a map, no layer
        L = cm._lib
        for kw in REFUSED_PARAMS:                      # every refusal of the restatement's validator is the library's
            q = dict(ok, **kw)
            assert cr.refusal(q, cell, nx, ny) is not None
            p = capi.CostParams(float(F32(q["inscribed_radius"])), float(F32(q["inflation_radius"])), float(F32(q["cost_scaling"])), q["flags"])
            assert L.cm_map_cost_configure(cm._ctx, C.byref(p)) == capi.BAD_ARG and L.cm_last_error(cm._ctx), kw
        tm.refused(cm, cm.map_cost_update, text=b"cm_map_cost_configure")                      # a refused call configured nothing
        for q in (ok, cr.params(0.0, 0.0, 0.0), cr.params(1.05, 1.05, 3.0), cr.params(0.0, 128.0, 0.0), dict(ok, flags=1)):
            assert cr.refusal(q, cell, nx, ny) is None
            cm.map_cost_configure(q["inscribed_radius"], q["inflation_radius"], q["cost_scaling"], bool(q["flags"]))
            assert cm.map_cost_table().tobytes() == cr.table(cell, q).tobytes()
        # a window wider or taller than CM_COST_MAX_AXIS cells (dist2 would not fit): the map takes it, the layer does not
        for wide in ((2049, 1), (1, 4096)):
            tm.configure(cm, map_q(cell, *wide))
            assert cr.refusal(ok, cell, *wide) == "axis"
            tm.refused(cm, configure, ok, text=b"CM_COST_MAX_AXIS")
        tm.configure(cm, map_q(cell, nx, ny))
        configure(ok)
        tg.run_frame(cm, frame_of([(3, 2)], cell, nx, ny, OUTSIDE), PARAMS)
        cm.map_integrate(None)
        info = cm.map_cost_update()
        cost, dist2, _ = cm.map_cost()
        lut = cm.map_cost_table()
        # destinations that are too small: CM_CAPACITY, nothing copied, the info or n still written
        n = nx * ny
        bc, bd, bt = np.full(n, 7, np.uint8), np.full(n, 7, np.uint32), np.full(len(lut), 7, np.uint8)
        for cap in (n - 1, 0):
            got, cnt = capi.MapInfo(), C.c_uint64(0)
            assert L.cm_map_cost_copy(cm._ctx, bc.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (bc == 7).all()
            assert tm.info_tuple(got) == tm.info_tuple(info)
            got = capi.MapInfo()
            assert L.cm_map_dist_copy(cm._ctx, bd.ctypes.data, cap, C.byref(got)) == capi.CAPACITY and (bd == 7).all()
            assert tm.info_tuple(got) == tm.info_tuple(info)
            assert L.cm_map_cost_table_copy(cm._ctx, bt.ctypes.data, min(cap, len(lut) - 1), C.byref(cnt)) == capi.CAPACITY and (bt == 7).all()
            assert cnt.value == len(lut)
        assert L.cm_map_cost_copy(cm._ctx, bc.ctypes.data, n, None) == capi.OK and bc.tobytes() == cost.tobytes()
        assert L.cm_map_dist_copy(cm._ctx, bd.ctypes.data, n + 5, None) == capi.OK and bd.tobytes() == dist2.tobytes()
        assert L.cm_map_cost_table_copy(cm._ctx, bt.ctypes.data, len(lut), None) == capi.OK and bt.tobytes() == lut.tobytes()
        assert L.cm_map_cost_copy(cm._ctx, None, n, None) == capi.BAD_ARG                     # no destination
        pc = C.c_void_p()
        assert L.cm_map_cost_device(cm._ctx, C.byref(pc), None, None) == capi.OK and pc.value  # either pointer may be NULL
        # a frame in flight
        cm.submit_all(frame_of([(3, 2)], cell, nx, ny, OUTSIDE))
        cm.merge_voxelize_async(capi.make_params(PARAMS))
        tm.refused(cm, configure, ok, text=b"flight")
        tm.refused(cm, cm.map_cost_update, text=b"flight")
        tm.refused(cm, cm.map_cost, text=b"flight")
        tm.refused(cm, cm.map_cost_device, text=b"flight")
        tm.refused(cm, cm.map_cost_table, text=b"flight")
        assert cm.wait().status == capi.OK
        assert cm.map_cost()[0].tobytes() == cost.tobytes()                                   # none of it touched the tables


@pytest.mark.gpu
def test_stage_names_under_profile():
    nx, ny, cell = 40, 24, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        tm.configure(cm, map_q(cell, nx, ny))
        cm.map_cost_configure(0.35, 1.05, 3.0)
        sensors = frame_of([(3, 2)], cell, nx, ny, OUTSIDE)
        tg.run_frame(cm, sensors, PARAMS)
        cm.map_integrate(None)
        assert not any("cost" in n for n, _ in cm.stage_times())
        cm.map_cost_update()
        names = [n for n, _ in cm.stage_times()]
        assert names == ["k_cost_colmask", "k_cost_colcarry", "k_cost_rows"], names
        assert all(ms >= 0.0 for _, ms in cm.stage_times())
        tg.run_frame(cm, sensors, PARAMS)               # a frame's own list never holds the call's stages
        assert not any("cost" in n for n, _ in cm.stage_times())


# ---- no update call allocates: the counts of the test build, as tests/test_ctx_memory.py takes them ---------------------------
def case_no_update_allocates():
    nx, ny, cell = 96, 64, 0.1
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        tm.configure(cm, map_q(cell, nx, ny))
        before = capi.device_allocations()
        cm.map_cost_configure(0.35, 1.05, 3.0)        # every buffer of the layer is taken here:
        after = capi.device_allocations()
        assert [a - b for a, b in zip(after, before)] == [4, 4]        # cost, dist2, the column pass's tables, the cost table
        totals = []
        for k in range(4):
            if k:
                tg.run_frame(cm, frame_of(scattered(23 + k, nx, ny, 9), cell, nx, ny, (0.0, 0.0, 0.0)), PARAMS)
                cm.map_integrate(tm.pose_t(0.0, 0.0))
            b = capi.device_allocations()
            cm.map_cost_update()                       # (k = 0: before any integration)
            cm.map_cost()
            cm.map_cost_device()
            cm.map_cost_table()
            a = capi.device_allocations()
            print(f"update {k}: before {b} after {a}")
            totals.append((b, a))
        assert all(b == a for b, a in totals), totals
        live = capi.device_allocations()[0]
        cm.map_cost_configure(None)
        assert capi.device_allocations()[0] == live - 4
        cm.map_cost_configure(0.35, 1.05, 3.0)
        cm.map_configure(None)                         # the map takes its layer with it
        assert capi.device_allocations()[0] == live - 4 - 5


@pytest.mark.gpu
def test_no_update_call_allocates():
    assert os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")), "the test build is missing"
    env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK")}
    env.update(CM_LIB_VARIANT="testhooks", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_map_cost", "no_update_allocates"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    {"no_update_allocates": case_no_update_allocates}[sys.argv[1]]()
