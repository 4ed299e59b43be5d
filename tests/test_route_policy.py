"""The route policy (cloud_merger_amd/csrc/cm_route.cpp) on the CPU: the file is built with a small driver that reads one
command per line and prints what the policy decided. The expected values are the policy's arithmetic: global pass counts,
the quantile passes' rests, the back-offs after a hand-back and the predicted box's margins."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cloud_merger_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "cm_route.hpp"

static RouteState rt;
static FramePlan pl;
static CmFrameDev f;

static void frame(uint32_t n_in) {
    std::memset(&f, 0, sizeof f);
    f.n_tiles = (n_in + CM_TILE - 1) / CM_TILE;
    f.n_padded = f.n_tiles * CM_TILE;
}

static void counters() {
    std::printf(" extra=%u good=%u retry=%u v2_off=%u pre_off=%u pre_backoff=%u shrink=%u quant_off=%u quant_hist=%u"
                " quant_rest=%u quant_good=%u arm=%u lds=%d misrank=%d pred_ok=%d\n", rt.v2_extra_passes, rt.v2_good_frames,
                rt.v2_retry_after, rt.v2_off_frames, rt.pre_bucket_off, rt.pre_bucket_backoff, rt.grid_shrink_off,
                rt.quant_off_frames, rt.quant_hist, rt.quant_rest, rt.quant_good, rt.quant_big_arm, rt.lds_rank ? 1 : 0,
                rt.debug_misrank, rt.pred.ok ? 1 : 0);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "passes") {                       // kb est extra
            uint32_t kb, extra; uint64_t est;
            in >> kb >> est >> extra;
            std::printf("%u\n", bucket_passes(kb, est, extra));
        } else if (cmd == "set") {                   // name value
            std::string k; uint64_t v;
            in >> k >> v;
            if (k == "extra") rt.v2_extra_passes = v;
            else if (k == "retry") rt.v2_retry_after = v;
            else if (k == "last_n_merged") rt.last_n_merged = v;
            else if (k == "lds") rt.lds_rank = v != 0;
            else if (k == "finish_v2") rt.finish_v2 = v != 0;
            else if (k == "misrank") rt.debug_misrank = static_cast<int>(v);
            else if (k == "pred_ok") rt.pred.ok = v != 0;
            else return 2;
        } else if (cmd == "settle") {                // bucket quant measured redone err outside
            int b, q, m, r; uint32_t err, outside;
            in >> b >> q >> m >> r >> err >> outside;
            pl.bucket = b; pl.quant = q; pl.measured = m; pl.redone = r;
            CmFrameState h;
            std::memset(&h, 0, sizeof h);
            h.err = err; h.outside = outside;
            const Replay how = rt.settle(pl, h);
            std::printf("replay=%d err=%u", static_cast<int>(how), h.err);
            counters();
        } else if (cmd == "quant_done") {            // redone quant_big: a quantile frame that finished and left splitters
            int r; uint32_t big;
            in >> r >> big;
            FramePlan p;
            p.bucket = true; p.quant = true; p.redone = r;
            CmFrameState h;
            std::memset(&h, 0, sizeof h);
            h.status = CM_OK; h.n_valid = 1000; h.quant_big = big;
            rt.adopt(p, h, f, false);
            std::printf("spl_valid=%d", rt.spl_valid ? 1 : 0);
            counters();
        } else if (cmd == "plan") {                  // n_in spl_n: a frame in a crop box whose grid the splitters were cut in
            uint32_t n_in, spl_n;
            in >> n_in >> spl_n;
            frame(n_in);
            pl = FramePlan();
            pl.params.crop_enable = 1;
            const float lo[3] = {-50.f, -50.f, -2.f}, hi[3] = {50.f, 50.f, 6.f};
            for (int a = 0; a < 3; ++a) {
                pl.params.crop_min[a] = lo[a]; pl.params.crop_max[a] = hi[a]; pl.params.leaf[a] = 0.05f;
                f.crop_min[a] = lo[a]; f.crop_max[a] = hi[a]; f.inv_leaf[a] = 1.0f / 0.05f;
            }
            f.crop_enable = 1;
            pl.grid_mode = box_grid(lo, hi, f.inv_leaf, &pl.key_bits) ? 1 : 0;
            box_grid(lo, hi, f.inv_leaf, &pl.key_bits, rt.spl_min_b, rt.spl_div_b);
            std::memcpy(rt.spl_inv_leaf, f.inv_leaf, sizeof rt.spl_inv_leaf);
            rt.spl_n = spl_n;
            const float inv_cell[3] = {0, 0, 0};
            rt.plan(pl, f, nullptr, inv_cell, spl_n != 0, n_in, 1u << 22);
            std::printf("bucket=%d quant=%d g=%u low=%u nb=%u big=%d nt_later=%u k3=%d", pl.bucket, pl.quant, pl.g, pl.low, pl.nb,
                        pl.big_armed, pl.nt_later, pl.k3);
            counters();
        } else if (cmd == "fixed") {                 // n_in: a fixed-grid launch in the crop box
            uint32_t n_in;
            in >> n_in;
            frame(n_in);
            f.crop_enable = 1;
            pl = FramePlan();
            pl.b_grid_mode = 1;
            rt.size_fixed_grid(pl, f, n_in);
            std::printf("nt_later=%u pack=%d sparse=%d k3=%d", pl.nt_later, pl.pack, pl.sparse, pl.k3);
            counters();
        } else if (cmd == "sorcell") {               // requested last_mean row_cap|crop|bounds min xyz max xyz
            // (tokens through strtod: "nan" and "inf" parse; key_bits starts at 99 so an unwritten one shows)
            std::string tok[9];
            for (auto& t : tok) in >> t;
            const float req = std::strtof(tok[0].c_str(), nullptr);
            const double mean = std::strtod(tok[1].c_str(), nullptr);
            float mn[3], mx[3];
            for (int a = 0; a < 3; ++a) {
                mn[a] = std::strtof(tok[3 + a].c_str(), nullptr);
                mx[a] = std::strtof(tok[6 + a].c_str(), nullptr);
            }
            const float c0 = sor_cell(req, mean);
            float cell = c0;
            uint32_t kb = 99;
            int gm = -1;
            if (tok[2] == "crop") {
                cm_params p;
                std::memset(&p, 0, sizeof p);
                p.crop_enable = 1;
                for (int a = 0; a < 3; ++a) { p.crop_min[a] = mn[a]; p.crop_max[a] = mx[a]; }
                gm = sor_crop_grid(p, &cell, &kb);
            } else if (tok[2] == "bounds") {
                cell = sor_bounds_cell(c0, mn, mx, &kb);
                for (int a = 0; a < 3; ++a) { mn[a] -= c0; mx[a] += c0; }
            } else {
                cell = sor_fit_cell(c0, mn, mx, static_cast<uint32_t>(std::strtoul(tok[2].c_str(), nullptr, 10)), &kb);
            }
            // the fitted grid's rows ((y,z) cell pairs) and cells along x
            unsigned long long rows = 0, nx = 0;
            if (cell > 0.0f) {
                const float inv = 1.0f / cell, iv[3] = {inv, inv, inv};
                int32_t mb[3], db[3];
                uint32_t kb2 = 0;
                if (box_grid(mn, mx, iv, &kb2, mb, db)) {
                    rows = static_cast<unsigned long long>(db[1]) * static_cast<unsigned long long>(db[2]);
                    nx = static_cast<unsigned long long>(db[0]);
                }
            }
            std::printf("%.9g %.9g %u %llu %llu %d\n", c0, cell, kb, rows, nx, gm);
        } else if (cmd == "box" || cmd == "update") {   // min xyz, max xyz, leaf xyz
            float mn[3], mx[3], leaf[3];
            for (float& v : mn) in >> v;
            for (float& v : mx) in >> v;
            for (float& v : leaf) in >> v;
            if (cmd == "box") rt.set_predicted_box(mn, mx, leaf);
            else rt.update_predicted_box(mn, mx, leaf);
            std::printf("%d %.9g %.9g %.9g %.9g %.9g %.9g\n", rt.pred.ok ? 1 : 0, rt.pred.min[0], rt.pred.min[1], rt.pred.min[2],
                        rt.pred.max[0], rt.pred.max[1], rt.pred.max[2]);
        } else {
            return 3;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("route")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "route_driver"
    # the library's host flags: no FMA contraction (the box arithmetic must match the device's)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    os.path.join(CSRC, "cm_route.cpp"), str(d / "driver.cpp"), "-o", str(exe)], check=True)

    def run(commands):
        p = subprocess.run([str(exe)], input="\n".join(commands) + "\n", capture_output=True, text=True, check=True)
        return p.stdout.splitlines()
    return run


def fields(line):
    """'replay=3 err=0 extra=1 ...' -> {'replay': 3, ...}"""
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


# kb, est, extra -> global passes
PASSES = [
    (30, 200_000, 0, 2),          # sparse: 14 low bits left to the finish
    (30, 200_000, 1, 3),
    (30, 200_000, 2, 4),
    (30, 200_000, 3, 0),          # beyond CM_MAX_PASSES
    (22, 200_000, 0, 2),          # an average bucket of more than 256 points adds a pass
    (22, 50_000, 0, 1),
    (23, 50_000, 0, 2),           # one bit more than a pass plus CM2_MAX_LOW_BITS
    (20, 100_000_000, 0, 3),      # dense: (est >> kb) >= 1, the whole index sorted globally
    (24, 20_000_000, 0, 3),
    (24, 16_777_216, 0, 3),
    (24, 16_777_215, 0, 2),
    (26, 20_000_000, 0, 3),       # sparse, but est >> 16 > 256 adds a pass
    (8, 100, 1, 0),               # nothing left for the finish
    (9, 100, 1, 2),
    (32, 0, 0, 3),
]


def test_bucket_passes(driver):
    out = driver([f"passes {kb} {est} {extra}" for kb, est, extra, _ in PASSES])
    assert [int(v) for v in out] == [want for *_, want in PASSES]


def test_quantile_rest_doubles_to_128_and_resets_after_16_good(driver):
    cmds, rests = [], []
    # five rounds of three hand-backs in a row: each starts a rest, 8, 16, 32, 64, 128 frames, then the cap
    for _ in range(6):
        cmds += ["settle 1 1 0 0 7 0"] * 3
    out = [fields(l) for l in driver(cmds)]
    assert all(o["replay"] == 1 for o in out)                  # Replay::fixed_grid
    assert all(o["arm"] == 16 for o in out)                     # every hand-back arms the large shape
    rests = [o["quant_off"] for o in out[2::3]]
    assert rests == [8, 16, 32, 64, 128, 128]
    assert [o["quant_hist"] for o in out[:3]] == [1, 3, 0]
    # 16 good attempts bring the next rest back to 8; a redone frame is not an attempt
    out = [fields(l) for l in driver(cmds + ["quant_done 1 0"] + ["quant_done 0 0"] * 16 + ["settle 1 1 0 0 7 0"] * 3)]
    assert out[len(cmds)]["quant_good"] == 0 and out[len(cmds)]["quant_rest"] == 128
    assert [o["quant_good"] for o in out[len(cmds) + 1:len(cmds) + 17]] == list(range(1, 17))
    assert out[len(cmds) + 16]["quant_rest"] == 8
    assert out[-1]["quant_off"] == 8 and out[-1]["quant_rest"] == 16


def test_quantile_three_in_the_last_eight(driver):
    # F G G G G G F F: the third hand-back within eight attempts starts a rest
    out = [fields(l) for l in driver(["settle 1 1 0 0 7 0"] + ["quant_done 0 0"] * 5 + ["settle 1 1 0 0 7 0"] * 2)]
    assert out[-2]["quant_off"] == 0 and out[-1]["quant_off"] == 8
    # F G G G G G G F F: the first one has left the window
    out = [fields(l) for l in driver(["settle 1 1 0 0 7 0"] + ["quant_done 0 0"] * 6 + ["settle 1 1 0 0 7 0"] * 2)]
    assert out[-1]["quant_off"] == 0 and out[-1]["quant_hist"] == 3
    # unsorted or overflowing buckets of a quantile frame are stale splitters too; a box miss is not
    for err, outside, want in ((2, 0, 1), (4, 0, 1), (7, 1, 2), (0, 1, 2)):
        o = fields(driver([f"settle 1 1 0 0 {err} {outside}"])[0])
        assert o["replay"] == want, (err, outside)


def test_quantile_plan_rest_and_large_shape(driver):
    # 200 000 points in a 100 x 100 x 8 m crop box at 5 cm: 30 key bits, two fixed-grid passes, 105 quantile buckets
    out = [fields(l) for l in driver(["plan 200000 200000", "plan 200000 0"])]
    assert (out[0]["bucket"], out[0]["quant"], out[0]["g"], out[0]["low"], out[0]["nb"], out[0]["big"]) == (1, 1, 2, 14, 105, 0)
    assert (out[1]["bucket"], out[1]["quant"], out[1]["nt_later"], out[1]["k3"]) == (1, 0, 49, 1)
    # a hand-back arms the large shape for the next 16 quantile frames; a rest counts down on frames that would take them
    cmds = ["settle 1 1 0 0 7 0"] + ["plan 200000 200000"] * 17
    out = [fields(l) for l in driver(cmds)[1:]]
    assert [o["big"] for o in out] == [1] * 16 + [0]
    assert [o["arm"] for o in out] == list(range(15, -1, -1)) + [0]
    cmds = ["settle 1 1 0 0 7 0"] * 3 + ["plan 200000 200000"] * 9 + ["plan 200000 0"]
    out = [fields(l) for l in driver(cmds)[3:]]
    assert [o["quant"] for o in out] == [0] * 8 + [1, 0]
    assert [o["quant_off"] for o in out] == [7, 6, 5, 4, 3, 2, 1, 0, 0, 0]
    assert [o["arm"] for o in out] == [16] * 8 + [15, 15]      # only quantile launches disarm


def test_bucket_overflow_adds_passes_and_backs_off(driver):
    out = [fields(l) for l in driver(["settle 1 0 0 0 4 0"] * 5)]
    assert [o["replay"] for o in out] == [2] * 5               # Replay::measured_box (the caller falls back to the general path)
    assert [o["extra"] for o in out] == [1, 2, 3, 4, 4]         # capped at CM_MAX_PASSES
    assert [o["retry"] for o in out] == [512, 1024, 2048, 4096, 8192]   # every retry failed at once
    # good frames, on either path, take a pass away after retry_after of them; redone frames do not count
    cmds = ["set extra 2", "set retry 4"] + ["settle 0 0 0 0 0 0"] * 3 + ["settle 1 0 0 1 0 0", "settle 1 0 0 0 0 0"] + \
           ["settle 0 0 0 0 0 0"] * 4
    out = [fields(l) for l in driver(cmds)]
    assert [o["replay"] for o in out] == [0] * 9
    assert [o["good"] for o in out] == [1, 2, 3, 3, 0, 1, 2, 3, 0]
    assert [o["extra"] for o in out] == [2, 2, 2, 2, 1, 1, 1, 1, 0]
    # a failure eight or more good frames after the last one keeps retry_after
    cmds = ["settle 1 0 0 0 4 0"] + ["settle 0 0 0 0 0 0"] * 8 + ["settle 1 0 0 0 4 0"]
    out = [fields(l) for l in driver(cmds)]
    assert (out[-2]["good"], out[-1]["retry"], out[-1]["extra"], out[-1]["good"]) == (8, 512, 2, 0)


def test_outlier_bucket_backoff_doubles(driver):
    out = [fields(l) for l in driver(["settle 1 0 0 0 5 0"] * 3)]
    assert [o["pre_off"] for o in out] == [16, 32, 64]
    assert [o["pre_backoff"] for o in out] == [32, 64, 128]
    assert all(o["extra"] == 0 for o in out)


def test_grid_error_gives_64_frames_of_whole_grids(driver):
    # the last frame kept 20 000 of 1 000 000 points: later passes get ceil((20 000 * 1.5 + 8192) / 4096) = 10 tiles
    out = [fields(l) for l in driver(["set last_n_merged 20000", "fixed 1000000", "settle 1 0 0 0 6 0"] + ["fixed 1000000"] * 65)
           if l.startswith(("nt_later", "replay"))]
    assert (out[0]["nt_later"], out[0]["pack"], out[0]["sparse"]) == (10, 1, 1)
    assert out[1]["replay"] == 2 and out[1]["shrink"] == 64
    assert [o["nt_later"] for o in out[2:]] == [245] * 64 + [10]
    assert [o["shrink"] for o in out[2:5]] == [63, 62, 61]


def test_lookback_turns_the_bucket_path_off(driver):
    out = [fields(l) for l in driver(["settle 1 0 0 0 3 0"] + ["plan 200000 200000"] * 3)]
    assert out[0]["v2_off"] == 0xFFFFFFFF
    assert all(o["bucket"] == 0 for o in out[1:])
    assert out[-1]["v2_off"] == 0xFFFFFFFF - 3


def test_unsorted_demotes_to_ballot_ranking(driver):
    out = [fields(l) for l in driver(["set lds 1", "set finish_v2 1", "set misrank 1", "fixed 100000", "settle 1 0 0 0 2 0",
                                      "fixed 100000"])]
    assert out[0]["k3"] == 0                                    # CM_FINISH=v2 with lane-ordered adds: k2_local
    assert (out[1]["replay"], out[1]["err"], out[1]["lds"], out[1]["misrank"]) == (2, 0, 0, 0)
    assert out[2]["k3"] == 1                                    # k2_local ranks by returning LDS adds only


def test_measured_redo_settles_or_goes_general(driver):
    out = [fields(l) for l in driver(["set pred_ok 1", "settle 1 0 1 1 0 0", "settle 1 0 1 1 0 1", "settle 1 0 1 1 4 0"])]
    assert [o["replay"] for o in out] == [0, 3, 3]
    assert [o["pred_ok"] for o in out] == [1, 0, 0]
    assert all(o["extra"] == 0 for o in out)                    # the redo's own overflow is not counted


def margins(mn, mx, leaf, part=8.0):
    f32 = np.float32
    lo, hi = [], []
    for a in range(3):
        m = max(f32(f32(mx[a]) - f32(mn[a])) / f32(part), f32((8.0 if part <= 8.0 else 2.0)) * f32(leaf[a]))
        lo.append(f32(f32(mn[a]) - m))
        hi.append(f32(f32(mx[a]) + m))
    return lo + hi


def box(line):
    v = line.split()
    return int(v[0]), [np.float32(float(x)) for x in v[1:]]


def test_predicted_box_margins(driver):
    leaf = (0.1, 0.1, 0.1)
    mn, mx = (-10.0, -10.0, -1.0), (10.0, 10.0, 3.0)
    args = lambda a, b: " ".join(str(x) for x in (*a, *b, *leaf))
    ok, b0 = box(driver([f"box {args(mn, mx)}"])[0])
    assert ok == 1 and b0 == margins(mn, mx, leaf)               # max(extent / 8, 8 leaves): 2.5 m in x, y; 0.8 m in z
    # kept while the cloud stays between a quarter and three margins from every face
    for shift, keep in ((0.0, True), (1.25, True), (1.8, True), (2.0, False), (-1.8, True), (-5.5, False)):
        m2, x2 = (mn[0] + shift, mn[1], mn[2]), (mx[0] + shift, mx[1], mx[2])
        out = driver([f"box {args(mn, mx)}", f"update {args(m2, x2)}"])
        ok, b1 = box(out[1])
        assert ok == 1
        assert (b1 == b0) == keep, shift
        if not keep:
            assert b1 == margins(m2, x2, leaf)
    # a cloud that shrank to a tenth: the box is far too large, and redone around it
    small = ((-1.0, -1.0, -0.1), (1.0, 1.0, 0.3))
    ok, b1 = box(driver([f"box {args(mn, mx)}", f"update {args(*small)}"])[1])
    assert b1 == margins(*small, leaf)
    # without a box, update_predicted_box makes one
    ok, b1 = box(driver([f"update {args(mn, mx)}"])[0])
    assert ok == 1 and b1 == b0


# ---- the statistical outlier stage's search grid (sor_cell, sor_fit_cell, sor_crop_grid, sor_bounds_cell) --------------
ROW_CAP = 1 << 22                                                # CM_ROW_TABLE_CAP (cm_device.h)


def sorcell(driver, cmds):
    """'sorcell req mean cap|crop|bounds mn.. mx..' -> (requested cell, fitted cell, key bits, rows, cells in x, grid mode)"""
    out = []
    for line in driver(["sorcell " + c for c in cmds]):
        v = line.split()
        out.append((np.float32(float(v[0])), np.float32(float(v[1])), int(v[2]), int(v[3]), int(v[4]), int(v[5])))
    return out


def fit_model(cell, mn, mx, cap):
    """sor_fit_cell restated in numpy fp32: (cell, key bits, rows) of the first doubling whose grid fits, (0, None, 0)
    when the cell reaches +inf first."""
    f32 = np.float32
    cell = f32(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        while np.isfinite(cell):
            inv = f32(1.0) / cell
            ext = [f32(f32(f32(mx[a]) - f32(mn[a])) * inv) for a in range(3)]
            if all(e < f32(2.0 ** 31) and e >= 0 for e in ext):
                lo = [int(np.floor(f32(f32(mn[a]) * inv))) for a in range(3)]
                hi = [int(np.floor(f32(f32(mx[a]) * inv))) for a in range(3)]
                div = [h - l + 1 for l, h in zip(lo, hi)]
                d = [int(e) + 1 for e in ext]
                cells = div[0] * div[1] * div[2]
                if d[0] * d[1] * d[2] <= 2 ** 31 - 1 and cells <= 2 ** 32 - 1 and div[1] * div[2] <= cap and max(div) < 2 ** 24:
                    return cell, max(1, (cells - 1).bit_length()), div[1] * div[2]
            cell = f32(cell * f32(2.0))
    return f32(0.0), None, 0


def test_sor_cell_choice(driver):
    # (requested, last frame's mean) -> cell: a request is taken as it is; else the mean clamped to [0.05, 5], 0.5 without one
    cases = [(0, "nan", 0.5), (0, "inf", 0.5), (0, "-inf", 0.5), (0, 0, 0.5), (0, -1, 0.5), (0, 1e-30, 0.05), (0, 0.3, 0.3),
             (0, 1e6, 5.0), (0.7, 1e6, 0.7), (1e-6, "nan", 1e-6), (1e3, 0.1, 1e3)]
    got = sorcell(driver, [f"{r} {m} {ROW_CAP} 0 0 0 1 1 1" for r, m, _ in cases])
    assert [g[0] for g in got] == [np.float32(w) for *_, w in cases]


def test_sor_fit_cell_pins(driver):
    half, quarter = ROW_CAP // 2, ROW_CAP // 4
    got = sorcell(driver, [f"0 nan {half} 0 0 0 1 1 1",
                           f"0 nan {half} -5000 -5000 -5000 5000 5000 5000",
                           f"0 nan {quarter} -5000 -5000 -5000 5000 5000 5000"])
    # [0, 1]^3 at 0.5 m: cells 0..2 per axis, 27 cells (5 bits), 9 rows
    assert got[0][1:5] == (np.float32(0.5), 5, 9, 3)
    # +-5 km: 8 m is the first doubling with at most 2^21 rows (1251^2; 1251^3 cells: 31 bits); 16 m for 2^20 rows (626 per
    # axis: floor(312.5) - floor(-312.5) + 1; 28 bits)
    assert got[1][1:5] == (np.float32(8.0), 31, 1251 ** 2, 1251)
    assert got[2][1:5] == (np.float32(16.0), 28, 626 ** 2, 626)


@pytest.mark.parametrize("cap", [ROW_CAP // 2, ROW_CAP // 4])
def test_sor_fit_cell_boxes(driver, cap):
    boxes = [((0, 0, 0), (1, 1, 1)), ((-20, -20, -5), (20, 20, 5)), ((-5e3,) * 3, (5e3,) * 3), ((-5e29,) * 3, (5e29,) * 3),
             ((1e6, -1e6, 0), (1e6 + 30, -1e6 + 30, 3)), ((-1e38,) * 3, (1e38,) * 3), ((-1.7e38, 0, 0), (1.7e38, 1, 1))]
    over = [((-2e38,) * 3, (2e38,) * 3), ((-3.4e38,) * 3, (3.4e38,) * 3), ((-2e38, -10, -10), (2e38, 10, 10)),
            ((0, 0, -3.4e38), (1, 1, 3.4e38))]
    for req, mean in ((0, "nan"), (0, 1e-30), (0.05, 0), (1e-6, 0), (1e3, 0)):
        cmds = [f"{req} {mean} {cap} " + " ".join(str(v) for v in (*mn, *mx)) for mn, mx in boxes + over]
        got = sorcell(driver, cmds)
        for (mn, mx), g in zip(boxes + over, got):
            cell, kb, rows = fit_model(g[0], mn, mx, cap)
            if (mn, mx) in over:
                # no finite cell fits: 0, key_bits left as it was
                assert (g[1], g[2], g[3]) == (0.0, 99, 0) and kb is None, (mn, mx, g)
            else:
                assert (g[1], g[2], g[3]) == (cell, kb, rows), (req, mean, mn, mx, g, (cell, kb, rows))
                assert 0 < rows <= cap and 1 <= kb <= 32 and g[4] < 2 ** 24
                # the first doubling that fits: half of it (above the request) did not
                if g[1] > g[0]:
                    assert fit_model(g[1] / np.float32(2.0), mn, mx, cap)[0] != g[1] / np.float32(2.0)


def test_sor_search_grid_of_an_overflowing_crop_box(driver):
    """A crop box of +-2e38 or +-FLT_MAX on any axis fits no finite cell: the frame's search grid is then over the cloud's own
    bounds (grid mode 0, the cell untouched), as for a frame without a crop box. A cloud whose own extent overflows fp32 gets
    one cell of +inf (inverse 0); any other cloud a finite cell whose grid fits a quarter of the row table."""
    got = sorcell(driver, ["0 nan crop -20 -20 -5 20 20 5", "0 nan crop -2e38 -20 -5 2e38 20 5",
                           "0 nan crop -20 -20 -2e38 20 20 2e38", "0 nan crop -3.4e38 -3.4e38 -3.4e38 3.4e38 3.4e38 3.4e38",
                           "0 1.5 crop -2e38 -2e38 -2e38 2e38 2e38 2e38", "0 nan crop -1e30 -1e30 -1e30 1e30 1e30 1e30"])
    assert got[0][5] == 1 and got[0][1] == np.float32(0.5) and got[0][2] < 32
    for g in got[1:5]:
        assert g[5] == 0 and g[1] == g[0] and g[2] == 99, g
    assert got[5][5] == 1 and np.isfinite(got[5][1]) and got[5][2] <= 32
    got = sorcell(driver, ["0 nan bounds -3e38 0 0 3e38 1 1", "0 nan bounds 0 0 -3.4e38 1 1 3.4e38",
                           "0 nan bounds -1e38 -1e38 -1e38 1e38 1e38 1e38", "0 nan bounds -20 -20 -5 20 20 5",
                           "0.05 nan bounds 1e6 1e6 1e6 1000010 1000010 1000010"])
    for g in got[:2]:
        assert g[1] == np.inf and g[2] == 99, g
    for g in got[2:]:
        assert np.isfinite(g[1]) and g[2] <= 32 and 0 < g[3] <= ROW_CAP // 4, g
    assert got[3][1] == np.float32(0.5)
