"""tests/ground_ref.py (the ground stage restated in numpy / Python) against the oracle's C++ text of the same
definition, answers for the slab / band rules written out by hand, and the conditions that tests/ground_edge_frames.py's
frames were built for, asserted on the restatement alone. CPU only. tests/test_ground_edges.py then holds the device to
ground_ref on the same frames."""
import collections

import numpy as np
import pytest

from oracle import oracle
from tests import ground_edge_frames as gf
from tests import ground_ref as gr
from tests.ground_ref import BAND, DROPPED, KEPT

F = np.float32


def bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


def cropped(frame):
    """every sensor's cloud as the stage sees it: transformed, finite, inside the crop box (oracle records)"""
    out = []
    for c in frame.sensors:
        pts = oracle.make_points(np.stack([c.data["x"], c.data["y"], c.data["z"]], 1), c.data["intensity"])
        tp = oracle.transform(pts, oracle.quat_to_matrix(c.q_xyzw, c.t_xyz))
        if frame.params.crop_min is not None:
            out.append(oracle.crop(tp, frame.params.crop_min, frame.params.crop_max))
        else:
            out.append(tp[np.isfinite(tp["x"]) & np.isfinite(tp["y"]) & np.isfinite(tp["z"])])
    return out


FRAMES = {f.name: f for f in gf.all_frames() + [gf.special_values_frame(False)]}
_SPLIT = {}


def split(name):
    """[(cloud, keep, ground, planes)] per sensor of a frame by ground_ref, computed once"""
    if name not in _SPLIT:
        f = FRAMES[name]
        _SPLIT[name] = [(cp,) + gr.ground_split(cp, f.zones[s], s, f.gp) for s, cp in enumerate(cropped(f))]
    return _SPLIT[name]


def planes_of(name):
    return [(s, k, pl) for s, (_, _, _, pls) in enumerate(split(name)) for k, pl in enumerate(pls) if pl is not None]


def same_plane_result(a, b):
    return (a.found == b.found and a.iterations == b.iterations and a.n_inliers == b.n_inliers
            and a.best_hypothesis == b.best_hypothesis and bits(list(a.plane)) == bits(list(b.plane)))


# ---- ground_ref against the oracle --------------------------------------------------------------------------------------
SIZES = (3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385, 20000)


def band_points(rng, n, variant, offset):
    xy = rng.uniform(-10, 10, (n, 2))
    xyz = np.column_stack([xy, 0.02 * xy[:, 0] + 0.03 * rng.standard_normal(n)])
    if variant == "clutter":
        m = rng.random(n) < 0.7
        xyz[m, 2] = rng.uniform(-0.5, 0.5, int(m.sum()))
    elif variant == "duplicates":
        xyz[rng.random(n) < 0.6] = xyz[0]
    elif variant == "lattice":
        xyz = np.round(xyz * 4) / 4
    return (xyz + offset).astype(np.float32)


@pytest.mark.parametrize("variant", ["clutter", "duplicates", "lattice"])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_ransac_equals_the_oracle_bit_for_bit(variant, offset):
    rng = np.random.default_rng(len(variant) + int(offset))
    n_found = n_none = 0
    for i, n in enumerate(SIZES):
        xyz = band_points(rng, n, variant, offset)
        pts = oracle.make_points(xyz)
        its = (1, 8, 31, 32, 33, 56, 200) if n < 8000 else (1, 33, 200)
        for max_it in its:
            for optimize in (True, False):
                key = (127, 0, 64 + i, 8 * 15 + i % 8)[(i + max_it) % 4]
                seed = 12345 + 977 * i + max_it
                want, want_mask = oracle.ransac_plane(pts, max_it, 0.05, 0.99, optimize, seed, key)
                got, got_mask = gr.ransac(xyz, max_it, 0.05, 0.99, optimize, seed, key)
                assert same_plane_result(got, want), (n, max_it, optimize, key, got.plane, list(want.plane))
                assert np.array_equal(got_mask, want_mask), (n, max_it, optimize, key)
                n_found += got.found
                n_none += not got.found
    assert n_found >= 100 and (variant != "duplicates" or n_none >= 1)


@pytest.mark.parametrize("name", list(FRAMES))
def test_ground_split_equals_the_oracle_on_every_edge_frame(name):
    f = FRAMES[name]
    for s, (cp, keep, ground, planes) in enumerate(split(name)):
        o_keep, o_ground, o_planes = oracle.ground_split(cp, f.zones[s], s, f.gp)
        assert np.array_equal(keep, o_keep) and np.array_equal(ground, o_ground), (name, s)
        assert len(planes) == len(o_planes) == len(f.zones[s])
        for k, (a, b) in enumerate(zip(planes, o_planes)):
            assert (a is None) == (b is None), (name, s, k)
            if a is not None:
                assert same_plane_result(a, b) and a.band_points == b.band_points, (name, s, k, a.plane, list(b.plane))


def test_sample3_gives_three_distinct_indices_over_the_whole_range():
    for n in (3, 4, 5, 64, 1000):
        seen = set()
        for j in range(400):
            idx = gr.sample3(12345, 127, j, n)
            assert len(set(idx)) == 3 and all(0 <= i < n for i in idx)
            seen.update(idx)
        assert len(seen) >= min(n, 600) * 0.6
    assert gr.sample3(1, 0, 0, 3) != gr.sample3(1, 1, 0, 3) or gr.sample3(1, 0, 1, 3) != gr.sample3(1, 1, 1, 3)


# ---- the slab and band rules, by hand ---------------------------------------------------------------------------------------
def test_classify_known_answers_on_the_border_table():
    up, dn = (lambda v: gf.step(v, 1)), (lambda v: gf.step(v, -1))
    x01, x08 = F(0.1), F(F(0.1) + F(0.7))
    assert float(x08) != 0.8 and x08 == F(0.8)                       # fl(0.1) + fl(0.7) in fp32 is the fp32 nearest 0.8,
    zlo0 = F(0.31)                                                   # and fl32(double(fl(0.3)) + 0.01) the one nearest 0.31
    assert gr.slab_limits(gf.BORDER_ZONES[0])[3] == zlo0 and np.float64(F(0.3)) + 0.01 != np.float64(zlo0)
    cases = [  # x, z, slab, fate
        (x01, 0.0, 0, BAND), (dn(x01), 0.0, -1, DROPPED), (up(x01), 0.0, 0, BAND),          # slab 0's lower limit
        (x08, 0.0, 0, BAND), (up(x08), 0.0, 1, BAND), (up(x08), 1.5, 1, KEPT),              # shared with slab 1: first wins
        (x08, 0.005, 0, BAND), (up(x08), 0.005, 1, DROPPED),                                # (slab 1: gap (0, 0.01))
        (0.6, 0.4, 0, KEPT), (0.5, 0.0, 0, BAND), (0.7, 0.31, 0, KEPT),                     # inside slab 2: slab 0 has them
        (0.3, F(0.3), 0, BAND), (0.3, up(F(0.3)), 0, DROPPED), (0.3, F(-0.3), 0, BAND), (0.3, dn(F(-0.3)), 0, DROPPED),
        (0.3, zlo0, 0, KEPT), (0.3, dn(zlo0), 0, DROPPED), (0.3, 3.0, 0, KEPT), (0.3, up(F(3.0)), 0, DROPPED),
        (1.5, 0.0, 1, BAND), (1.5, -0.0, 1, BAND), (1.5, 1e-45, 1, DROPPED), (1.5, -1e-45, 1, DROPPED),   # zmax 0
        (1.5, F(0.01), 1, KEPT), (1.5, dn(F(0.01)), 1, DROPPED),
        (5.0, 0.0, 3, BAND), (dn(F(5.0)), 0.0, 6, BAND), (up(F(5.0)), 0.0, 7, BAND),        # x_length 0 between 6 and 7
        (5.0, 0.75, 3, KEPT), (up(F(5.0)), 0.75, 7, BAND), (dn(F(5.0)), 0.505, 6, DROPPED),
        (4.5, 0.75, 6, KEPT), (4.0, 0.75, 6, KEPT), (dn(F(4.0)), 1.0, 6, KEPT),             # overlap [4, 5]: slab 6 is first
        (-4.0, -7.0, 4, KEPT), (-2.0, 100.0, 4, KEPT), (up(F(-2.0)), 0.0, -1, DROPPED), (dn(F(-4.0)), 0.0, -1, DROPPED),
        (-10.0, 0.5, 5, BAND), (-10.0, up(F(0.5)), 5, DROPPED), (dn(F(-10.0)), 0.0, -1, DROPPED),
        (-6.0, F(0.51), 5, KEPT), (-6.0, dn(F(0.51)), 5, DROPPED), (up(F(-6.0)), 0.0, -1, DROPPED),
        (-8.0, -0.5, 5, BAND), (-8.0, dn(F(-0.5)), 5, DROPPED),
        (8.0, 1.0, 7, BAND), (up(F(8.0)), 0.0, -1, DROPPED), (6.5, -1.0, 7, BAND), (6.5, dn(F(-1.0)), 7, DROPPED),
        (6.5, F(1.01), 7, KEPT), (6.5, dn(F(1.01)), 7, DROPPED), (6.5, up(F(1.0)), 7, DROPPED),
    ]
    xyz = np.array([(x, 0.0, z) for x, z, _, _ in cases], np.float32)
    slab, fate = gr.classify(xyz, gf.BORDER_ZONES, 3.0)
    for (x, z, want_slab, want_fate), s, f in zip(cases, slab, fate):
        assert (s, f) == (want_slab, want_fate), (float(x), float(z), s, f)
    # and the oracle's composition says the same (one point per case, no band of three: fate from keep / planes)
    pts = oracle.make_points(xyz)
    gp = dict(gf.GP, z_keep_max=3.0)
    keep, ground, planes = oracle.ground_split(pts, gf.BORDER_ZONES, 0, gp)
    assert np.array_equal(keep | ground, fate != DROPPED) and keep[fate == KEPT].all() and not ground[fate == KEPT].any()
    assert [p.band_points if p is not None else None for p in planes] == \
        [int(((slab == k) & (fate == BAND)).sum()) if k != 4 else None for k in range(8)]


def test_ground_split_bookkeeping_of_the_restatement():
    """the oracle ground test's bookkeeping case (tests/test_oracle_ground.py), same answers"""
    xyz = np.array([[5, 0, 0.0], [5, 0, 0.4], [5, 0, 0.505], [5, 0, 0.52], [5, 0, 2.9], [5, 0, 3.1], [10, 0, 0.1],
                    [15, 0, 2.0], [25, 0, 0.0], [40, 0, 0.0]], np.float32)
    gp = dict(max_iterations=10, threshold=0.3, probability=0.99, optimize=True, z_keep_max=3.0, seed=1)
    keep, ground, planes = gr.ground_split(oracle.make_points(xyz), [(0.0, 10.0, 0.5), (10.0, 10.0, -1.0)], 0, gp)
    assert planes[1] is None and planes[0].found == 1 and planes[0].band_points == 3
    assert ground[[0, 1, 6]].all() and list(np.nonzero(keep)[0]) == [3, 4, 7]
    assert not keep[[2, 5, 8, 9]].any() and not ground[[2, 5, 8, 9]].any()


def test_radius_filter_is_strict_at_the_radius():
    line = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.5, 0.125, 0]], np.float32)
    assert list(gr.radius_keep(line, 0.25, 1)) == [False, False, True, True]          # 0.25 apart: d2 == r2, not inside
    assert list(gr.radius_keep(line, 0.25, 2)) == [False] * 4
    for xyz in (line, np.random.default_rng(1).uniform(0, 1, (300, 3)).astype(np.float32)):
        _, want = oracle.radius_outlier_removal(oracle.make_points(xyz), 0.25, 1)
        assert np.array_equal(gr.radius_keep(xyz, 0.25, 1), want)


# ---- what the frames are for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["border_nocrop", "border_crop"])
def test_border_frame_conditions(name):
    f = FRAMES[name]
    (cp0, keep0, ground0, planes0), (cp1, keep1, ground1, planes1) = split(name)
    # sensor 1 sees the same world points through its pose, bit for bit
    if name == "border_nocrop":
        assert bits(np.stack([cp0["x"], cp0["z"]], 1)) == bits(np.stack([cp1["x"], cp1["z"]], 1))      # (y: no limit on it)
        assert bits(np.stack([cp0["x"], cp0["y"], cp0["z"]], 1)) == bits(f.world + F(0.0))       # (the pose's +0.0 turns a -0.0 into +0.0)
    assert np.array_equal(keep0, keep1) and np.array_equal(ground0, ground1)
    probes = np.array([(x, 0.0, z) for x, z, _ in f.probes], np.float32)
    tags = [t for _, _, t in f.probes]
    slab, fate = gr.classify(probes, gf.BORDER_ZONES, gf.BORDER_Z_KEEP)
    for k, zone in enumerate(gf.BORDER_ZONES):
        mine = np.array([t.startswith(f"s{k}.") for t in tags])
        if k == 2:
            continue
        assert {KEPT} <= set(fate[mine]) and (zone[2] < 0 or {BAND, DROPPED} <= set(fate[mine])), k
    assert not (slab == 2).any() and (slab[np.array([t.startswith("s2.") for t in tags])] == 0).any()   # the inner slab: nothing
    on_shared = {t: s for t, s in zip(tags, slab) if t in ("s0.x1+0", "s1.x0+0", "s3.x0+0", "s6.x1+0", "s7.x0+0")}
    assert on_shared["s0.x1+0"] == on_shared["s1.x0+0"] == 0 and on_shared["s3.x0+0"] == on_shared["s6.x1+0"] == 3
    assert on_shared["s7.x0+0"] == 6                                                     # x == 4: slab 6 before slab 7
    for lim in ("x0", "x1", "-zmax", "zmax", "zlo", "zkeep"):                            # both sides of every kind of limit
        fates = {d: {f for t, f in zip(tags, fate) if f"{lim}{d}" in t} for d in ("-1", "+0", "+1")}
        assert len(fates["-1"] | fates["+1"]) >= 2, lim
    found = [pl for pl in planes0 if pl is not None]
    assert len(found) == 7 and sum(pl.found for pl in found) == 6 and planes0[2].band_points == 0       # every band fits a plane
    if name == "border_crop":                                                            # the box's faces are slab limits
        assert f.params.crop_min[0] == gf.BORDER_ZONES[5][0] and f.params.crop_max[2] == gf.BORDER_Z_KEEP
        assert len(cp0) < f.sensors[0].n


@pytest.mark.parametrize("name", ["small_bands_it32", "small_bands_it33"])
def test_small_bands_frame_conditions(name):
    pls = planes_of(name)
    sizes = {(s, k): pl.band_points for s, k, pl in pls}
    assert sizes == FRAMES[name].sizes
    assert set(gf.SMALL_SIZES) <= set(sizes.values())
    assert sum(n > 0 for n in sizes.values()) >= 20 and sum(0 < n < 3 for n in sizes.values()) >= 5
    assert sizes[(15, 7)] > 3 and dict(((s, k), pl) for s, k, pl in pls)[(15, 7)].found          # zone key 127
    keys = np.repeat([s * 8 + k for s, k in sizes], list(sizes.values()))                # the sorted band
    assert np.all(np.diff(keys) >= 0)
    runs = [keys[i:i + 1024] for i in range(0, len(keys), 1024)]
    distinct = [np.unique(r) for r in runs]
    assert max(len(d) for d in distinct) >= 4
    assert any(len(d) >= 3 and np.any(np.diff(d) > 1) for d in distinct)                 # an empty slab between occupied ones
    assert any(len(set(d // 8)) >= 2 for d in distinct)                                  # slabs of different sensors


def test_large_bands_frame_conditions():
    sizes = {pl.band_points for _, _, pl in planes_of("large_bands_it200")}
    assert set(gf.LARGE_SIZES) <= sizes
    refit = [pl for _, _, pl in planes_of("large_bands_it200") if pl.band_points in gf.LARGE_SIZES]
    assert all(pl.found and pl.n_inliers > 3 for pl in refit)


def test_skip_frame_conditions():
    pls = [pl for _, _, pl in planes_of("skip")]
    gp = FRAMES["skip"].gp
    spare = [pl for pl in pls if pl.end == "spare"]
    assert all(pl.iterations + pl.skipped == gp["max_iterations"] + gr.SPARE for pl in spare)
    assert sum(pl.found == 1 and pl.iterations < gp["max_iterations"] for pl in spare) >= 3
    assert sum(pl.found == 0 and pl.iterations == 0 for pl in spare) >= 1
    assert sum(pl.skipped > 0 for pl in pls) >= 3
    assert sum(pl.end == "max" for pl in pls) >= 1
    # valid and skipped samples alternate: some band's best hypothesis comes after a skipped one
    assert sum(pl.found and 0 < pl.best_hypothesis for pl in spare) >= 3


def test_threshold_frame_conditions():
    f = FRAMES["threshold"]
    (cp, keep, ground, planes), = split("threshold")
    xyz = np.stack([cp["x"], cp["y"], cp["z"]], 1)
    slab, fate = gr.classify(xyz, f.zones[0], f.gp["z_keep_max"])
    thr = F(f.gp["threshold"])
    assert bits(planes[0].plane[:2]) in ([0, 0], [0x80000000, 0x80000000], [0, 0x80000000], [0x80000000, 0]) \
        and abs(planes[0].plane[2]) == 1.0 and planes[0].plane[3] == 0.0                # the plane z = 0 exactly
    d0 = np.abs(gr.distance(planes[0].plane, xyz[(slab == 0) & (fate == BAND)]))
    at = (slab == 0) & (fate == BAND)
    at[at] = d0 == thr
    assert at.sum() >= 100 and not ground[at].any() and keep[at].all()
    assert {-0.25, 0.25} == set(xyz[at, 2].tolist())                                     # on both sides
    m1 = (slab == 1) & (fate == BAND)
    d1 = np.abs(gr.distance(planes[1].plane, xyz[m1]))
    near = np.array(bits(d1), np.int64) - bits(thr)
    assert (near == 0).any() or ((near == -1).any() and (near == 1).any()), collections.Counter(near[np.abs(near) < 4].tolist())
    assert (np.abs(near) <= 1).sum() >= 20 and (near < 0).any() and (near >= 0).any()
    assert np.array_equal(ground[m1], d1 < thr) and 0 < ground[m1].sum() < m1.sum()


def test_extreme_frame_conditions():
    for _, keep, ground, planes in split("no_band"):
        assert not ground.any() and keep.any() and not keep.all()
        assert all(pl is None or pl.band_points == 0 for pl in planes)
    for cp, keep, ground, planes in split("all_ground"):
        assert ground.all() and not keep.any() and len(cp) == FRAMES["all_ground"].n_points
    (cp0, keep0, ground0, planes0), (cp1, keep1, ground1, planes1) = split("no_zones_sensor")
    assert len(cp0) > 0 and planes0 == [] and not keep0.any() and not ground0.any() and ground1.any() and keep1.any()
    f = FRAMES["special_values"]
    with_, without = split("special_values"), split("special_values_removed")
    assert f.n_vanishing == 18 and f.n_points - FRAMES["special_values_removed"].n_points == 18
    for (cp_a, keep_a, ground_a, pl_a), (cp_b, keep_b, ground_b, pl_b) in zip(with_, without):
        assert cp_a.tobytes() == cp_b.tobytes() and np.array_equal(keep_a, keep_b) and np.array_equal(ground_a, ground_b)
        assert all(same_plane_result(a, b) for a, b in zip(pl_a, pl_b))
    cp = with_[0][0]
    assert (np.abs(cp["x"]) < 1e-37).sum() >= 4 and (cp["z"] == 0).any()   # denormal and zero coordinates stay
    assert np.isnan(cp["intensity"]).any() and np.isinf(cp["intensity"]).any()
    (cp, keep, ground, planes), = split("far")
    assert cp["x"].min() > 980 and cp["y"].max() < -990 and all(pl.found for pl in planes) and ground.any() and keep.any()


def test_filter_frame_conditions():
    f = FRAMES["filter"]
    (cp0, keep0, ground0, _), (cp1, keep1, ground1, _) = split("filter")
    no_filter = dict(f.gp, outlier_radius=0.0)

    def state(cp, keep, pts):
        xyz = np.stack([cp["x"], cp["y"], cp["z"]], 1)
        return [bool(keep[np.nonzero((xyz == p).all(1))[0][0]]) for p in pts]
    assert not any(state(cp0, keep0, f.lattice))                          # every neighbour at exactly the radius: lonely
    assert all(state(cp0, keep0, f.lattice2)) and all(state(cp0, keep0, f.centres))
    assert state(cp0, keep0, f.pair) == [False, False]                    # 10 cm apart, the slab border between them
    assert state(cp0, keep0, f.shared) == [False] and state(cp1, keep1, f.shared) == [False]      # one per sensor
    for s, (cp, keep, ground, _) in enumerate(split("filter")):           # without the filter every one of them stays
        k0, g0, _ = gr.ground_split(cp, f.zones[s], s, no_filter)
        assert np.array_equal(g0, ground) and k0.sum() > keep.sum()
        if s == 0:
            assert all(state(cp, k0, f.lattice)) and all(state(cp, k0, f.pair)) and all(state(cp, k0, f.shared))
    # with a closed test at the radius the lattice would stay: the pairs do sit at d2 == r2
    d = f.lattice[0] - f.lattice[1]
    assert F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) == F(np.float64(F(0.25)) ** 2)


def test_loop_coverage_across_the_frames():
    ends, rounds, its = collections.Counter(), collections.Counter(), set()
    for name, f in FRAMES.items():
        its.add(f.gp["max_iterations"])
        for _, _, pl in planes_of(name):
            if pl.band_points >= 3:
                ends[pl.end] += 1
                rounds[min((pl.iterations + pl.skipped - 1) // 32 + 1, 3)] += 1
                assert pl.end != "max" or pl.iterations == f.gp["max_iterations"] + 1
    assert {32, 33} <= its
    assert min(ends["max"], ends["probability"], ends["spare"]) >= 5, ends
    assert min(rounds[1], rounds[2], rounds[3]) >= 2, rounds
    it32 = [pl for _, _, pl in planes_of("small_bands_it32") if pl.end == "max"]
    it33 = [pl for _, _, pl in planes_of("small_bands_it33") if pl.end == "max"]
    assert len(it32) >= 5 and len(it33) >= 5                              # iterations 33 / 34: first and second hypothesis of round 2
