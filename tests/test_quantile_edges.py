"""The quantile route (cm_kernels_v4.hip, the k3_local<QUANT> finish) on DESIGNED frames: every data-dependent branch of the
route is placed exactly — ties at a splitter, duplicate splitters and the empty buckets between them, a bucket at exactly
the finish's capacity and one record beyond, the large finish shape and its list, frames of fewer records than buckets,
the packed 16-bit column counters, tile and sensor edges — instead of waiting for a random scene to hit it.

tests/quantile_model.py says, from the oracle's merged cloud of the previous frame, which splitters the device holds, how
many records of this frame fall into each bucket and what the route must therefore do; tests/quantile_frames.py builds
clouds with the populations a case names. The CPU tests prove that every designed frame really has those populations (from
the oracle's merged cloud, not from the generator's intent); the GPU tests run every frame through
tests/test_quantile.py::frame_against_oracle (merged cloud and occupancy bit-exact, centroids bit-exact up to 17 points) and
hold cm_result.path_flags against the model's outcome on EVERY frame. The device's splitters cannot be read through the
C-ABI, but a splitter that is off by one record moves a population across 4032 / 4033 or 8064 / 8065 and flips the flags."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest

from cloud_merger_amd import capi
from oracle import oracle
from tests import quantile_frames as qf
from tests import quantile_model as qm
from tests.test_quantile import PREDICTED, QUANTILE, REDONE, frame_against_oracle, needs_lds_rank

CAP, CAP_BIG, MAX_BIG, TARGET = qm.CM4_CAP, qm.CM4_CAP_BIG, qm.CM4_MAX_BIG, qm.CM4_TARGET


# ------------------------------------------------------------------------------------------------
# A case is a script: frames, and for each what the model says the route does with it.
# ------------------------------------------------------------------------------------------------
@dataclass
class Step:
    frame: qf.Frame
    what: str            # the model's outcome, from the oracle's merged clouds of this frame and the one before
    expect: str          # the outcome the case was designed for
    pops: object         # records per bucket (None: the route does not take the frame)
    claims: tuple        # (bucket, records) pairs the design names
    n_kept: int          # kept records, from the oracle
    longest: int         # longest voxel, from the oracle


def oracle_keys(frame):
    st, merged, out, rep = oracle.merge_voxelize(frame.sensors, frame.params, threads=4, stable=True)
    assert st == oracle.OK
    cells = oracle.voxel_cells(merged, frame.params.leaf)
    return cells, qm.keys_of_cells(cells)


class Script:
    def __init__(self):
        self.ctx = qm.Context()
        self.steps = []

    @property
    def spl(self):
        return self.ctx.spl

    def add(self, frame, expect, claims=()):
        cells, keys = oracle_keys(frame)
        what, pops = self.ctx.frame(keys, frame.n_in, frame.crop)
        # A frame that the fixed-grid passes take (at once, or as the redo of a hand-back) leaves splitters only if they need not
        # hand it back themselves.
        if what in ("fixed", "handed_back") and frame.crop and not qf.fixed_grid_fits(cells):
            self.ctx.known = False
        self.steps.append(Step(frame, what, expect, pops, tuple(claims), len(keys), int(np.unique(keys, return_counts=True)[1].max())))
        return self


def ordinary(n_buckets, seed, min_pts=0, longest=3):
    """n_buckets * CM4_TARGET records in small voxels spread over the whole box: exactly n_buckets buckets of CM4_TARGET."""
    rng = np.random.default_rng(seed)
    u, l = qf.spread(qf.small(n_buckets * TARGET, rng, longest))
    return qf.clouds(u, l, seed, min_pts=min_pts, note=f"ordinary, {n_buckets} buckets")


def designed(script, want, seed, ordinary_pop=1800, **kw):
    rng = np.random.default_rng(seed)
    u, l = qf.design(script.spl, want, rng, ordinary=ordinary_pop)
    return qf.clouds(u, l, seed, **kw)


def mixed_frame(crop=True):
    rng = np.random.default_rng(101)
    u, l = qf.spread(rng.integers(1, 41, size=1000))
    return qf.clouds(u, l, 101, crop=crop, note="1000 voxels of 1..40 points")


def case_replay():
    """1. A frame of mixed voxel sizes follows itself twice: every splitter is a key that occurs (a voxel on a quantile position
    goes whole into the upper bucket)."""
    a = mixed_frame()
    return Script().add(a, "fixed").add(a, "quantile").add(a, "quantile")


def _dup(u, l, pops):
    a = qf.clouds(u, l, 202)
    claims = list(enumerate(pops))
    return Script().add(a, "fixed").add(a, "quantile", claims).add(a, "quantile", claims)


def case_duplicate_mid():
    """2. 880 single-record voxels, one voxel of 3000 records, 880 single-record voxels: splitters [0, V, V], an empty bucket
    between two equal splitters, populations [880, 0, 3880]."""
    mid = qf.U_END // 2 + 5
    u = np.r_[qf.place(1, mid - 1, 880), mid, qf.place(mid + 1, qf.U_END, 880)]
    return _dup(u, np.r_[np.ones(880, int), 3000, np.ones(880, int)], [880, 0, 3880])


def case_duplicate_first_key():
    """2. The long voxel at index 0 of the box: splitters [0, 0, 0] — buckets 0 AND 1 are empty (two in a row), every record
    is in the last one."""
    u = np.r_[0, qf.place(1, qf.U_END, 1000)]
    return _dup(u, np.r_[3000, np.ones(1000, int)], [0, 0, 4000])


def case_duplicate_last_key():
    """2. The long voxel at the largest index of the box (its points lie ON the box's max corner)."""
    u = np.r_[qf.place(1, qf.U_END, 1000), qf.CORNER]
    return _dup(u, np.r_[np.ones(1000, int), 3000], [1000, 0, 3000])


def case_duplicate_two_in_a_row():
    """2. Two empty buckets in a row in the middle of a frame: a bucket that is ONE voxel of 4032 records covers three
    quantile positions of its frame (splitters [0, V, V, V]); the frame behind it runs on those."""
    s = Script().add(ordinary(3, 210), "fixed")
    x = designed(s, {0: 1000, 1: [CAP], 2: 760}, 211)
    s.add(x, "quantile", [(0, 1000), (1, CAP), (2, 760)])
    assert len(s.spl) == 4 and s.spl[1] == s.spl[2] == s.spl[3]
    y = designed(s, {0: 900, 1: 0, 2: 0, 3: [17] + qf.small(1500, np.random.default_rng(212))}, 212)
    return s.add(y, "quantile", [(0, 900), (1, 0), (2, 0), (3, 1517)])


FINISH_POPS = [1, 2, 511, 512, 513, 1024, 1025, 2016, 2017, 4031, 4032]


def case_finish_geometry():
    """3. Buckets of 1, 2, 511, 512, 513, 1024, 1025, 2016, 2017, 4031 and 4032 records in one frame: the finish's records per
    thread step from 1 to 8, and its second load half starts at 2017. Then the ordinary predecessor again: the buckets cut
    for the thin ones are too wide for it, and it is handed back."""
    p = ordinary(12, 300)
    s = Script().add(p, "fixed")
    f = designed(s, dict(enumerate(FINISH_POPS)), 301)
    s.add(f, "quantile", list(enumerate(FINISH_POPS)))
    return s.add(p, "handed_back")


def pinned(t, pop, rng, stays):
    """Bucket t with pop records, and its neighbours, such that a splitter that is off by one voxel in either direction (or a
    tie at a splitter that goes to the wrong side) flips the frame's outcome: a bucket at a capacity it must still fit
    (stays) has voxels of 1 record at its two ends and the neighbours voxels of 3 records beside them — either mistake
    gives it 2 records more; a bucket one record beyond a capacity has it the other way round and would lose 2."""
    own, other = (1, 3) if stays else (3, 1)
    return {t - 1: qf.small(1800 - other, rng) + [other], t: [own] + qf.small(pop - 2 * own, rng) + [own],
            t + 1: [other] + qf.small(1800 - other, rng)}


def capacity_script():
    """4. Unarmed: exactly CM4_CAP stays, CM4_CAP + 1 is handed back (and arms the large shape). Armed: CM4_CAP + 1 and exactly
    CM4_CAP_BIG run on the route, CM4_CAP_BIG + 1 is handed back."""
    rng = np.random.default_rng(410)
    s = Script().add(ordinary(10, 400), "fixed")
    s.add(designed(s, pinned(3, CAP, rng, True), 401), "quantile", [(3, CAP)])
    s.add(designed(s, pinned(5, CAP + 1, rng, False), 402), "handed_back", [(5, CAP + 1)])
    s.add(designed(s, {**pinned(2, CAP + 1, rng, False), **pinned(7, CAP_BIG, rng, True)}, 403), "big", [(2, CAP + 1), (7, CAP_BIG)])
    return s.add(designed(s, pinned(4, CAP_BIG + 1, rng, False), 404), "handed_back", [(4, CAP_BIG + 1)])


CAPACITY_BIG_STEP = 3            # the frame of capacity_script that needs the large shape


def _big_list(n_big):
    # 5. 70 buckets throughout: the hand-back that arms the large shape has as many records as its predecessor. The last frame
    # stays below twice its predecessor's points (a crop box that drops more than half makes a packed frame, which the route
    # does not take).
    s = Script().add(ordinary(70, 500), "fixed")
    s.add(designed(s, {35: CAP + 1}, 501, ordinary_pop=1889), "handed_back", [(35, CAP + 1)])
    assert len(s.spl) == 70
    want = {t: CAP + 1 for t in range(3, 3 + n_big)}
    f = designed(s, want, 502, ordinary_pop=900)
    return s.add(f, "big" if n_big <= MAX_BIG else "handed_back", [(t, CAP + 1) for t in want])


def case_big_list_full():
    """5. Armed, 70 buckets, CM4_MAX_BIG of them above CM4_CAP: the list is full, the frame stays on the route."""
    return _big_list(MAX_BIG)


def case_big_list_overflows():
    """5. ... and CM4_MAX_BIG + 1 of them: handed back."""
    return _big_list(MAX_BIG + 1)


def case_one_voxel_takes_all():
    """6. After a spread predecessor of 20 buckets, 70 000 records go into one voxel: one column of k4_colscan's packed 16-bit
    prefixes passes 65 535 and carries into its neighbour. Read in cm_kernels_v4.hip: k4_colscan adds the two halves of a word
    apart (32-bit) for the totals, so the total is right and raises quant_abort; k4_scatter returns on quant_abort before it
    loads its row of the prefixes (and k3_local<QUANT> and k3_compact leave on it too) — nothing reads the carried words.
    Handed back, and right (the fixed-grid redo cannot hold the voxel either and ends on the general path)."""
    s = Script().add(ordinary(20, 600), "fixed")
    f = designed(s, {7: [70_000]}, 601, ordinary_pop=300)
    return s.add(f, "handed_back", [(7, 70_000)])


def _few_records(n, high):
    """7. Far fewer records than buckets: behind a predecessor of 40 320 records (21 buckets) a frame of n records, all below
    S[1] or all at or above the last splitter; then the predecessor again."""
    # (a frame of 1, 5 or 64 records is a packed frame for its successor whatever that holds, so every size gets a context of
    # its own; the predecessor behind it is not taken by the route: more than twice the last frame's records)
    p = ordinary(21, 700)
    s = Script().add(p, "fixed").add(p, "quantile")
    t = len(s.spl) - 1 if high else 0
    lengths = {1: [1], 5: [2, 1, 2], 64: qf.small(64, np.random.default_rng(701))}[n]
    want = {b: 0 for b in range(len(s.spl))}
    want[t] = lengths
    f = designed(s, want, 702 + n, kept_per_sensor=[n - n // 2, n // 2])
    s.add(f, "quantile", [(b, n if b == t else 0) for b in range(len(s.spl))])
    return s.add(p, "fixed")


def case_long_voxels():
    """8. A bucket that is one voxel of 4032 points; a bucket of 100 voxels of 40 points (every voxel runs past its owner's block:
    many wave jobs); voxels of 16, 17, 18, 33, 64, 65 and 513 points that end exactly at their bucket's end."""
    s = Script().add(ordinary(12, 800), "fixed")
    rng = np.random.default_rng(801)
    want = {1: [CAP], 3: [40] * 100}
    for t, tail in zip(range(4, 11), (16, 17, 18, 33, 64, 65, 513)):
        want[t] = qf.small(1500, rng) + [tail]
    claims = [(t, sum(v)) for t, v in want.items()]
    return s.add(designed(s, want, 802), "quantile", claims)


def _min_pts(m):
    """9. min_points_per_voxel = m at bucket ends: the first and the last voxel of a bucket hold exactly m and m - 1 points (and
    the other way round in the next bucket), a bucket in the middle keeps no voxel at all, a bucket is one voxel of m - 1
    points, a bucket is one voxel of m points."""
    s = Script().add(ordinary(8, 900 + m, min_pts=m, longest=2 * m), "fixed")
    rng = np.random.default_rng(910 + m)
    want = {1: [m] + qf.small(1500, rng, 2 * m) + [m - 1],
            2: [m - 1] + qf.small(1500, rng, 2 * m) + [m],
            3: [m - 1] * (1800 // (m - 1)),          # keeps no voxel at all
            4: [m - 1],                              # a single voxel, dropped
            5: [m]}                                  # a single voxel, kept
    claims = [(t, sum(v)) for t, v in want.items()]
    return s.add(designed(s, want, 920 + m, min_pts=m), "quantile", claims)


def _tiles(n, three_sensors):
    """10. n kept records in one sensor, or over three sensors with an empty one in the middle, with NaN and out-of-box points
    sprinkled in (a tile's slots and its records differ); the frame follows itself, then once more without the sprinkled
    points (slots and records agree: n slots exactly)."""
    rng = np.random.default_rng(1000 + n)
    u, l = qf.spread(qf.small(n, rng))
    per = [n - n // 3, 0, n // 3] if three_sensors else [n]
    a = qf.clouds(u, l, 1000 + n, kept_per_sensor=per, junk=0.3, note="sprinkled")
    b = qf.clouds(u, l, 2000 + n, kept_per_sensor=per, note="clean")
    return Script().add(a, "fixed").add(a, "quantile").add(b, "quantile").add(a, "quantile")


CASES = {
    "replay": case_replay,
    "duplicate_mid": case_duplicate_mid,
    "duplicate_first_key": case_duplicate_first_key,
    "duplicate_last_key": case_duplicate_last_key,
    "duplicate_two_in_a_row": case_duplicate_two_in_a_row,
    "finish_geometry": case_finish_geometry,
    "capacity": capacity_script,
    "big_list_full": case_big_list_full,
    "big_list_overflows": case_big_list_overflows,
    "one_voxel_takes_all": case_one_voxel_takes_all,
    "long_voxels": case_long_voxels,
}
for _n in (1, 5, 64):
    CASES[f"few_records_{_n}_low"] = functools.partial(_few_records, _n, False)
    CASES[f"few_records_{_n}_high"] = functools.partial(_few_records, _n, True)
for _m in (2, 3, 6):
    CASES[f"min_pts_{_m}"] = functools.partial(_min_pts, _m)
for _n in (4095, 4096, 4097, 8192, 8193):
    CASES[f"tiles_{_n}_one_sensor"] = functools.partial(_tiles, _n, False)
    CASES[f"tiles_{_n}_three_sensors"] = functools.partial(_tiles, _n, True)


@functools.lru_cache(maxsize=None)
def script_of(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------
# CPU: the model, and that every designed frame has the populations its case names
# ------------------------------------------------------------------------------------------------
def test_constants_mirror_the_header():
    assert (qm.CM4_TARGET, qm.CM4_BINS, qm.CM4_CAP, qm.CM4_CAP_BIG, qm.CM4_MAX_BIG) == (1920, 2048, 4032, 8064, 64)
    assert (qm.CM4_MAX_AVG, qm.CM4_MAX_BUCKETS, qm.CM_TILE) == (2600, 8192, 4096)
    assert [qm.buckets(n) for n in (0, 1, 100, 1920, 1921, 3840, 3841)] == [0, 1, 1, 1, 2, 2, 3]
    assert qm.buckets(2048 * 1920 + 1) == 2048 and qm.buckets(2048 * 2600) == 2048       # one pass while 2048 buckets of <= 2600 hold it
    assert qm.buckets(2048 * 2600 + 1) == (2048 * 2600 + 1 + 1919) // 1920 and qm.buckets(20_000_000) == 8192


def random_keys(rng, n_voxels, longest):
    keys = np.unique(rng.integers(1, 1 << 28, size=n_voxels, dtype=np.int64))
    n_voxels = len(keys)
    return np.repeat(keys, rng.integers(1, longest + 1, size=n_voxels))


@pytest.mark.parametrize("n_voxels,longest", [(1, 1), (1, 5000), (7, 3), (1000, 40), (3000, 1), (20_000, 17), (500, 900)])
def test_model_properties(n_voxels, longest):
    rng = np.random.default_rng(n_voxels * 7919 + longest)
    keys = random_keys(rng, n_voxels, longest)
    n = len(keys)
    spl, q = qm.splitters(keys)
    assert len(spl) == qm.buckets(n) and q == -(-n // len(spl)) and spl[0] == 0
    assert (np.diff(spl) >= 0).all(), "splitters ascend (no bucket: above every key)"
    assert all(s == qm.NO_BUCKET or s in keys for s in spl[1:]), "every splitter is a key that occurs"
    pops = qm.populations(spl, keys)
    assert pops.sum() == n
    run = int(np.unique(keys, return_counts=True)[1].max())
    assert pops.max() <= q + run, "replayed on its own splitters a bucket holds at most Q records and one voxel's rest"
    # a voxel is never split, and a key ON a splitter belongs to the upper bucket
    b = qm.bucket_of(spl, keys)
    assert all(len(set(b[keys == k])) == 1 for k in np.unique(keys)[:50])
    for j in range(1, len(spl)):
        if spl[j] != qm.NO_BUCKET:
            assert qm.bucket_of(spl, [spl[j]])[0] >= j > qm.bucket_of(spl, [spl[j] - 1])[0]
    # another frame on these splitters: every record lands somewhere
    other = random_keys(rng, max(1, n_voxels // 3), longest)
    assert qm.populations(spl, other).sum() == len(other)


def test_hand_checked_duplicate_splitters():
    v = 5000
    keys = np.r_[np.arange(1, 881), np.full(3000, v), np.arange(v + 1, v + 881)]
    spl, q = qm.splitters(keys)
    assert qm.buckets(len(keys)) == 3 and q == 1587
    assert list(spl) == [0, v, v]
    assert list(qm.populations(spl, keys)) == [880, 0, 3880]
    assert qm.outcome(qm.populations(spl, keys), armed=False) == "quantile"


def test_hand_checked_replay():
    rng = np.random.default_rng(5)
    keys = np.repeat(np.arange(1, 1001) * 977, rng.integers(1, 41, size=1000))
    spl, q = qm.splitters(keys)
    pops = qm.populations(spl, keys)
    assert len(spl) == qm.buckets(len(keys)) == -(-len(keys) // 1920)
    assert pops.sum() == len(keys) and q - 40 < pops[:-1].min() and pops.max() < q + 40, (q, pops)


def test_outcome_and_arming():
    assert qm.outcome([CAP, 0, 1], False) == "quantile" and qm.outcome([CAP + 1], False) == "handed_back"
    assert qm.outcome([CAP + 1, CAP_BIG], True) == "big" and qm.outcome([CAP_BIG + 1], True) == "handed_back"
    assert qm.outcome([CAP + 1] * MAX_BIG + [5], True) == "big" and qm.outcome([CAP + 1] * (MAX_BIG + 1), True) == "handed_back"
    ctx = qm.Context()
    one = np.arange(1, 3841, dtype=np.int64) * 1000                     # 3840 records: two buckets
    many = np.repeat(one, 3)[: CAP + 1]                               # 4033 records into the first of them
    assert ctx.frame(one, 3840)[0] == "fixed"
    assert ctx.frame(one, 3840)[0] == "quantile"
    assert ctx.frame(many, len(many))[0] == "handed_back" and ctx.arm == qm.ARMED_FRAMES
    assert ctx.frame(many[:CAP], CAP)[0] == "quantile"                # (4033 records left 3 buckets)
    spent = 1
    while ctx.arm:                                                    # armed for 16 quantile frames, then no more
        assert ctx.frame(one, 3840)[0] == "quantile"
        spent += 1
    assert spent == qm.ARMED_FRAMES
    assert ctx.frame(many, len(many))[0] == "handed_back"
    assert ctx.frame(one, 3840)[0] == "quantile" and ctx.frame(many, len(many))[0] == "big" and ctx.arm == qm.ARMED_FRAMES
    # a crop-packed frame (more than twice the last frame's records come in) is not taken
    assert ctx.frame(np.arange(1, 40, dtype=np.int64), 10 * len(many))[0] == "fixed"


@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_frames_have_the_populations_the_case_names(name):
    s = script_of(name)
    assert s.ctx.hand_backs <= 2, "three hand-backs in eight attempts rest the route: the case would test nothing"
    for k, st in enumerate(s.steps):
        where = f"{name}, frame {k} ({st.frame.note})"
        assert st.what == st.expect, (where, None if st.pops is None else st.pops.tolist())
        assert st.n_kept == st.frame.n_kept, where
        assert st.frame.n_in < 2 * st.frame.n_kept, f"{where}: more junk than records"
        if st.pops is not None:
            assert st.pops.sum() == st.n_kept, where
            for bucket, records in st.claims:
                assert st.pops[bucket] == records, (where, bucket, records, st.pops.tolist())
        else:
            assert not st.claims, where
        if k and s.steps[k - 1].frame is st.frame and st.pops is not None:     # a frame behind itself
            q = -(-st.n_kept // len(st.pops))
            assert st.pops.max() <= q + st.longest, where


def test_case_designs_reach_what_they_are_for():
    """Beyond the named populations: the structure each case exists for, read off the model."""
    s = script_of("duplicate_mid")
    assert s.spl[1] == s.spl[2] != qm.NO_BUCKET
    s = script_of("duplicate_first_key")
    assert s.spl[1] == s.spl[2] == qm.keys_of_cells(qf.cells_of_u([0]))[0], "the splitters are the box's first index"
    s = script_of("duplicate_last_key")
    assert s.spl[1] == s.spl[2] == qm.keys_of_cells([(512, 512, 128)])[0], "the splitters are the box's last index"
    assert qf.box_keys(np.array([[512, 512, 128]]))[0] == 1025 * 1025 * 257 - 1 < 1 << qf.KEY_BITS
    s = script_of("capacity")
    assert [st.what for st in s.steps] == ["fixed", "quantile", "handed_back", "big", "handed_back"]
    assert s.steps[CAPACITY_BIG_STEP].what == "big"
    for name, n_big in (("big_list_full", MAX_BIG), ("big_list_overflows", MAX_BIG + 1)):
        st = script_of(name).steps[-1]
        assert len(st.pops) == 70 and int((st.pops > CAP).sum()) == n_big and st.pops.max() <= CAP_BIG
        prev = script_of(name).steps[-2]
        assert st.frame.n_in <= 2 * prev.n_kept and min(st.frame.n_in, prev.n_kept + prev.n_kept // 4) <= 2 * prev.n_kept + qm.CM_TILE
    st = script_of("one_voxel_takes_all").steps[-1]
    assert st.pops.max() == 70_000 > 0xFFFF and len(st.pops) == 20
    for n in (1, 5, 64):
        for side in ("low", "high"):
            st = script_of(f"few_records_{n}_{side}").steps[2]
            assert len(st.pops) == 21 and st.n_kept == n
    st = script_of("long_voxels").steps[-1]
    assert st.longest == CAP
    # every frame that the fixed-grid passes take in the middle of a script leaves splitters (the model keeps track)
    for name in CASES:
        s = script_of(name)
        assert s.ctx.known or s.steps[-1].what in ("fixed", "handed_back"), name


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
VARIANTS = ["lds_rank", "ballot"]                 # default; CM_LDS_RANK=0 (ranks by ballots in every kernel)


def set_variant(variant, monkeypatch):
    if variant == "ballot":
        monkeypatch.setenv("CM_LDS_RANK", "0")


def assert_outcome(res, what, where):
    f = res.path_flags
    if what in ("quantile", "big"):
        assert f & QUANTILE and not f & REDONE and res.sort_passes == 1, (where, what, hex(f), res.sort_passes)
    elif what == "handed_back":
        assert f & REDONE and not f & QUANTILE, (where, what, hex(f))
    else:
        assert not f & QUANTILE, (where, what, hex(f))


def run_script(script, variant, flags=capi.FLAG_OCCUPANCY, after_frame=None):
    cap = max(max(st.frame.n_in for st in script.steps), 1 << 17)
    n_sensors = max(len(st.frame.sensors) for st in script.steps)
    assert all(len(st.frame.sensors) == n_sensors for st in script.steps)
    seen = []
    with capi.CloudMerger(max_points_total=cap, max_sensors=n_sensors, flags=flags) as cm:
        for k, st in enumerate(script.steps):
            res, rep = frame_against_oracle(cm, st.frame.sensors, st.frame.params, cap)
            if variant == "lds_rank":
                needs_lds_rank(res)
            else:
                assert not res.path_flags & 1
            if k == 0 and st.frame.crop:
                assert 23 <= res.key_bits <= 30 and tuple(res.div_b) == qf.BOX_DIV, (res.key_bits, tuple(res.div_b))
            assert res.n_merged == st.n_kept
            assert_outcome(res, st.what, (k, st.frame.note))
            seen.append((st.what, hex(res.path_flags)))
            if after_frame:
                after_frame(k, cm, res)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_designed_case(name, variant, monkeypatch):
    """Cases 1 to 10 of the module's table (CASES): every frame against the oracle, every frame's flags against the model."""
    set_variant(variant, monkeypatch)
    run_script(script_of(name), variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_large_shape_shows_as_a_stage(variant, monkeypatch):
    """4. A context with CM_FLAG_PROFILE: the armed frames (behind the hand-back) have a k3_local(big) stage, the unarmed ones
    have none."""
    set_variant(variant, monkeypatch)
    s = script_of("capacity")
    stages = {}

    def note(k, cm, res):
        stages[k] = [n for n, _ in cm.stage_times()]
    run_script(s, variant, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE, after_frame=note)
    assert "k3_local(big)" not in stages[1] and "k3_local" in stages[1], stages[1]
    assert "k3_local(big)" in stages[CAPACITY_BIG_STEP], stages[CAPACITY_BIG_STEP]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_large_shape_is_deterministic(variant, monkeypatch):
    """12. The frame of case 4 that needs the large shape, on two contexts with the same history: identical result, cells and
    counts, byte for byte."""
    set_variant(variant, monkeypatch)
    s = script_of("capacity")
    got = []
    for _ in range(2):
        grabbed = {}

        def grab(k, cm, res):
            if k == CAPACITY_BIG_STEP:
                cells, counts = cm.cells(res.n_out)
                grabbed["bytes"] = (cm.result(res.n_out).tobytes(), cells.tobytes(), counts.tobytes())
        run_script(s, variant, after_frame=grab)
        got.append(grabbed["bytes"])
    assert got[0] == got[1]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_replay_without_a_crop_box(variant, monkeypatch):
    """11. Case 1 without a crop box: the frame runs in the box predicted from its predecessor's bounds. The voxels are spread
    over the whole +-32, +-32, +-8 m, so the predicted box has a 29-bit index as well and the fixed-grid route needs two global
    passes (the quantile route replaces two or more). A frame carries CM_PATH_PREDICTED and CM_PATH_QUANTILE together as soon
    as a frame in the same predicted box has left splitters; the model's populations hold from there on (keys are
    order-only, the box does not matter to them)."""
    set_variant(variant, monkeypatch)
    a = mixed_frame(crop=False)
    _, keys = oracle_keys(a)
    spl, q = qm.splitters(keys)
    assert qm.outcome(qm.populations(spl, keys), armed=False) == "quantile"
    flags = []
    with capi.CloudMerger(max_points_total=1 << 17, max_sensors=len(a.sensors), flags=capi.FLAG_OCCUPANCY) as cm:
        for k in range(6):
            res, rep = frame_against_oracle(cm, a.sensors, a.params, 1 << 17)
            if variant == "lds_rank":
                needs_lds_rank(res)
            flags.append(res.path_flags)
            assert not res.path_flags & REDONE, [hex(f) for f in flags]
            if flags[-1] & QUANTILE:
                assert flags[-1] & PREDICTED and res.sort_passes == 1 and 23 <= res.key_bits <= 30, (hex(flags[-1]), res.key_bits)
            if len(flags) >= 2 and flags[-1] & QUANTILE and flags[-2] & QUANTILE:
                break
    assert any(f & QUANTILE and f & PREDICTED for f in flags), [hex(f) for f in flags]
    first = next(k for k, f in enumerate(flags) if f & QUANTILE)
    assert all(f & QUANTILE for f in flags[first:]), [hex(f) for f in flags]
