"""The quantile finish (k3_local<QUANT>, cm_kernels_v3.hip) at the edges of its straight-line rounds. The kernel runs its
per-record loops for a compile-time number of rounds (4, or all 8), a wave whose rounds are all full tests nothing per lane,
and a thread takes its block of sorted positions in one batch. The sizes at which that can go wrong are a wave's last full
round (multiples of 64 and of 256 and their neighbours), the step from four rounds to more (2048 | 2049 records at 512
threads, 4096 | 4097 at the large shape's 1024), a round more per thread (1536 | 1537, 3584 | 3585, 5120 | 5121) and a thread
block's end (2111 to 2113: 33 waves' worth), up to the capacity itself.

One designed frame holds a bucket of every such size (tests/quantile_frames.py places them on the splitters the model says the
device holds); a second one, armed as tests/test_quantile_edges.py::capacity_script arms its context, holds the large shape's.
The CPU test proves the frames have those populations from the oracle's keys; the GPU tests hold every frame against the
oracle (merged cloud, occupancy and centroids, tests/test_quantile.py::frame_against_oracle) and its flags against the
model's outcome, for both rankings and min_points_per_voxel 0 and 2."""
import functools

import pytest

from tests import quantile_model as qm
from tests.test_quantile_edges import VARIANTS, Script, designed, ordinary, run_script, set_variant

CAP, CAP_BIG = qm.CM4_CAP, qm.CM4_CAP_BIG

ROUND_POPS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1535, 1536, 1537, 2047, 2048, 2049, 2111, 2112, 2113,
              3583, 3584, 3585, 4031, 4032]
BIG_POPS = [4095, 4096, 4097, 5119, 5120, 5121, 8064]
MIN_PTS = [0, 2]


@functools.lru_cache(maxsize=None)
def rounds_script(min_pts):
    """Behind 25 ordinary buckets: buckets 0 to 23 hold ROUND_POPS, bucket 24 an ordinary 1800 (39 048 records)."""
    s = Script().add(ordinary(25, 1100 + min_pts, min_pts=min_pts), "fixed")
    f = designed(s, dict(enumerate(ROUND_POPS)), 1110 + min_pts, min_pts=min_pts)
    return s.add(f, "quantile", list(enumerate(ROUND_POPS)))


@functools.lru_cache(maxsize=None)
def big_rounds_script(min_pts):
    """Armed by a hand-back (one bucket of CM4_CAP + 1), then buckets 2, 5, 8, ... of BIG_POPS among thin ordinary ones: the
    large shape takes them (1024 threads: four rounds up to 4096 records, five up to 5120, eight at 8064)."""
    s = Script().add(ordinary(25, 1200 + min_pts, min_pts=min_pts), "fixed")
    s.add(designed(s, {12: CAP + 1}, 1210 + min_pts, ordinary_pop=1889, min_pts=min_pts), "handed_back", [(12, CAP + 1)])
    want = {2 + 3 * i: pop for i, pop in enumerate(BIG_POPS)}
    f = designed(s, want, 1220 + min_pts, ordinary_pop=900, min_pts=min_pts)
    return s.add(f, "big", sorted(want.items()))


SCRIPTS = {"rounds": (rounds_script, ROUND_POPS), "big_rounds": (big_rounds_script, BIG_POPS)}


@pytest.mark.parametrize("min_pts", MIN_PTS)
@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_designed_frames_have_the_populations_named(name, min_pts):
    make, pops = SCRIPTS[name]
    s = make(min_pts)
    assert s.ctx.hand_backs <= 2
    for k, st in enumerate(s.steps):
        where = f"{name}, min_pts {min_pts}, frame {k} ({st.frame.note})"
        assert st.what == st.expect, (where, None if st.pops is None else st.pops.tolist())
        assert st.n_kept == st.frame.n_kept, where
        assert st.frame.n_in < 2 * st.frame.n_kept, where
        if st.pops is not None:
            assert st.pops.sum() == st.n_kept, where
            for bucket, records in st.claims:
                assert st.pops[bucket] == records, (where, bucket, records, st.pops.tolist())
        else:
            assert not st.claims, where
    last = s.steps[-1]
    assert sorted(records for _, records in last.claims) == sorted(pops), "every size of the list is a bucket of the frame"
    if name == "rounds":
        assert last.n_kept == 39_048 and len(last.pops) == 25 and last.pops.max() == CAP
    else:
        assert int((last.pops > CAP).sum()) == len(BIG_POPS) <= qm.CM4_MAX_BIG and last.pops.max() == CAP_BIG


@pytest.mark.gpu
@pytest.mark.parametrize("min_pts", MIN_PTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_round_edges(variant, min_pts, monkeypatch):
    """Buckets of every size in ROUND_POPS in one frame, on the usual shape."""
    set_variant(variant, monkeypatch)
    seen = run_script(rounds_script(min_pts), variant)
    assert [what for what, _ in seen] == ["fixed", "quantile"]


@pytest.mark.gpu
@pytest.mark.parametrize("min_pts", MIN_PTS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_round_edges_of_the_large_shape(variant, min_pts, monkeypatch):
    """Buckets of every size in BIG_POPS in one armed frame: the large shape's rounds."""
    set_variant(variant, monkeypatch)
    seen = run_script(big_rounds_script(min_pts), variant)
    assert [what for what, _ in seen] == ["fixed", "handed_back", "big"]
