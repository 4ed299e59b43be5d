"""CPU-side checks of bench.py's --dump-outputs writer (a stand-in context, no GPU): the last step's centroids as float32
.npy files, a fixed sample above the size cap, and the command line that asks for them."""
import os
import sys

import numpy as np
import pytest

import bench
from cloud_merger_amd.types import XYZI_DTYPE


class FakeContext:
    """What dump_outputs uses of capi.CloudMerger: result(n_out) -> (n_out,) XYZI records."""

    def __init__(self, n):
        rng = np.random.Generator(np.random.PCG64(7))
        self.out = np.zeros(n, dtype=XYZI_DTYPE)
        for name in ("x", "y", "z", "intensity"):
            self.out[name] = rng.standard_normal(n).astype(np.float32)

    def result(self, n_out):
        assert n_out == len(self.out)
        return self.out.copy()


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_voxel_below_the_cap(tmp_path):
    cm = FakeContext(1000)
    bench.dump_outputs(str(tmp_path / "d"), cm, 1000)
    got = load(tmp_path / "d")
    assert sorted(got) == ["intensity", "n_out", "x", "y", "z"]
    assert got["n_out"].dtype == np.float64 and got["n_out"].tolist() == [1000.0]
    for name in ("x", "y", "z", "intensity"):
        assert got[name].dtype == np.float32
        assert np.array_equal(got[name].view(np.uint32), cm.out[name].view(np.uint32))


def test_dump_samples_a_large_result_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VOXELS", 64)
    cm = FakeContext(5000)
    bench.dump_outputs(str(tmp_path / "a"), cm, 5000)
    bench.dump_outputs(str(tmp_path / "b"), cm, 5000)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert sorted(a) == ["index", "intensity", "n_out", "x", "y", "z"]
    idx = a["index"].astype(np.int64)
    assert a["index"].dtype == np.float64 and len(idx) == 64
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 5000
    assert a["n_out"].tolist() == [5000.0]
    for name in a:
        assert np.array_equal(a[name], b[name])
    for name in ("x", "y", "z", "intensity"):
        assert np.array_equal(a[name], cm.out[name][idx])


def test_dump_stays_under_64_mb():
    assert bench.DUMP_MAX_VOXELS * (4 * 4 + 8) + 1024 <= 64 * 1000 * 1000


def test_command_line(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 0 and args.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
