"""Numpy model of what the quantile route (cm_kernels_v4.hip, the k3_local<QUANT> finish of cm_kernels_v3.hip) predicts and
decides, in plain integer arithmetic — written from the comments of cm_device.h, cm_kernels_v3.hip ("the next frame's
splitters") and cm_route.cpp, not by calling the library. tests/test_quantile_edges.py holds the device's path_flags against it.

A frame whose kept records (after transform and crop) have the ascending keys k[0..n) leaves, for the NEXT frame,
bn = buckets(n) buckets of Q = ceil(n / bn) records: splitter S[0] = 0 (below every key), S[j] = k[j * Q] while j * Q < n,
"no bucket" from there on. The bucket of a key is the number of S[1..] that are <= the key: a voxel is never split, a voxel
that sits on a quantile position goes whole into the upper bucket, two equal splitters leave the bucket between them empty.

Keys: the device's is the linear index of a point's cell in the box the frame is sorted in, x fastest and z slowest. Only
order and equality matter here, so the model's key of a cell is (z, y, x) packed into one integer — the same order in any box."""
import os
import re

import numpy as np

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cloud_merger_amd", "csrc", "cm_device.h")


def _header_constants(names):
    with open(_HEADER) as f:
        text = f.read()
    out = {}
    for name in names:
        m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, text, re.M)
        assert m, f"{name} not found in cm_device.h"
        out[name] = int(m.group(1))
    return out


_C = _header_constants(["CM4_TARGET", "CM4_BINS", "CM4_CAP", "CM4_CAP_BIG", "CM4_MAX_BIG", "CM4_MAX_AVG", "CM4_MAX_BUCKETS",
                        "CM_TILE"])
CM4_TARGET, CM4_BINS, CM4_CAP, CM4_CAP_BIG = _C["CM4_TARGET"], _C["CM4_BINS"], _C["CM4_CAP"], _C["CM4_CAP_BIG"]
CM4_MAX_BIG, CM4_MAX_AVG, CM4_MAX_BUCKETS, CM_TILE = _C["CM4_MAX_BIG"], _C["CM4_MAX_AVG"], _C["CM4_MAX_BUCKETS"], _C["CM_TILE"]

ARMED_FRAMES = 16                 # cm_route.cpp: the large finish shape stays armed for 16 quantile frames
NO_BUCKET = np.int64(2**63 - 1)   # a splitter beyond the frame's buckets (the device's 0xFFFFFFFF): above every key
_OFF, _BITS = 1 << 20, 21         # a cell coordinate lies within +-2^20 (the route wants fewer than 2^24 cells per axis)


def buckets(n):
    """cm_quant_buckets: buckets the NEXT frame uses when this one sorted n records."""
    if n == 0:
        return 0
    b = (n + CM4_TARGET - 1) // CM4_TARGET
    if b > CM4_BINS and (n + CM4_BINS - 1) // CM4_BINS <= CM4_MAX_AVG:
        b = CM4_BINS
    return min(b, CM4_MAX_BUCKETS)


def keys_of_cells(cells):
    """(n, 3) absolute cells -> int64 keys in z-major order (the order of the device's linear index in any box)."""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    assert (np.abs(c) < _OFF).all()
    return ((c[:, 2] + _OFF) << (2 * _BITS)) | ((c[:, 1] + _OFF) << _BITS) | (c[:, 0] + _OFF)


def cells_of_keys(keys):
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    m = (1 << _BITS) - 1
    return np.stack([(k & m) - _OFF, ((k >> _BITS) & m) - _OFF, (k >> (2 * _BITS)) - _OFF], axis=1)


def splitters(keys):
    """The splitters a frame with these kept records leaves: (S, Q). len(S) == buckets(n)."""
    k = np.sort(np.asarray(keys, dtype=np.int64))
    n = len(k)
    bn = buckets(n)
    if bn == 0:
        return np.zeros(0, dtype=np.int64), 1
    q = (n + bn - 1) // bn
    s = np.full(bn, NO_BUCKET, dtype=np.int64)
    j = np.arange(bn, dtype=np.int64)
    has = j * q < n
    s[has] = k[j[has] * q]
    s[0] = 0                                    # below every key (a packed key is positive): bucket 0 has no lower end
    return s, q


def bucket_of(spl, keys):
    """Bucket of every key = how many of S[1..] are <= the key."""
    return np.searchsorted(spl[1:], np.asarray(keys, dtype=np.int64), side="right")


def populations(spl, keys):
    """Records per bucket of a frame with these kept records, under the splitters spl."""
    return np.bincount(bucket_of(spl, keys), minlength=len(spl)).astype(np.int64)


def outcome(pops, armed):
    pops = np.asarray(pops)
    if (pops <= CM4_CAP).all():
        return "quantile"
    if armed and (pops <= CM4_CAP_BIG).all() and int((pops > CM4_CAP).sum()) <= CM4_MAX_BIG:
        return "big"
    return "handed_back"


class Context:
    """Follows one context of the library through a stream of frames on ONE grid (the caller keeps the grid fixed).

    frame(keys, n_in, crop) returns the model's outcome and the populations:
      "fixed"        the route does not take the frame (no splitters yet, a crop-packed frame, the size rules of
                     RouteState::plan): fixed-grid passes, no CM_PATH_QUANTILE
      "quantile"     every bucket within CM4_CAP
      "big"          armed, every bucket within CM4_CAP_BIG, at most CM4_MAX_BIG of them above CM4_CAP
      "handed_back"  a bucket too large: redone with the fixed-grid passes (CM_PATH_REDONE)
    Splitters are replaced after every frame that finishes (a redone one too: the fixed-grid redo leaves them). `armed` is
    true for the 16 quantile frames behind a hand-back and is renewed by a frame that used the large shape.
    Not modelled (the cases keep clear of them): the rest after three hand-backs in eight attempts, frames of empty clouds,
    shared bins (more than CM4_BINS buckets), and what a frame leaves that the fixed-grid passes had to hand back themselves
    — `known` turns False where the model can no longer say what the context holds."""

    def __init__(self):
        self.spl = None
        self.spl_n = 0
        self.last_n = 0
        self.arm = 0
        self.hand_backs = 0
        self.known = True

    def admitted(self, n_in, crop):
        if self.spl is None or self.spl_n == 0:
            return False
        if crop and self.last_n and 2 * self.last_n < n_in:          # crop-packed (RouteState::pack_survivors)
            return False
        nb = buckets(self.spl_n)
        est = min(n_in, self.last_n + self.last_n // 4) if self.last_n else n_in
        return nb != 0 and nb <= CM4_BINS and self.spl_n // nb <= CM4_MAX_AVG and est <= 2 * self.spl_n + CM_TILE

    def frame(self, keys, n_in, crop=True):
        assert self.known, "the model lost track of this context"
        keys = np.sort(np.asarray(keys, dtype=np.int64))
        assert len(keys), "frames without a kept record are not modelled"
        if not self.admitted(n_in, crop):
            pops, what = None, "fixed"
        else:
            pops = populations(self.spl, keys)
            armed = self.arm > 0
            if self.arm:
                self.arm -= 1
            what = outcome(pops, armed)
            if what == "handed_back":
                self.arm = ARMED_FRAMES
                self.hand_backs += 1
            elif what == "big":
                self.arm = ARMED_FRAMES
        # Behind a crop box the fixed-grid passes (a frame the route does not take, or the redo of a hand-back) size their later
        # launches for half as many records again as the last frame kept, plus two tiles (RouteState::size_fixed_grid). A frame
        # that keeps more is handed on to the general path, which leaves no splitters: right, but not followed from here.
        if what in ("fixed", "handed_back") and crop and self.last_n and len(keys) > self.last_n + self.last_n // 2 + 2 * CM_TILE:
            self.known = False
        self.spl, _ = splitters(keys)
        self.spl_n = self.last_n = len(keys)
        return what, pops
