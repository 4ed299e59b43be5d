"""The bucket finishes divide a voxel's sums by its count as q = RN(x * RN(1/c)) plus one FMA correction
(centroid_div_rc, cm_common.hpp), not with a division. This states on the host, from exact
rationals, where that sequence is pcl's correctly rounded fp32 quotient and where it is not: it misrounds exact ties in
the subnormal range (c = 6: 9 ulps / 6 = 1.5 ulps gives 1 ulp, not 2), which is why the kernels fall back to a
correctly rounded division (of the sum plus +0.0f, like centroid_div) for quotients that are not normal numbers."""
from fractions import Fraction

import numpy as np
import pytest

from tests.edge_frames import (F, FLT_MIN, bits_of, device_div_exact, device_div_vec, f32_bits, quot32, rn32, ulps)

SUMS = np.arange(0, 1 << 12, dtype=np.uint32)          # +0 and every subnormal sum of up to 2^12 - 1 ulps


def rn_ulps(s, c):
    return np.array([round(Fraction(int(k), c)) for k in s], dtype=np.uint32)


def test_rn32_rounds_ties_to_even_and_keeps_subnormals():
    assert bits_of(rn32(Fraction(3, 2) * Fraction(2) ** -149)) == 2
    assert bits_of(rn32(Fraction(5, 2) * Fraction(2) ** -149)) == 2
    assert bits_of(rn32(Fraction(1, 2) * Fraction(2) ** -149)) == 0
    assert bits_of(rn32(-Fraction(2) ** -149)) == 0x80000001
    assert rn32(Fraction(1, 3)) == F(1) / F(3)
    assert np.isinf(rn32(Fraction(2) ** 128)) and rn32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) == np.finfo(F).max
    assert np.isinf(rn32(Fraction(2) ** 128 - Fraction(2) ** 103))                  # the tie above the largest: even = inf
    rng = np.random.default_rng(3)
    for x, c in zip(rng.uniform(-1e6, 1e6, 200).astype(F), rng.integers(1, 5000, 200)):
        assert bits_of(quot32(x, c)) == bits_of(F(x) / F(c))           # numpy's fp32 division is correctly rounded


def test_vectorised_emulation_matches_the_exact_one():
    rng = np.random.default_rng(4)
    for c in (1, 2, 3, 6, 7, 18, 64):
        for s in rng.choice(SUMS, 40, replace=False):
            x = f32_bits(int(s))
            for fb in (False, True):
                assert bits_of(device_div_vec(np.array([x]), c, fb)[0]) == bits_of(device_div_exact(x, c, fb)), (s, c, fb)


@pytest.mark.parametrize("c", range(1, 65))
def test_device_division_of_subnormal_sums(c):
    x = SUMS.view(np.float32)
    want = rn_ulps(SUMS, c)
    for sgn in (1, -1):
        xs = x * F(sgn)
        w = want.view(np.float32) * F(sgn)
        w[SUMS == 0] = F(0.0)                            # a -0.0 sum gives +0.0, pcl's accumulator starts at +0.0f
        got = device_div_vec(xs, c, fallback=True)
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), f"count {c}: the fallback must give RN32(x / c)"
        raw = device_div_vec(xs, c, fallback=False)
        bad = SUMS[raw.view(np.uint32) != w.view(np.uint32)]
        # without the fallback: ties rounded to the odd neighbour for some counts
        if c in (1, 2, 3, 4, 5, 17, 64):
            assert bad.tolist() == [], (c, bad[:5])
        if c == 6:
            assert {9, 0xAB9} <= set(bad.tolist()) and int((bad[bad < 3000] > 0).sum()) == 250
        if c == 18:
            assert 0x1B in bad.tolist() and int((bad[bad < 3000] > 0).sum()) == 83


def test_device_division_near_the_smallest_normal():
    """Quotients from just below to just above 2^-126 (where the fallback starts and ends), and ordinary normal sums:
    the sequence with the fallback is RN32(x / c) in every case."""
    rng = np.random.default_rng(6)
    for c in list(range(1, 20)) + [64, 1000, 65535]:
        lo = F(FLT_MIN * c)
        for x in [ulps(lo, k) for k in range(-3, 4)] + list(rng.uniform(0.5, 1.5, 8).astype(F) * lo):
            for s in (F(x), -F(x)):
                assert bits_of(device_div_exact(s, c)) == bits_of(quot32(s, c)), (bits_of(s), c)
        for x in rng.uniform(-3000, 3000, 10).astype(F):
            assert bits_of(device_div_exact(x, c)) == bits_of(quot32(x, c)), (x, c)
