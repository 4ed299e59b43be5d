#!/usr/bin/env python3
"""Writes tests/golden/known_answers.json: the hand-derived known-answer cases of SURVEY.md
Appendix B.  The reference holds no fixtures for this path (parity unpinned), so every expectation
below is derived here from the algorithm statement with explicit scalar
float32 arithmetic — this script imports neither oracle nor the product.

Floats are stored as uint32 bit patterns so the fixture is exact.
Run:  python tests/golden/make_known_answers.py
"""
import json
import os
from fractions import Fraction

import numpy as np

F = np.float32


def bits(v):
    return int(np.asarray(v, dtype=F).view(np.uint32))


def pts(rows):
    """rows of (x,y,z,i) -> list of 4 bit patterns"""
    return [[bits(c) for c in r] for r in rows]


def rn32(fr):
    """an exact rational rounded to the nearest fp32: ties to even, subnormals kept, +-inf beyond the largest value"""
    if fr == 0:
        return F(0.0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    e += 1 if Fraction(2) ** (e + 1) <= a else (-1 if Fraction(2) ** e > a else 0)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    v = round(a / quantum) * quantum                  # Fraction.__round__ rounds ties to even
    out = np.inf if v >= Fraction(2) ** 128 else float(v)
    return F(out if fr > 0 else -out)


def mean_exact(vals):
    """fp32 running sum from +0.0f in the given order, then RN32(sum / count) from exact rationals"""
    acc = F(0)
    with np.errstate(over="ignore"):
        for v in vals:
            acc = F(acc + F(v))
    if not np.isfinite(acc) or acc == 0:
        return F(acc / F(len(vals)))
    return rn32(Fraction(float(acc)) / len(vals))


def sub(k):
    """k subnormal ulps (k < 0: negative)"""
    v = np.array([abs(k)], dtype=np.uint32).view(F)[0]
    return F(-v) if k < 0 else v


def mean_seq(vals):
    """fp32 running sum in the given order, then one fp32 division by the count."""
    acc = F(0)
    for v in vals:
        acc = F(acc + F(v))
    return F(acc / F(len(vals)))


IDENT = dict(q=[0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0])
cases = []

# 1. Identity, one voxel.
a, b = (0.01, 0.01, 0.01, 10.0), (0.09, 0.09, 0.09, 30.0)
c = [mean_seq([a[k], b[k]]) for k in range(4)]
cases.append(dict(name="identity_one_voxel", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts([a, b]), **IDENT)],
                  expect=dict(status="OK", out=pts([c]), cells=[[0, 0, 0]], counts=[2])))

# 2. Face inclusion: fl32(x * fl32(1/0.1f)).
inv = F(1) / F(0.1)
assert inv == F(10.0)
xs = [F(0.1), F(0.3)]
cells2 = [int(np.floor(F(x * inv))) for x in xs]
assert cells2 == [1, 3], cells2          # 0.3f*10 is an exact tie, rounds to even = 3.0f
cases.append(dict(name="face_inclusion", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts([(x, 0.05, 0.05, 1.0) for x in xs]), **IDENT)],
                  expect=dict(status="OK", cells=[[1, 0, 0], [3, 0, 0]], counts=[1, 1],
                              out=pts([(x, 0.05, 0.05, 1.0) for x in xs]))))

# 3. Negative coordinates: floor, not truncation.
xn = [F(-0.01), F(-0.1), np.nextafter(F(-0.1), F(-1))]
cells3 = [int(np.floor(F(x * inv))) for x in xn]
assert cells3 == [-1, -1, -2], cells3
cases.append(dict(name="negative_floor", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts([(x, 0.05, 0.05, 0.0) for x in xn]), **IDENT)],
                  expect=dict(status="OK",
                              cells=[[-2, 0, 0], [-1, 0, 0]], counts=[1, 2],
                              out=pts([(xn[2], 0.05, 0.05, 0.0),
                                       (mean_seq([xn[0], xn[1]]), mean_seq([0.05, 0.05]),
                                        mean_seq([0.05, 0.05]), 0.0)]))))

# 4. min_points_per_voxel: voxels holding 1, 2, 3 points -> 3,3,2,1 voxels for 0,1,2,3.
p4 = [(0.05, 0.05, 0.05, 1.0),
      (0.15, 0.05, 0.05, 2.0), (0.16, 0.05, 0.05, 4.0),
      (0.25, 0.05, 0.05, 3.0), (0.26, 0.05, 0.05, 6.0), (0.27, 0.05, 0.05, 9.0)]
for mp, nvox in [(0, 3), (1, 3), (2, 2), (3, 1)]:
    groups = [[0], [1, 2], [3, 4, 5]]
    kept = [g for g in groups if len(g) >= mp]
    out = [[mean_seq([p4[i][k] for i in g]) for k in range(4)] for g in kept]
    assert len(out) == nvox
    cases.append(dict(name=f"min_points_{mp}", leaf=0.1, min_pts=mp, crop=None,
                      sensors=[dict(points=pts(p4), **IDENT)],
                      expect=dict(status="OK", out=pts(out), counts=[len(g) for g in kept],
                                  cells=[[len(g) - 1, 0, 0] for g in kept])))

# 5. Output order = ascending linear index: x fastest, then y, then z.
p5 = [(0.15, 0.05, 0.05, 1.0), (0.05, 0.15, 0.05, 2.0), (0.05, 0.05, 0.15, 3.0), (0.05, 0.05, 0.05, 4.0)]
cases.append(dict(name="ordering", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p5), **IDENT)],
                  expect=dict(status="OK", out=pts([p5[3], p5[0], p5[1], p5[2]]), counts=[1, 1, 1, 1],
                              cells=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])))

# 6. Crop inclusivity with the reference ROI (Parameter.h:31-35): closed interval, NaN dropped.
z6 = [F(-0.5), F(3.0), np.nextafter(F(3.0), F(10)), F(np.nan)]
p6 = [(1.0 + k, 0.0, z6[k], float(k)) for k in range(4)]
cases.append(dict(name="crop_inclusive", leaf=0.1, min_pts=0,
                  crop=dict(min=[-15.0, -5.0, -0.5], max=[60.0, 5.0, 3.0]),
                  sensors=[dict(points=pts(p6), is_dense=False, **IDENT)],
                  expect=dict(status="OK", merged=pts(p6[:2]), counts=[1, 1],
                              out=pts([p6[0], p6[1]]),
                              cells=[[10, 0, -5], [20, 0, 30]])))

# 7. Transform rounding: 90 degree yaw given as doubles.
s = float(np.sqrt(0.5))
q7 = [0.0, 0.0, s, s]
x, y, z, w = F(q7[0]), F(q7[1]), F(q7[2]), F(q7[3])
tx, ty, tz = F(2) * x, F(2) * y, F(2) * z
twx, twy, twz = F(tx * w), F(ty * w), F(tz * w)
txx, txy, txz = F(tx * x), F(ty * x), F(tz * x)
tyy, tyz, tzz = F(ty * y), F(tz * y), F(tz * z)
m7 = [F(1) - F(tyy + tzz), F(txy - twz), F(txz + twy), F(0.5),
      F(txy + twz), F(1) - F(txx + tzz), F(tyz - twx), F(-0.25),
      F(txz - twy), F(tyz + twx), F(1) - F(txx + tyy), F(0.125)]
pin = (F(1), F(2), F(3))
img = [F(F(F(m7[4 * r] * pin[0]) + F(m7[4 * r + 1] * pin[1])) + F(m7[4 * r + 2] * pin[2])) + m7[4 * r + 3]
       for r in range(3)]
cases.append(dict(name="transform_rounding", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts([(1.0, 2.0, 3.0, 7.0)]), q=q7, t=[0.5, -0.25, 0.125])],
                  expect=dict(status="OK", matrix=[bits(v) for v in m7],
                              merged=pts([(img[0], img[1], img[2], 7.0)]),
                              out=pts([(img[0], img[1], img[2], 7.0)]), counts=[1])))

# 8. Overflow guard: 40001^3 cells > INT32_MAX -> output = input.
p8 = [(-1000.0, -1000.0, -1000.0, 1.0), (1000.0, 1000.0, 1000.0, 2.0)]
cases.append(dict(name="overflow_guard", leaf=0.05, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p8), **IDENT)],
                  expect=dict(status="GRID_OVERFLOW", out=pts(p8))))

# 9. Concatenation order: sensor 0's points precede sensor 1's in the merged cloud.
p9a = [(0.05, 0.05, 0.05, 1.0), (0.55, 0.05, 0.05, 2.0)]
p9b = [(0.35, 0.05, 0.05, 3.0)]
cases.append(dict(name="concat_order", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p9a), **IDENT), dict(points=pts(p9b), **IDENT)],
                  expect=dict(status="OK", merged=pts(p9a + p9b), counts=[1, 1, 1],
                              out=pts([p9a[0], p9b[0], p9a[1]]),
                              cells=[[0, 0, 0], [3, 0, 0], [5, 0, 0]])))

# 10. Empty input: width = height = 0.
cases.append(dict(name="empty_input", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=[], **IDENT)],
                  expect=dict(status="EMPTY_INPUT", out=[])))

# 11. downsample_all_data = false: xyz only, intensity left at 0 (A.4 step 8).
cases.append(dict(name="xyz_only_centroid", leaf=0.1, min_pts=0, crop=None, downsample_all=False,
                  sensors=[dict(points=pts([a, b]), **IDENT)],
                  expect=dict(status="OK", out=pts([(c[0], c[1], c[2], 0.0)]), counts=[2])))

# 12. Subnormal intensity sums whose quotient is an exact tie in the subnormal range (9 / 6 = 1.5 ulps -> 2, even;
#     0xAB9 / 6 = 457.5 ulps -> 458; 27 / 18 = 1.5 ulps -> 2) and one just above the smallest normal value. Sums of
#     subnormals and of the dyadic coordinates here are exact in any order.
d = F(0.0625)
grp = [([1, 1, 1, 2, 2, 2], 0), ([0x1C9, 0x1C9, 0x1C9, 0x1CA, 0x1CA, 0x1CA], 1), ([1] * 9 + [2] * 9, 2), ([-1, -1, -1, -2, -2, -2], 3)]
p12, o12 = [], []
for ints, k in grp:
    xs = F((0.0625, 0.15625, 0.25, 0.3125)[k])         # dyadic: the sums of x are exact too
    rows = [(xs, d, d, sub(v)) for v in ints]
    p12 += rows
    o12.append([mean_exact([r[j] for r in rows]) for j in range(4)])
fm = np.array([0x00800000], dtype=np.uint32).view(F)[0]
rows = [(F(0.4625), d, d, np.nextafter(fm, F(1)))] * 2
p12 += rows
o12.append([mean_exact([r[j] for r in rows]) for j in range(4)])
assert [bits(v[3]) for v in o12] == [2, 0x1CA, 2, 0x80000002, bits(np.nextafter(fm, F(1)))]
cases.append(dict(name="subnormal_tie_quotients", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p12), **IDENT)],
                  expect=dict(status="OK", out=pts(o12), counts=[6, 6, 18, 6, 2],
                              cells=[[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]])))

# 13. Subnormal and signed-zero coordinates, translation -0.0: a negative subnormal x lands in cell -1, a positive one in
#     cell 0; -0.0 survives the transform only where every term is -0.0 (merged cloud), and the centroid of a voxel of
#     -0.0 values (x and intensity) is +0.0: pcl's accumulator starts at +0.0f.
NZ = dict(q=[0.0, 0.0, 0.0, 1.0], t=[-0.0, -0.0, -0.0])
e = F(0.1625)
p13 = [(sub(3), e, e, F(1.0)), (sub(-3), d, d, F(2.0)), (sub(5), e, e, F(3.0)), (sub(-0x7FFFFF), d, d, F(4.0)),
       (F(-0.0), F(-0.0), F(-0.0), F(-0.0)), (F(-0.0), F(-0.0), F(-0.0), F(-0.0))]
m13 = [r for r in p13]                                    # identity, t = -0.0: every coordinate keeps its bits
o13 = [[mean_exact([r[j] for r in p13[:1] + p13[2:3]]) for j in range(4)],
       [mean_exact([r[j] for r in [p13[1], p13[3]]]) for j in range(4)],
       [mean_exact([r[j] for r in p13[4:]]) for j in range(4)]]
assert bits(o13[0][0]) == 4 and bits(o13[1][0]) == bits(F(-(sub(3) + sub(0x7FFFFF)) / F(2)))
assert [bits(v) for v in o13[2]] == [0, 0, 0, 0]
cases.append(dict(name="subnormal_and_signed_zero_coordinates", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p13), **NZ)],
                  expect=dict(status="OK", merged=pts(m13),
                              cells=[[-1, 0, 0], [0, 0, 0], [0, 1, 1]], counts=[2, 2, 2],
                              out=pts([o13[1], o13[2], o13[0]]))))

# 14. Finite intensities whose sum overflows: 3e38 + 3e38 = +inf (+inf / 2 = +inf), the same negated, and 3 x 1e38.
p14 = [(F(0.05), d, d, F(3e38)), (F(0.06), d, d, F(3e38)),
       (F(0.15), d, d, F(-3e38)), (F(0.16), d, d, F(-3e38)),
       (F(0.25), d, d, F(1e38)), (F(0.25), d, d, F(1e38)), (F(0.25), d, d, F(1e38))]
o14 = [[mean_exact([r[j] for r in p14[a:b]]) for j in range(4)] for a, b in ((0, 2), (2, 4), (4, 7))]
assert np.isposinf(o14[0][3]) and np.isneginf(o14[1][3]) and np.isfinite(o14[2][3])
cases.append(dict(name="overflowing_intensity_sums", leaf=0.1, min_pts=0, crop=None,
                  sensors=[dict(points=pts(p14), **IDENT)],
                  expect=dict(status="OK", out=pts(o14), counts=[2, 2, 3], cells=[[0, 0, 0], [1, 0, 0], [2, 0, 0]])))

# 15. Voxel faces at leaf 0.05 (fl32(1/0.05f) = 20.000002f): the fp32 value nearest k * 0.05 and 1, 2 ulps to either
#     side, near the origin and 1 km out, each point alone in a voxel (a y row of its own); crop faces at
#     non-representable values with points on them and 1 ulp outside.
inv5 = F(1) / F(0.05)
p15, c15 = [], []
row = 0
for k in (3, -7, 20001):
    face = F(k * 0.05)
    for dd in (-2, -1, 0, 1, 2):
        x = face
        for _ in range(abs(dd)):
            x = np.nextafter(x, F(np.inf) if dd > 0 else F(-np.inf))
        y = F(0.125 * row + 0.0625)
        row += 1
        p15.append((x, y, F(0.0125), F(row)))
crop15 = dict(min=[-1.03, -0.07, -0.0327], max=[1000.07, 3.07, 0.0327])
lo, hi = [F(v) for v in crop15["min"]], [F(v) for v in crop15["max"]]
for a, lim in ((2, lo[2]), (2, hi[2])):
    for dd in (-1, 0, 1):
        v = lim if dd == 0 else np.nextafter(lim, F(np.inf) if dd > 0 else F(-np.inf))
        y = F(0.125 * row + 0.0625)
        row += 1
        p15.append((F(0.5125), y, v, F(row)))
kept = [r for r in p15 if all(not (r[a] < lo[a] or r[a] > hi[a]) for a in range(3))]
assert len(kept) == len(p15) - 2
cl = [tuple(int(np.floor(F(r[a] * (inv5)))) for a in range(3)) for r in kept]
assert len(set(cl)) == len(cl)
order = sorted(range(len(kept)), key=lambda i: (cl[i][2], cl[i][1], cl[i][0]))
cases.append(dict(name="face_ulps_and_crop_faces", leaf=0.05, min_pts=0, crop=crop15,
                  sensors=[dict(points=pts(p15), **IDENT)],
                  expect=dict(status="OK", merged=pts(kept), counts=[1] * len(kept),
                              cells=[list(cl[i]) for i in order], out=pts([kept[i] for i in order]))))

here = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(here, "known_answers.json"), "w") as f:
    json.dump(dict(note="SURVEY.md Appendix B known-answer cases; floats as uint32 bit patterns "
                        "[x,y,z,intensity]; derived by tests/golden/make_known_answers.py",
                   cases=cases), f, indent=1)
print("wrote", len(cases), "cases")
