"""Zone-wise ground removal restated in plain numpy / Python, apart from oracle/ (no ctypes) and from the kernels: what
oracle/cm_oracle.h (orc_ransac_plane) and include/cloudmerge.h (cm_zone, cm_ground_params) define.

Number formats: every fp32 operation is one numpy float32 operation (rounded once, never contracted), the sample
generator runs in Python integers, the refit's sums are float64 in the header's blocked order and the Jacobi iteration
runs in Python floats (IEEE double, math.sqrt correctly rounded).

  classify      slab and fate (band / kept / dropped) of every point of a transformed + cropped cloud
  sample3       the three distinct indices of hypothesis j of a zone
  plane_from_3  PCL's plane through three points, fp32
  inlier        |a x + b y + c z + d| < threshold, strict, fp32
  ransac        PCL's accept / stop loop over the hypothesis sequence, then the refit
  refit         least-squares plane through the inliers
  radius_keep   RadiusOutlierRemoval by brute force (strict d2 < r2, more than min_neighbors points itself included)
  ground_split  the stage for one sensor: same signature and return value as oracle.ground_split
"""
import math

import numpy as np

F = np.float32
M64 = (1 << 64) - 1
DROPPED, BAND, KEPT = 0, 1, 2
SPARE = 24                                 # hypotheses beyond max_iterations that skipped samples may use up
CHUNK, PARTIALS = 8192, 256                # the refit's blocked order
EPS = 2.220446049250313e-16


# ---- slabs and bands ----------------------------------------------------------------------------------------------------
def slab_limits(zone):
    """(x0, x1, zmax, zlo) of a slab (x_min, x_length, z_max_ground) as fp32: x1 is the fp32 sum, zlo the double sum
    zmax + 0.01 rounded to fp32"""
    x0, ln, zm = F(zone[0]), F(zone[1]), F(zone[2])
    return x0, F(x0 + ln), zm, F(np.float64(zm) + 0.01)


def classify(xyz, zones, z_keep_max):
    """slab (index into zones, -1: none) and fate (DROPPED / BAND / KEPT) per point. The first slab in table order whose
    closed interval [x0, x1] holds x takes the point; there a negative zmax keeps it, the closed band [-zmax, zmax]
    sends it to the plane fit, the closed interval [zlo, z_keep_max] keeps it, everything else is dropped."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    x, z = xyz[:, 0], xyz[:, 2]
    slab = np.full(len(xyz), -1, np.int64)
    fate = np.full(len(xyz), DROPPED, np.int64)
    zk = F(z_keep_max)
    for k in reversed(range(len(zones))):                  # later slabs first, earlier ones overwrite: first wins
        x0, x1, zm, zlo = slab_limits(zones[k])
        inside = (x >= x0) & (x <= x1)
        slab[inside] = k
        if zm < 0:
            fate[inside] = KEPT
        else:
            fate[inside] = np.where((z >= -zm) & (z <= zm), BAND, np.where((z >= zlo) & (z <= zk), KEPT, DROPPED))[inside]
    return slab, fate


# ---- samples ------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sample3(seed, zone_key, j, n):
    """three distinct indices in [0, n), n >= 3: the k-th is drawn uniformly from the n - k indices not yet taken
    (high 64 bits of random * range), counted over the free indices in ascending order"""
    base = (int(seed) ^ (int(zone_key) << 40) ^ (int(j) << 2)) & M64
    draw = lambda k: (splitmix64((base + k) & M64) * (n - k)) >> 64
    i0 = draw(0)
    i1 = draw(1)
    i1 += i1 >= i0
    i2 = draw(2)
    for taken in sorted((i0, i1)):
        i2 += i2 >= taken
    return i0, i1, i2


# ---- planes -------------------------------------------------------------------------------------------------------------
def plane_from_3(p0, p1, p2):
    """SampleConsensusModelPlane::computeModelCoefficients in fp32: None for a collinear (or repeated) sample, else
    (a, b, c, d) with unit normal (p1 - p0) x (p2 - p0) and d = -n . p0"""
    p0, p1, p2 = (np.asarray(p, np.float32) for p in (p0, p1, p2))
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        r = a / b
        if r[0] == r[1] and r[2] == r[1]:
            return None
        n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)
        ln = np.sqrt(F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        if not ln > 0:
            return None
        n = n / ln
        d = F(-1.0) * F(F(n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])
    pl = np.array([n[0], n[1], n[2], d], np.float32)
    return pl if np.isfinite(pl).all() else None


def distance(pl, xyz):
    """signed fp32 distance ((a x + b y) + c z) + d of every point"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pl = np.asarray(pl, np.float32)
    with np.errstate(all="ignore"):
        return ((pl[0] * xyz[:, 0] + pl[1] * xyz[:, 1]) + pl[2] * xyz[:, 2]) + pl[3]


def inlier(pl, xyz, threshold):
    return np.abs(distance(pl, xyz)) < F(threshold)


def jacobi3(a):
    """cyclic Jacobi on a symmetric 3x3 (lists of Python floats), 12 sweeps over the pairs (0,1), (0,2), (1,2); returns
    the rotated matrix and the eigenvectors as columns"""
    a = [list(r) for r in a]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(12):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if abs(apq) < 1e-300:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):                                       # columns p, q
                a[k][p], a[k][q] = c * a[k][p] - s * a[k][q], s * a[k][p] + c * a[k][q]
            for k in range(3):                                       # rows p, q
                a[p][k], a[q][k] = c * a[p][k] - s * a[q][k], s * a[p][k] + c * a[q][k]
            for k in range(3):
                v[k][p], v[k][q] = c * v[k][p] - s * v[k][q], s * v[k][p] + c * v[k][q]
    return a, v


def blocked_sums(xyz, mask):
    """the ten sums (x y z xx xy xz yy yz zz 1) over the masked points in float64: chunks of 8192 points of the band;
    inside a chunk element i adds to partial i mod 256 in order, the partials fold pairwise (128, 64, .. 1), the chunk
    sums add up one after the other. (A point outside the mask contributes +0.0, which changes no partial: none of
    them can be -0.0.)"""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    terms = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z, np.ones(len(p))], 1) * np.asarray(mask)[:, None]
    total = np.zeros(10)
    for c0 in range(0, len(p), CHUNK):
        rows = np.zeros((CHUNK, 10))
        rows[:len(terms[c0:c0 + CHUNK])] = terms[c0:c0 + CHUNK]
        part = np.zeros((PARTIALS, 10))
        for r in rows.reshape(CHUNK // PARTIALS, PARTIALS, 10):
            part = part + r
        stride = PARTIALS // 2
        while stride:
            part = part[:stride] + part[stride:2 * stride]
            stride //= 2
        total = total + part[0]
    return [float(v) for v in total]


def refit(xyz, mask):
    """optimizeModelCoefficients: mean and covariance of the masked points, normal = eigenvector of the smallest
    eigenvalue, d = -n . mean; None if the result is not finite"""
    S = blocked_sums(xyz, mask)
    cnt = S[9]
    m = [S[0] / cnt, S[1] / cnt, S[2] / cnt]
    a = [[0.0] * 3 for _ in range(3)]
    for (i, j), s in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), S[3:9]):
        a[i][j] = a[j][i] = s / cnt - m[i] * m[j]
    a, v = jacobi3(a)
    k = 0
    if a[1][1] < a[k][k]:
        k = 1
    if a[2][2] < a[k][k]:
        k = 2
    n = [v[0][k], v[1][k], v[2][k]]
    ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    try:
        n = [c / ln for c in n]
    except ZeroDivisionError:
        return None
    d = -1.0 * ((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2])
    if not all(math.isfinite(c) for c in n + [d]):
        return None
    return np.array(n + [d], np.float64).astype(np.float32)


class Plane:
    """the result of ransac: the fields of the oracle's PlaneResult plus skipped and band_points"""

    def __init__(self, n):
        self.found, self.plane, self.n_inliers, self.iterations, self.skipped, self.best_hypothesis = 0, [0.0] * 4, 0, 0, 0, 0
        self.band_points = n
        self.end = "none"                  # how the loop ended: "max" | "probability" | "spare" | "none" (n < 3)


def ransac(xyz, max_iterations=1000, threshold=0.3, probability=0.99, optimize=True, seed=12345, zone_key=0):
    """PCL's RandomSampleConsensus::computeModel over hypotheses j = 0, 1, ..: a collinear sample is skipped and is no
    iteration; a hypothesis replaces the best with strictly more inliers; the loop ends after more than max_iterations
    iterations, once (1 - w^3)^iterations <= 1 - probability (the power by repeated multiplication), or when
    max_iterations + 24 hypotheses are used up. Returns (Plane, inlier mask)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    res, mask = Plane(n), np.zeros(n, bool)
    if n < 3:
        return res, mask
    iterations = skipped = 0
    best, best_pl = -1, None
    pno = pw = 1.0
    stop = 1.0 - float(F(probability))
    res.end = "spare"
    while iterations + skipped < max_iterations + SPARE:
        j = iterations + skipped
        pl = plane_from_3(*(xyz[i] for i in sample3(seed, zone_key, j, n)))
        if pl is None:
            skipped += 1
            continue
        c = int(inlier(pl, xyz, threshold).sum())
        iterations += 1
        if c > best:
            best, best_pl, res.best_hypothesis = c, pl, j
            w = c / n
            pno = min(max(1.0 - (w * w) * w, EPS), 1.0 - EPS)
            pw = 1.0
            for _ in range(iterations):
                pw *= pno
        else:
            pw *= pno
        if iterations > max_iterations:
            res.end = "max"
            break
        if not pw > stop:
            res.end = "probability"
            break
    res.iterations, res.skipped = iterations, skipped
    if best < 0:
        return res, mask
    res.found = 1
    pl = best_pl
    if optimize and best > 3:
        better = refit(xyz, inlier(pl, xyz, threshold))
        if better is not None:
            pl = better
    mask = inlier(pl, xyz, threshold)
    res.plane, res.n_inliers = [float(v) for v in pl], int(mask.sum())
    return res, mask


# ---- the band's radius filter ---------------------------------------------------------------------------------------------
def radius_keep(xyz, radius, min_neighbors=1):
    """a point stays iff more than min_neighbors points of the set, itself included, lie at fp32 squared distance
    (dx*dx + dy*dy) + dz*dz strictly below fl32(double(r) * double(r)) (FLANN's strict radius test)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    r2 = F(np.float64(F(radius)) * np.float64(F(radius)))
    keep = np.zeros(len(xyz), bool)
    for i0 in range(0, len(xyz), 512):
        d = xyz[i0:i0 + 512, None, :] - xyz[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        keep[i0:i0 + 512] = (d2 < r2).sum(1) > min_neighbors
    return keep


# ---- the stage for one sensor ---------------------------------------------------------------------------------------------
def ground_split(points, zones, sensor, gp):
    """oracle.ground_split's contract: points are the transformed + cropped records of one sensor (fields x, y, z),
    zones its slab table, gp the RANSAC numbers. Returns (keep mask, ground mask, planes): planes[k] is None for a
    slab kept whole, else the Plane of slab k (zone key sensor * 8 + k) with band_points set."""
    xyz = np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float32)
    slab, fate = classify(xyz, zones, gp["z_keep_max"])
    keep = fate == KEPT
    ground = np.zeros(len(xyz), bool)
    planes = []
    for k, zone in enumerate(zones):
        if F(zone[2]) < 0:
            planes.append(None)
            continue
        idx = np.nonzero((slab == k) & (fate == BAND))[0]
        res, inl = ransac(xyz[idx], gp["max_iterations"], gp["threshold"], gp["probability"], gp["optimize"], gp["seed"],
                          sensor * 8 + k)
        ground[idx[inl]] = True
        rest = idx[~inl]
        if gp.get("outlier_radius", 0) and len(rest):
            rest = rest[radius_keep(xyz[rest], gp["outlier_radius"], gp.get("outlier_min_neighbors", 1))]
        keep[rest] = True
        planes.append(res)
    return keep, ground, planes
