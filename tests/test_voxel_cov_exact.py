"""The kernel-order restatement of the covariance table (tests/voxel_cov_exact.py) on its own, without a GPU: the known
answers test_voxel_cov.py holds the eigh restatement to, and agreement of the two restatements within that file's
tolerances on well-conditioned voxels — so the exact one is no blind copy of the kernel."""
import numpy as np

from cloud_merger_amd import capi
from tests import voxel_cov_exact as vx
from tests import voxel_cov_ref as vr


def one_voxel(pts, min_points=6, eig_mult=0.01):
    pts = np.asarray(pts, dtype=np.float32)
    t, info = vx.voxel_stats(pts, np.zeros(len(pts), np.int64), 1, min_points, eig_mult)
    return t[0], info["lam"][0]


def test_known_answer_tetrahedron():
    """Population covariance 3/16 and -1/16; PCL's (n - 1) / n makes that 9/64 and -3/64. Eigenvalues 3/64, 12/64, 12/64: not
    inflated at 0.01. Inverse (16/3)(I + J)."""
    e, lam = one_voxel([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], min_points=3)
    assert e["count"] == 4 and np.array_equal(e["mean"], np.float32([0.25, 0.25, 0.25]))
    assert np.array_equal(e["cov"], np.float32([9, -3, -3, 9, -3, 9]) / np.float32(64))
    assert e["flags"] == capi.COV_VALID
    assert np.allclose(lam, [3 / 64, 12 / 64, 12 / 64], rtol=1e-14)
    assert np.allclose(e["evals"], [3 / 64, 12 / 64, 12 / 64], rtol=1e-6)
    assert np.allclose(e["icov"], np.array([2, 1, 1, 2, 1, 2]) * 16 / 3, rtol=1e-5)


def test_known_answer_planar_voxel_is_inflated():
    pts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (.5, .5, 0), (.25, .75, 0)]
    e, lam = one_voxel(pts)
    assert lam[0] == 0.0
    assert e["flags"] == capi.COV_VALID | capi.COV_INFLATED
    l2 = e["evals"][2]
    assert l2 > 0 and e["evals"][0] == np.float32(np.float64(np.float32(0.01)) * lam[2])
    c = capi.sym6_to_3x3(e["cov"].astype(np.float64))
    assert abs(c[2, 2] - 0.01 * l2) < 1e-7 and abs(c[0, 2]) < 1e-7 and abs(c[1, 2]) < 1e-7
    x = np.array([p[0] for p in pts])
    assert abs(c[0, 0] - x.var() * 5 / 6) < 1e-7
    assert np.allclose(capi.sym6_to_3x3(e["icov"].astype(np.float64)) @ c, np.eye(3), atol=1e-4)
    # without inflation the exact zero eigenvalue passes the eigenvalue test and fails the inverse: det == 0
    e0, _ = one_voxel(pts, eig_mult=0.0)
    assert e0["flags"] == 0 and e0["cov"].any() and not e0["icov"].any() and not e0["evals"].any()
    # eig_mult 1: every eigenvalue raised to lambda_2
    e1, lam1 = one_voxel(pts, eig_mult=1.0)
    assert e1["flags"] == capi.COV_VALID | capi.COV_INFLATED and (e1["evals"] == np.float32(lam1[2])).all()


def test_known_answer_identical_points_are_invalid():
    e, _ = one_voxel([(1.0, -2.0, 0.5)] * 8)
    assert e["count"] == 8 and np.array_equal(e["mean"], np.float32([1.0, -2.0, 0.5]))
    assert e["flags"] == 0 and not e["cov"].any() and not e["icov"].any() and not e["evals"].any()


def test_known_answer_below_min_points_has_count_and_mean_only():
    e, _ = one_voxel([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], min_points=6)
    assert e["count"] == 5 and np.array_equal(e["mean"], np.float32([0.4, 0.4, 0.4]))
    assert e["flags"] == 0 and not e["cov"].any() and not e["icov"].any() and not e["evals"].any()


def test_sums_are_sequential():
    pts = np.float32([(1e16, 0, 0), (1, 0, 0), (-1e16, 0, 0), (1, 0, 0)])
    e, _ = one_voxel(pts, min_points=3)
    assert e["mean"][0] == np.float32(((1e16 + 1.0) - 1e16 + 1.0) / 4)


def test_ties_keep_their_place_in_the_sort():
    l = np.array([[2.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 2.0, 1.0], [3.0, 2.0, 1.0], [1.0, 1.0, 0.5], [np.nan, 1.0, 0.0]])
    assert vx.ascending(l).tolist() == [[1, 2, 0], [0, 1, 2], [0, 2, 1], [2, 1, 0], [2, 0, 1], [0, 2, 1]]   # (a NaN loses no comparison)
    assert vx.ascending(l, strict=False).tolist()[:2] == [[2, 1, 0], [2, 1, 0]]


def test_the_two_restatements_agree():
    """Random well-conditioned voxels (3 to 40 points, blobs of every aspect down to 1:30, some thin enough to inflate):
    count and mean the same bits, flags equal, the covariance of every voxel that was not inflated the same bits, the rest
    within check_table's tolerances (1e-5 lambda_2 on cov and evals, 1e-4 of the largest entry on icov)."""
    rng = np.random.default_rng(77)
    n_vox = 3000
    cnt = rng.integers(3, 41, n_vox)
    vox = np.repeat(np.arange(n_vox), cnt)
    centre = rng.uniform(-60, 60, (n_vox, 3))
    q, _ = np.linalg.qr(rng.normal(size=(n_vox, 3, 3)))
    sig = 0.1 * 10 ** rng.uniform(-1.5, 0, (n_vox, 3))
    xyz = centre[vox] + np.einsum("nij,nj->ni", q[vox], rng.normal(size=(len(vox), 3)) * sig[vox])
    perm = rng.permutation(len(vox))                                  # the points of a voxel are scattered over the cloud
    xyz, vox = xyz[perm].astype(np.float32), vox[perm]
    for min_points, eig_mult in ((6, 0.01), (3, 0.05), (10, 0.0)):
        a, info = vx.voxel_stats(xyz, vox, n_vox, min_points, eig_mult)
        b, lam = vr.voxel_stats(xyz, vox, n_vox, min_points, eig_mult)
        big = a["count"] >= min_points
        l2 = lam[:, 2]
        well = big & (lam[:, 0] > 1e-9 * l2)
        assert well.sum() > 0.6 * n_vox
        assert a["count"].tobytes() == b["count"].tobytes() and a["mean"].tobytes() == b["mean"].tobytes()
        assert np.array_equal(a["flags"][well], b["flags"][well]) and not a["flags"][~big].any()
        assert (np.abs(info["lam"][well] - lam[well]) <= 1e-12 * l2[well, None]).all()
        plain = well & ((a["flags"] & capi.COV_INFLATED) == 0)
        infl = well & ~plain
        if eig_mult:
            assert infl.sum() > 100
        assert a["cov"][plain].tobytes() == b["cov"][plain].tobytes()
        ok = well & ((a["flags"] & capi.COV_VALID) != 0)
        assert ok.sum() > 0.5 * n_vox
        tol = 1e-5 * np.abs(b["evals"][:, 2].astype(np.float64))[:, None]
        assert (np.abs(a["cov"][infl].astype(np.float64) - b["cov"][infl]) <= tol[infl]).all()
        assert (np.abs(a["evals"][ok].astype(np.float64) - b["evals"][ok]) <= tol[ok]).all()
        scale = np.abs(b["icov"][ok].astype(np.float64)).max(axis=1, keepdims=True)
        assert (np.abs(a["icov"][ok].astype(np.float64) - b["icov"][ok]) <= 1e-4 * scale).all()


def test_first_difference_names_voxel_and_field():
    pts = np.float32(np.random.default_rng(1).uniform(0, 0.4, (24, 3)))
    t, _ = vx.voxel_stats(pts, np.repeat(np.arange(3), 8), 3, 6, 0.01)
    assert vx.first_difference(t, t.copy()) is None
    u = t.copy()
    u["icov"][2, 4] = np.nextafter(u["icov"][2, 4], np.float32(np.inf))
    u["flags"][2] = 0
    k, f, got, want = vx.first_difference(u, t)
    assert (k, f) == (2, "icov") and got[4] != want[4]
