"""The vectorised restatement of jacobi3 (tests/jacobi_ref.py) against the scalar one of the ground stage
(tests/ground_ref.py::jacobi3, which test_ground pins to the device bit for bit): the same bits on every matrix."""
import numpy as np

from tests import ground_ref, jacobi_ref


def matrices():
    rng = np.random.default_rng(41)
    out = []

    def sym(m):
        return (m + np.swapaxes(m, 1, 2)) * 0.5

    out.append(sym(rng.normal(size=(1500, 3, 3))))                                   # generic
    d = np.zeros((300, 3, 3))
    d[:, [0, 1, 2], [0, 1, 2]] = rng.normal(size=(300, 3))
    out.append(d)                                                                    # diagonal
    u = rng.normal(size=(400, 3))
    out.append(u[:, :, None] * u[:, None, :])                                        # rank 1
    u[:200] = np.round(u[:200] * 4) / 4                                              # ... with exact entries
    out.append(u[:, :, None] * u[:, None, :])
    w = rng.normal(size=(400, 3))
    out.append(u[:, :, None] * u[:, None, :] + w[:, :, None] * w[:, None, :])       # rank 2
    q, _ = np.linalg.qr(rng.normal(size=(400, 3, 3)))
    lam = rng.uniform(0.1, 2.0, (400, 3))
    lam[:, 1] = lam[:, 0]                                                            # a repeated eigenvalue
    lam[:100, 2] = lam[:100, 0]                                                      # all three
    out.append(sym(np.einsum("nik,nk,njk->nij", q, lam, q)))
    a, b = rng.uniform(0.5, 2, 100), rng.uniform(-0.4, 0.4, 100)
    out.append(a[:, None, None] * np.eye(3) + b[:, None, None] * np.ones((3, 3)))   # exactly a I + b 11^T
    out.append(np.ones((1, 3, 3)) * np.array([1.0, 0.25, 3.0, 0.0])[:, None, None])  # c 11^T, and the zero matrix
    cov = np.array([[9, -3, -3], [-3, 9, -3], [-3, -3, 9]], np.float64) / 64         # the tetrahedron's
    out.append(cov[None])
    base = sym(rng.normal(size=(200, 3, 3)))
    out.append(base * 1e150)
    out.append(base * 1e-150)
    out.append(base * 1e-299)                                                        # entries on either side of the 1e-300 skip
    out.append(base * 1e-301)
    tiny = base.copy()
    tiny[:, 0, 1] = tiny[:, 1, 0] = rng.choice([1e-300, 9.9e-301, -1e-300, 1.1e-300, 0.0, -0.0], 200)
    out.append(tiny)
    return np.concatenate(out)


def test_vectorised_jacobi_equals_the_scalar_one_bit_for_bit():
    m = matrices()
    assert len(m) >= 4000
    a, v = jacobi_ref.jacobi3(m)
    assert (m == np.swapaxes(m, 1, 2)).all()
    for k in range(len(m)):
        sa, sv = ground_ref.jacobi3(m[k].tolist())
        assert np.array(sa).tobytes() == a[k].tobytes() and np.array(sv).tobytes() == v[k].tobytes(), k
    # the set is not trivial: rotations happened, and rotations were skipped
    assert (np.abs(v[:, 0, 1]) > 0.1).sum() > 1000 and (v == np.eye(3)).all(axis=(1, 2)).sum() >= 300
    # and it is an eigen-decomposition where the scale allows the check
    ok = np.abs(m).max(axis=(1, 2)) < 1e100
    lam = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1)
    back = np.einsum("nik,nk,njk->nij", v, lam, v)
    scale = np.abs(m).max(axis=(1, 2))
    assert (np.abs(back - m).max(axis=(1, 2))[ok] <= 1e-13 * scale[ok] + 1e-299).all()


def test_input_is_left_alone_and_sweeps_matter():
    m = matrices()[:200]
    keep = m.copy()
    a12, _ = jacobi_ref.jacobi3(m)
    assert m.tobytes() == keep.tobytes()
    a2, _ = jacobi_ref.jacobi3(m, sweeps=2)
    assert a2.tobytes() != a12.tobytes()
