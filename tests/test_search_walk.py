"""The walks of the by-products' search grid at the grid's edges (cm_search.hpp: for_row_cells, for_rows_3x3, for_row_ring).

The cluster hook, the normals' and the outlier removal's k-NN and the ICP match all walk the sorted cells of a search grid
through the same three helpers, so a mistake at a grid edge would be everybody's at once. Here the grid is degenerate along
each axis in turn: a straight line along x, y and z (two dimensions of one cell: a single row, or rows of a single cell), a
planar cloud in each coordinate plane (one dimension of one cell), and a block of 3 x 3 x 3 cells with one point per cell
and a second one in the centre cell (the centre's walks meet all 27 cells, the corners' are clipped on three sides, and in
the hook "my own row up to myself" is a range of one). Tolerance, radius and search cell are chosen so that the cell is
1.00390625 m everywhere (cluster_grid: 1.00390625 tol; the grid starts at the cloud's minimum).

Every call is judged exactly as in its own test file, by the restatement that file uses: clusters bit for bit
(test_cluster.check, cluster_ref), normals by test_normals.check (normals_ref; neighbour lists, distances and flags bit for
bit), one ICP evaluation by test_align.check_eval (align_ref; correspondences bit for bit, sums by value), the outlier
removal by test_sor.check_frame (sor_ref, brute force; distances and statistics bit for bit). On the CPU: the clouds have the
geometry claimed above, and every restatement runs on every cloud.
"""
import functools

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import align_ref as ar
from tests import cluster_ref as cr
from tests import normals_ref as nr
from tests import sor_ref as sr
from tests import test_align, test_cluster, test_normals, test_sor

F32 = np.float32
TOL = 1.0
CELL = 1.00390625                     # cluster_grid's cell for TOL, and the cell asked of normals and the outlier removal
K = 8
KS = (8, 5)                           # the normals' k: past the 27 cells for many points, and mostly inside them
VIEWPOINT = (3.0, -2.0, 40.0)
SHAPES = ["line_x", "line_y", "line_z", "plane_xy", "plane_xz", "plane_yz", "block"]
# where the neighbourhoods are collinear the smallest two eigenvalues coincide and a normal is any vector across the line:
# compared as test_normals compares its tied lattices (normals=False: lists, flags, residual and orientation)
COLLINEAR = {"line_x", "line_y", "line_z"}


@functools.lru_cache(maxsize=None)
def cloud(shape):
    """Finite float32 points, every one its own voxel at a leaf of 1/16 m (coordinates of lines and planes are multiples of 1/8)."""
    rng = np.random.default_rng(SHAPES.index(shape) + 11)
    if shape.startswith("line_"):
        # steps that put neighbours into one cell, into adjacent cells and two cells apart; 1.0 is the tolerance itself
        steps = rng.choice(F32([0.25, 0.75, 1.0, 2.0, 2.5]), 600)
        t = np.concatenate([[0.0], np.cumsum(steps[:-1], dtype=np.float64)]).astype(F32)
        xyz = np.zeros((len(t), 3), F32)
        xyz[:, "xyz".index(shape[-1])] = t
        xyz += F32([2.0, -3.0, 1.0])
    elif shape.startswith("plane_"):
        uv = np.unique(rng.integers(0, 8 * 36, (1500, 2)), axis=0).astype(F32) / F32(8)
        uv = uv[rng.permutation(len(uv))]
        xyz = np.full((len(uv), 3), F32(1.5))
        xyz[:, "xyz".index(shape[-2])] = uv[:, 0] - F32(7)
        xyz[:, "xyz".index(shape[-1])] = uv[:, 1] + F32(2)
    else:
        ijk = np.stack(np.meshgrid(*(np.arange(3),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
        u = rng.uniform(0.3, 0.8, (27, 3))
        u[ijk == 0] = 0.25                                  # the grid starts at the minimum: cell 0 begins at 0.25 cells
        u[13] = 0.3
        pts = (ijk + u) * CELL
        xyz = np.concatenate([pts, [[1.6 * CELL] * 3]]).astype(F32)
    return np.ascontiguousarray(xyz, F32)


def cells_of(xyz):
    """The search cell of every point: k_cl_keys' arithmetic for the grid of cluster_grid(TOL)."""
    inv = F32(1) / F32(CELL)
    return np.floor((xyz - xyz.min(axis=0)).astype(F32) * inv).astype(np.int64)


def sources(shape):
    """The ICP sources: the cloud moved by up to 0.6 m along every axis (so some leave the grid sideways and some match
    nothing) and points beyond both ends of every axis, nearer and farther than the radius."""
    xyz = cloud(shape)
    rng = np.random.default_rng(5)
    moved = xyz + rng.uniform(-0.6, 0.6, xyz.shape).astype(F32)
    ends = []
    for a in range(3):
        for p, s in ((xyz[xyz[:, a].argmin()], -1.0), (xyz[xyz[:, a].argmax()], 1.0)):
            for d in (0.5, 1.5, 40.0):
                q = p.copy(); q[a] += F32(s * d)
                ends.append(q)
    return np.ascontiguousarray(np.concatenate([moved, F32(ends)]), F32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_the_clouds_have_the_geometry_claimed(shape):
    xyz = cloud(shape)
    assert np.isfinite(xyz).all() and 28 <= len(xyz) <= 2000
    assert len(np.unique(np.floor(xyz / F32(0.0625)).astype(np.int64), axis=0)) == len(xyz)      # a voxel each
    c = cells_of(xyz)
    dims = c.max(axis=0) + 1
    if shape.startswith("line_"):
        a = "xyz".index(shape[-1])
        assert dims[a] > 300 and np.delete(dims, a).tolist() == [1, 1]
        assert {0, 1, 2} <= set(np.diff(c[:, a]).tolist())
        gaps = np.diff(xyz[:, a])
        assert (gaps == F32(TOL)).any() and (gaps < TOL).any() and (gaps > 2 * CELL).any()
    elif shape.startswith("plane_"):
        flat = "xyz".index(({"x", "y", "z"} - set(shape[-2:])).pop())
        assert dims[flat] == 1 and (np.delete(dims, flat) >= 30).all()
    else:
        assert dims.tolist() == [3, 3, 3]
        keys, counts = np.unique(c, axis=0, return_counts=True)
        assert len(keys) == 27 and counts.max() == 2 and keys[counts == 2].tolist() == [[1, 1, 1]]


@pytest.mark.parametrize("shape", SHAPES)
def test_every_restatement_runs_on_every_cloud(shape):
    xyz = cloud(shape)
    labels, table, members = cr.clusters_tree(xyz, TOL)
    assert 2 <= len(table) < len(xyz)                                       # what test_cluster.expected asks for
    for a, b in zip((labels, table, members), cr.clusters_brute(xyz, TOL)):
        assert a.tobytes() == b.tobytes()
    labels, table, _ = cr.clusters_tree(xyz, TOL, 2, 50)
    assert len(table) >= 2 and (labels == cr.NONE).any()
    for k in KS:
        want, pl = nr.table(xyz, k, VIEWPOINT, tree=False)
        assert (want["flags"] == nr.VALID).all()
        clear = (pl["evals"][:, 1] - pl["evals"][:, 0]) >= 1e-3 * pl["evals"][:, 2]
        # test_normals.compare's gap rule leaves out at most 1 % of the entries, or the cloud is compared without normals
        assert (~clear).sum() <= 0.01 * len(xyz) if shape not in COLLINEAR else not clear.any()
    src = sources(shape)
    ev = ar.evaluate(src, xyz, want, test_align.EYE, TOL, tree=False)
    matched = ev["corr"]["idx"] != ar.NONE
    assert matched.sum() >= 10 and (~matched).sum() >= 10
    d, (mean, sd, thr), keep = sr.sor(xyz, K, 1.0, brute=True)
    assert np.isfinite(d).all() and np.isfinite([mean, sd, thr]).all() and keep.any()
    assert d.view(np.uint32).tolist() == sr.sor(xyz, K, 1.0, cell=CELL)[0].view(np.uint32).tolist()


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_clusters_normals_and_icp_match(shape):
    xyz = cloud(shape)
    with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1, flags=capi.FLAG_OCCUPANCY) as cm:
        res = test_cluster.submit_as_voxels(cm, xyz, 0.0625, 0)
        test_cluster.check(cm, res, TOL)
        test_cluster.check(cm, res, TOL, 2, 50)
        for k in KS:
            test_normals.check(cm, res, k, VIEWPOINT, search_cell=CELL, tree=False, normals=shape not in COLLINEAR)
        got, corr, _ = test_align.check_eval(cm, res, sources(shape), TOL, k=K)
        assert (corr["idx"] != ar.NONE).sum() >= 10 and (corr["idx"] == ar.NONE).sum() >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_statistical_outlier_removal(shape, monkeypatch):
    monkeypatch.setenv("CM_PATH", "classic")
    xyz = cloud(shape)
    sensors, n_cap = [xyzi_cloud(xyz, np.ones(len(xyz), F32))], len(xyz)
    params = MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=1)
    P = test_sor.merged_input(sensors, n_cap, params)
    assert test_sor.xyz_of(P).tobytes() == xyz.tobytes()
    ref = sr.sor(xyz, K, 1.0, brute=True)
    test_sor.check_frame(P, test_sor.run_sor(sensors, n_cap, params, K, 1.0, cell=CELL)[0], K, 1.0, params, n_cap, ref=ref)
