"""The by-product calls on one context over results that grow and shrink, and over sources that grow and shrink: what the
buffers they keep between calls (cm_byproducts.cpp: PairSort, SearchIndex, PoseFit) must survive, and the order of the stages
they mark.

No bar of its own: every table goes through the checker of its own suite (test_cluster.check, test_normals.check,
test_align.check_eval, test_voxel_cov.check_table, test_ndt.check_eval — the restatements of tests/*_ref.py), and what a
context computes after it has grown and shrunk equals, byte for byte, what a fresh context computes."""
import ctypes as C

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import test_align as al
from tests import test_ndt as nd
from tests import test_normals as nm
from tests import test_voxel_cov as vc
from tests.test_cluster import check as check_clusters
from tests.test_cluster import hip_rt, submit_as_voxels

F32 = np.float32
FLAGS = capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE
CAP = 8192                                   # two tiles of CM_TILE = 4096
LATTICE_LEAF = 0.25
CORNER_LEAF = nd.LEAF
TOL = 1.05                                   # cluster tolerance and matching radius on the lattices: just above their pitch
K = 7


def sparse_lattice(dims, seed):
    """Every other point of an integer lattice, at random and shuffled: a giant component and many small ones at TOL."""
    g = [np.arange(m, dtype=F32) for m in dims]
    xyz = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    xyz = xyz[rng.random(len(xyz)) < 0.5]
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


def sources(xyz, n, seed=11):
    """n points near the cloud: some within reach of a centroid or a voxel, some not."""
    rng = np.random.default_rng(seed)
    return (xyz[rng.integers(0, len(xyz), n)] + rng.uniform(-0.6, 0.6, (n, 3))).astype(F32)


# result sizes: one tile, two tiles, one tile again (lattices: n_out == len(xyz); corners: the padded INPUT crosses the tile)
LATTICES = [((9, 9, 8), 1), ((22, 22, 21), 2), ((9, 8, 9), 3)]
CORNERS = [(1300, 17), (2700, 18), (1300, 19)]


def lattice_frame(cm, step):
    dims, seed = LATTICES[step]
    xyz = sparse_lattice(dims, seed)
    assert (250 <= len(xyz) <= 400) if step != 1 else (4096 < len(xyz) <= CAP)
    return submit_as_voxels(cm, xyz, LATTICE_LEAF, 0), xyz


def corner_frame(cm, step):
    n_per, seed = CORNERS[step]
    pts = nd.noisy_corner(n_per=n_per, seed=seed)
    assert (len(pts) <= 4096) if step != 1 else (4096 < len(pts) <= CAP)
    cm.submit(0, xyzi_cloud(pts, np.ones(len(pts), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=CORNER_LEAF, min_points_per_voxel=1))
    assert res.status == capi.OK and 80 <= res.n_out <= 400
    counts = cm.cells(res.n_out)[1]
    assert (counts >= 6).mean() > 0.5
    return res, pts


def five_calls(cm, res, pts, leaf, tol, checked=True):
    """All five calls on the result at rest, each through its suite's checker; what they returned, as bytes."""
    src = sources(pts, 300)
    if checked:
        check_clusters(cm, res, tol)
        nm.check(cm, res, K, (5.0, 4.0, 40.0), tree=False, normals=False)
        vc.check_table(cm, res, leaf, CAP)
        al.check_eval(cm, res, src, tol, al.GUESS, k=K)
        nd.check_eval(cm, res, src, leaf, nd.GUESS)
    out = [x.tobytes() for x in cm.clusters(tol)]
    out.append(cm.normals(K, (5.0, 4.0, 40.0)).tobytes())
    out.append(cm.voxel_covariance(res.n_out).tobytes())
    out.append(al.result_bytes(cm.align(src, tol, guess=al.GUESS, max_iterations=3, normals_k=K)))
    out.append(cm.align_correspondences(len(src)).tobytes())
    out.append(nd.result_bytes(cm.ndt_align(src, guess=nd.GUESS, max_iterations=3)))
    out.append(cm.ndt_correspondences(len(src)).tobytes())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["lattice", "corner"])
def test_results_that_grow_and_shrink(scene):
    frame, leaf, tol = (lattice_frame, (LATTICE_LEAF,) * 3, TOL) if scene == "lattice" else (corner_frame, CORNER_LEAF, 0.75)
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        for step in range(3):
            res, pts = frame(cm, step)
            last = five_calls(cm, res, pts, leaf, tol)
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        res, pts = frame(cm, 2)
        assert five_calls(cm, res, pts, leaf, tol, checked=False) == last


def device_copy(hip, rec):
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(rec.nbytes)) == 0
    assert hip.hipMemcpy(ptr, C.c_void_p(rec.ctypes.data), C.c_size_t(rec.nbytes), 1) == 0
    return ptr


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_sources_that_grow_and_shrink(where):
    """1, 3 and 1 blocks of CM_BLOCK = 256 source records against one result."""
    hip = hip_rt()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        res, pts = corner_frame(cm, 0)
        src = sources(pts, 700)
        outs = []
        for n in (100, 700, 100):
            s = src[:n]
            if where == "host":
                al.check_eval(cm, res, s, 0.75, al.GUESS, k=K)
                assert len(cm.align_correspondences(1000)) == n
                nd.check_eval(cm, res, s, CORNER_LEAF, nd.GUESS)
                assert len(cm.ndt_correspondences(1000)) == n
                a = cm.align(s, 0.75, guess=al.GUESS, max_iterations=3, normals_k=K)
                ca = cm.align_correspondences(1000)
                b = cm.ndt_align(s, guess=nd.GUESS, max_iterations=3)
                cb = cm.ndt_correspondences(1000)
            else:
                rec = np.zeros((n, 4), F32)
                rec[:, :3] = s
                ptr = device_copy(hip, rec)
                try:
                    a = cm.align_device(ptr.value, n, 0.75, guess=al.GUESS, max_iterations=3, normals_k=K)
                    ca = cm.align_correspondences(1000)
                    b = cm.ndt_align_device(ptr.value, n, guess=nd.GUESS, max_iterations=3)
                    cb = cm.ndt_correspondences(1000)
                finally:
                    assert hip.hipFree(ptr) == 0
                # the host entry points: the same bytes
                assert al.result_bytes(cm.align(s, 0.75, guess=al.GUESS, max_iterations=3, normals_k=K)) == al.result_bytes(a)
                assert cm.align_correspondences(1000).tobytes() == ca.tobytes()
                assert nd.result_bytes(cm.ndt_align(s, guess=nd.GUESS, max_iterations=3)) == nd.result_bytes(b)
                assert cm.ndt_correspondences(1000).tobytes() == cb.tobytes()
            assert len(ca) == n and len(cb) == n
            outs.append((al.result_bytes(a), ca.tobytes(), nd.result_bytes(b), cb.tobytes()))
        assert outs[2] == outs[0] and outs[1] != outs[0]


def stage_names(cm):
    return [name for name, _ in cm.stage_times()]


def stage_lists():
    """The stages each call marks on a one-tile result, in order."""
    out = {}
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        _, xyz = lattice_frame(cm, 0)
        src = sources(xyz, 300)
        cm.clusters(TOL)
        out["clusters"] = stage_names(cm)
        cm.normals(K)
        out["normals"] = stage_names(cm)
        cm.align(src, TOL, guess=al.GUESS, max_iterations=2, normals_k=K)
        out["align"] = stage_names(cm)
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        _, pts = corner_frame(cm, 0)
        src = sources(pts, 300)
        cm.ndt_align(src, guess=nd.GUESS, max_iterations=2)
        out["ndt, computing the table"] = stage_names(cm)
        cm.ndt_align(src, guess=nd.GUESS, max_iterations=2)
        out["ndt, holding the table"] = stage_names(cm)
    return {call: ["k_nrm_rings n=" if s.startswith("k_nrm_rings n=") else s for s in names] for call, names in out.items()}


# Recorded from a run of stage_lists() against the parent of the commit that gave the by-products their own translation unit
# (commit ea650ee, "Add NDT scan registration against the voxel covariance table"; one MI355X, the library built from that
# commit's tree, this file copied into it): the full lists, so that order and count are held.
FRONT_END = ["k_cl_bounds", "k_cl_keys", "k_scatter(cells)", "k_hist", "k_scatter(cells)", "k_cl_gather", "cl_rows"]
STAGES = {
    "clusters": FRONT_END + ["k_cl_hook", "k_cl_roots", "k_cl_count", "k_cl_number", "k_cl_labels", "k_scatter(lists)", "k_cl_decode"],
    "normals": FRONT_END + ["k_nrm_knn(block)", "k_nrm_rings n="],
    # (one entry per name: the second scatter pass is the first one's entry)
    "align": ["k_cl_bounds", "k_cl_keys", "k_scatter(cells)", "k_hist", "k_cl_gather", "cl_rows", "k_aln_eval", "k_aln_sum", "aln_readback"],
    "ndt, computing the table": ["voxel_cov", "k_cl_bounds", "k_ndt_eval", "k_aln_sum", "ndt_readback"],
    "ndt, holding the table": ["k_cl_bounds", "k_ndt_eval", "k_aln_sum", "ndt_readback"],
}


@pytest.mark.gpu
def test_stage_lists():
    got = stage_lists()
    assert list(got) == list(STAGES)
    for call, names in got.items():
        assert names == STAGES[call], call


@pytest.mark.gpu
def test_an_empty_result():
    """CM_OK with no voxel at all (min_points_per_voxel above every voxel's count) in a fresh context: every call returns
    empty tables, the registrations their guess, CM_*_FEW and a table without a match. The values are the parent's (commit ea650ee),
    recorded in the run the stage lists are from."""
    xyz = sparse_lattice(*LATTICES[0])
    src = sources(xyz, 300)
    with capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS) as cm:
        cm.submit(0, xyzi_cloud(xyz, np.ones(len(xyz), F32)))
        res = cm.merge_voxelize(MergeParams(leaf=(LATTICE_LEAF,) * 3, min_points_per_voxel=2))
        assert res.status == capi.OK and res.n_out == 0 and res.n_merged == len(xyz)
        assert [len(x) for x in cm.clusters(TOL)] == [0, 0, 0]
        assert tuple(cm.clusters_device(TOL)) == (None, None, None, 0, 0)
        assert len(cm.normals(K)) == 0 and tuple(cm.normals_device(K)) == (None, 0)
        assert len(cm.voxel_covariance(0)) == 0 and tuple(cm.voxel_covariance_device(6, 0.01)) == (None, 0)
        a = cm.align(src, TOL, guess=al.GUESS, max_iterations=3, normals_k=K)
        assert np.array_equal(np.array(a.pose[:]).reshape(3, 4), al.GUESS)
        assert not any(a.H[:]) and not any(a.g[:]) and not any(a.pivot[:]) and a.sse == 0 and a.rms == 0
        assert (a.n_corr, a.iterations, a.flags) == (0, 0, capi.ALIGN_FEW)
        corr = cm.align_correspondences(1000)
        assert len(corr) == 300 and (corr["idx"] == capi.ALIGN_NONE).all() and not corr["d2"].any()
        b = cm.ndt_align(src, guess=nd.GUESS, max_iterations=3)
        assert np.array_equal(b.pose_matrix(), nd.GUESS)
        assert not any(b.H[:]) and not any(b.g[:]) and not any(b.pivot[:]) and b.score == 0
        assert (b.gauss_d1, b.gauss_d2) == (float.fromhex("-0x1.ecc50a4736ec0p-4"), float.fromhex("0x1.e842b0c66a915p-1"))
        assert (b.n_corr, b.iterations, b.flags) == (0, 0, capi.NDT_FEW)
        corr = cm.ndt_correspondences(1000)
        assert len(corr) == 300 and (corr["idx"] == capi.NDT_NONE).all() and not corr["n_used"].any() and not corr["score"].any()
        assert stage_names(cm) == ["k_ndt_eval", "k_aln_sum", "ndt_readback"]
