"""What a context takes it gives back, and a call in its steady state takes nothing: the counts of the test build
(-DCM_TEST_HOOKS: every DevBuf / PinnedBuf of cm_devbuf.hpp counts the allocations alive in the process and the allocations
made so far; the shipped library counts nothing).

Each case runs in a child process with CM_LIB_VARIANT=testhooks — a process loads one build of the library —: this module,
started as `python -m tests.test_ctx_memory <case>`, runs the case's function. The shapes are those of
tests/test_byproduct_reuse.py: a context of 8192 points, results of about 300 voxels, then more than 4096, then about 300 again
(one tile, two tiles, one tile), the smallest at which every grow path of the by-products runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud
from tests import test_align as al
from tests import test_ndt as nd
from tests.test_byproduct_reuse import CAP, FLAGS, K, LATTICE_LEAF, TOL, five_calls, lattice_frame, sources, sparse_lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LEAF = (LATTICE_LEAF,) * 3
# cm_create with CM_FLAG_OCCUPANCY: keys_a/b, vals_a/b, hist, grp, seg_tile_counts, seg_groups, partials, totals, seg_counts,
# merged_total, out, out_key, out_cnt, d_frame, d_tiles, h_tile_kept, d_state[0], d_state[1], h_state
CREATE_BUFFERS = 21
GRIDS = [((-2.0, -2.0), 0.5, 24, 20), ((-2.0, -2.0), 0.25, 60, 50)]          # the second one larger: both tables grow


def allocations():
    live, total = capi.device_allocations()
    print(f"live {live} total {total}")
    return live, total


def new_context():
    return capi.CloudMerger(max_points_total=CAP, max_sensors=1, flags=FLAGS)


def plain_frame(cm, xyz):
    cm.submit(0, xyzi_cloud(xyz, np.ones(len(xyz), F32)))
    res = cm.merge_voxelize(MergeParams(leaf=LEAF, min_points_per_voxel=1))
    assert res.status == capi.OK and res.n_out > 0
    return res


def map_calls(cm, grids=GRIDS):
    """The by-products that five_calls does not make: the boxes, and the grid map and the rays at each grid."""
    cm.cluster_boxes(TOL)
    for origin, cell, nx, ny in grids:
        cm.grid_map(origin, cell, nx, ny)
        cm.grid_rays(origin, cell, nx, ny)


def case_destroy_returns_everything():
    assert allocations() == (0, 0)
    cm = new_context()
    xyz = sparse_lattice((9, 9, 8), 1)
    # the pre-stages, each switched on for a frame: ground removal with its radius filter, ego-motion, statistical outliers
    cm.set_ground_removal(capi.make_ground_params([[(-1.0, 100.0, 0.5)]], outlier_radius=1.1, outlier_min_neighbors=1))
    plain_frame(cm, xyz)
    cm.ground(CAP)                                   # (refused unless the frame ran the stage)
    cm.set_ground_removal(None)
    t_ref = 1_700_000_000_000_000_000
    cm.set_ego_motion(capi.make_motion((12.0, 0.5, 0.0), (0.01, 0.0, 0.3), t_ref, [t_ref - 20_000_000]))
    assert plain_frame(cm, xyz).path_flags & capi.PATH_MOTION
    cm.set_ego_motion(None)
    cm.set_statistical_outlier(8, 0.5)
    assert plain_frame(cm, xyz).path_flags & capi.PATH_SOR
    cm.set_statistical_outlier(None)
    # a host submit and a published result at both output steps, a frame between them (the result buffers swap)
    for step_out in (16, 32):
        res = plain_frame(cm, xyz)
        dst = np.zeros(res.n_out * step_out, np.uint8)
        cm.publish_async(dst.ctypes.data, res.n_out, step_out)
        cm.publish_wait()
        assert dst.any()
        assert len(cm.result(res.n_out, 32)) == res.n_out and len(cm.merged(CAP)) == len(xyz)
    # a partial table, and the merge of that table
    cm.submit(0, xyzi_cloud(xyz, np.ones(len(xyz), F32)))
    params = MergeParams(leaf=LEAF, min_points_per_voxel=1)
    lo, hi, _ = cm.local_bounds(params)
    assert cm.merge_partial(params, np.concatenate([lo, hi])).status == capi.OK
    ptr, n = cm.partial_device()
    assert n == len(xyz)
    assert cm.merge_tables([ptr], [n], params).n_out == len(xyz)
    # every by-product over the three result sizes
    for step in range(3):
        res, pts = lattice_frame(cm, step)
        five_calls(cm, res, pts, LEAF, TOL, checked=False)
        map_calls(cm)
    live, _ = allocations()
    assert live >= CREATE_BUFFERS
    cm.close()
    assert allocations()[0] == 0


def unchanged(what, call):
    """call() twice with the same arguments: the second one allocates nothing."""
    call()
    before = allocations()[1]
    call()
    assert allocations()[1] == before, what


def case_steady_state_allocates_nothing():
    with new_context() as cm:
        res, pts = lattice_frame(cm, 0)
        src = sources(pts, 300)
        (origin, cell, nx, ny), = GRIDS[:1]
        calls = {
            "clusters": lambda: cm.clusters(TOL),
            "boxes": lambda: cm.cluster_boxes(TOL),
            "normals": lambda: cm.normals(K, (5.0, 4.0, 40.0)),
            "covariance": lambda: cm.voxel_covariance(res.n_out),
            "align": lambda: (cm.align(src, TOL, guess=al.GUESS, max_iterations=3, normals_k=K), cm.align_correspondences(len(src))),
            "ndt": lambda: (cm.ndt_align(src, guess=nd.GUESS, max_iterations=3), cm.ndt_correspondences(len(src))),
            "grid map": lambda: cm.grid_map(origin, cell, nx, ny),
            "grid rays": lambda: cm.grid_rays(origin, cell, nx, ny),
            "merged cloud": lambda: cm.merged(CAP),
            "32-byte result": lambda: cm.result(res.n_out, 32),
        }
        for what, call in calls.items():
            unchanged(what, call)

    # identical frames through merge_voxelize with ground removal, with statistical outlier removal (the two are not combined)
    # and with neither (the bucket path's buffers and the quantile passes'): the second frame allocates nothing, nor does any
    # later one. The host submits go to the slot's two staging buffers in turn: both exist from the third submit on.
    xyz = sparse_lattice((9, 9, 8), 1)
    cloud = xyzi_cloud(xyz, np.ones(len(xyz), F32))
    params = MergeParams(leaf=LEAF, min_points_per_voxel=1)
    for pre_stage in ("ground", "sor", None):
        with new_context() as cm:
            if pre_stage == "ground":
                cm.set_ground_removal(capi.make_ground_params([[(-1.0, 100.0, 0.5)]], outlier_radius=1.1, outlier_min_neighbors=1))
            if pre_stage == "sor":
                cm.set_statistical_outlier(8, 0.5)
            totals = []
            for frame in range(4):
                cm.submit(0, cloud)
                totals.append(allocations()[1])
                assert cm.merge_voxelize(params).status == capi.OK
                totals.append(allocations()[1])
            assert len(set(totals[2:])) == 1, (pre_stage, totals)


def case_growing_replaces_shrinking_keeps():
    with new_context() as cm:
        seen = []
        for step in range(3):
            res, pts = lattice_frame(cm, step)
            five_calls(cm, res, pts, LEAF, TOL, checked=False)
            map_calls(cm, GRIDS[:1])
            seen.append(allocations())
        (_, total_one), (live_two, total_two), (live_back, _) = seen
        assert live_back == live_two, "nothing is freed on shrink, nothing is duplicated on grow"
        assert total_two > total_one, "the two-tile result made the tables grow"


# What each layer of the occupancy map allocates at tests/test_map_layer_texts.py's configuration (every DevBuf and PinnedBuf of
# its struct in cm_ctx.hpp), recorded from the commit before the layer table (428edbf) with this case copied into its tree.
LAYER_BUFFERS = dict(map=5, cost=4, plan=4, traj=4, front=5, match=5, search=6, mcl=9, cast=7)


def case_map_layers_give_back_their_subtrees():
    from tests import test_map_layer_texts as lt
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        w = lt.Walk(cm)
        w.frame()
        base = allocations()[0]
        took = {}
        for layer in lt.LAYERS:
            before = allocations()[0]
            w.configure[layer]()
            took[layer] = allocations()[0] - before
        assert took == LAYER_BUFFERS
        live_all, total = allocations()
        # a producer call on every layer allocates nothing: the configure calls made every buffer
        cm.map_integrate()
        cm.map_cost_update()
        cm.map_plan_update(*lt.HERE)
        cm.map_path(*lt.HERE)
        cm.map_traj_evaluate(lt.HERE[0], lt.HERE[1], 0.0)
        cm.map_frontier_update()
        cm.map_match(lt.POSE)
        cm.map_match_search(lt.POSE)
        cm.map_mcl_init_pose(lt.HERE[0], lt.HERE[1], 0.0)
        cm.map_mcl_predict(0.0, 0.0, 0.0)
        cm.map_mcl_update()
        cm.map_mcl_init_uniform()
        cm.map_mcl_update()
        cm.map_cast([(lt.HERE[0], lt.HERE[1], 0.0)])
        assert allocations() == (live_all, total), "a producer call allocated"
        # a leaf layer configured again with the same parameters keeps its buffers
        for layer in ("traj", "front", "match", "search", "mcl", "cast"):
            w.configure[layer]()
            assert allocations() == (live_all, total), layer
        # a layer given back takes its subtree along, and nothing else
        cm.map_plan_configure(None)
        assert allocations()[0] == live_all - sum(took[k] for k in ("plan", "traj", "front"))
        cm.map_cost_configure(None)
        assert allocations()[0] == base + took["map"]
        cm.map_configure(None)
        assert allocations() == (base, total), "giving back allocates nothing and leaves nothing"
        # ... and from the full tree in one call
        for layer in lt.LAYERS:
            w.configure[layer]()
        assert allocations()[0] == live_all
        cm.map_configure(None)
        assert allocations()[0] == base


CASES = {f.__name__[len("case_"):]: f for f in (case_destroy_returns_everything, case_steady_state_allocates_nothing,
                                                case_growing_replaces_shrinking_keeps, case_map_layers_give_back_their_subtrees)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_ctx_memory(case):
    if not os.path.exists(os.path.join(ROOT, "cloud_merger_amd", "lib", "libcloudmerge_hip_testhooks.so")):
        pytest.skip("test build missing: python -m cloud_merger_amd.build --test-hooks")
    env = {k: v for k, v in os.environ.items() if k not in ("CM_PATH", "CM_QUANT", "CM_DEBUG_MISRANK")}
    env.update(CM_LIB_VARIANT="testhooks", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "tests.test_ctx_memory", case], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]


if __name__ == "__main__":
    CASES[sys.argv[1]]()
