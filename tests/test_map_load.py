"""cm_map_load: a recorded occupancy map put back (include/cloudmerge.h; localisation in a map that was built earlier is the
main use of the localisation layer). Two frames are integrated in one context, the state is copied and loaded into a second
context: the state, the image and both tables of the cost layer are equal bytes, and integrating the same third frame under
the same pose in both contexts gives equal maps. The CPU part restates the image of a loaded table by tests/map_ref.py."""
import ctypes as C

import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams
from tests import map_ref as mr
from tests import test_grid_map as tg
from tests import test_grid_rays as tr
from tests import test_occupancy_map as tm

LOAD_TYPES = (capi.MclParams,)                       # (a library without cm_map_load fails every test here, at import)
SEQ = tm.SEQUENCES["fractional"]                     # three poses, the window scrolls between them
PARAMS = MergeParams(**tm.COARSE)


def test_the_image_of_a_table_on_the_restatement():
    """Step 8 on hand-made cells: unobserved cells are unknown whatever their logodds, the thresholds are closed."""
    q = mr.params(0.5, 4, 2)
    lo = np.array([[q["l_occ"], q["l_occ"] - 1, q["l_free"], q["l_free"] + 1], [q["l_max"], q["l_min"], 0, q["l_max"]]], np.int32)
    n = np.array([[1, 1, 1, 1], [0, 0, 7, 0xFFFFFFFF]], np.uint32)
    assert mr.image_of(lo, n, q).tolist() == [[100, -1, 0, -1], [-1, -1, -1, 100]]


def states(cm):
    table, info = cm.map()
    image, _ = cm.map_occupancy()
    cm.map_cost_update()
    cost, dist2, _ = cm.map_cost()
    return table, image, cost, dist2, info


@pytest.mark.gpu
def test_a_loaded_map_is_the_recorded_map():
    seed, q, poses, _ = SEQ
    frames = tm.frames_of(seed, 3)
    n_cap = tm.n_cap_of(frames)
    with capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as a, capi.CloudMerger(max_points_total=n_cap, max_sensors=3) as b:
        for cm in (a, b):
            tm.configure(cm, q)
            cm.map_cost_configure(0.35, 1.05, 3.0, True)
        for parts, P in zip(frames[:2], poses[:2]):
            tg.run_frame(a, tr.clouds_of(parts, tm.TRANS[:3]), PARAMS)
            a.map_integrate(P)
        ta, ia, ca, da, info_a = states(a)
        assert (ia == 0).sum() > 100 and (ia == 100).sum() > 20 and info_a.n_frames == 2
        # b holds a frame of its own while the map is loaded: it counts as not yet integrated
        tg.run_frame(b, tr.clouds_of(frames[2], tm.TRANS[:3]), PARAMS)
        info_b = b.map_load(ta, tuple(info_a.anchor))
        assert tm.info_tuple(info_b) == (tuple(info_a.anchor), q["nx"], q["ny"], 1, 0, 0)
        tm.refused(b, b.map_cost, text=b"stale")                       # as after an integration
        tb, ib, cb, db, _ = states(b)
        assert tb.tobytes() == ta.tobytes() and ib.tobytes() == ia.tobytes() and cb.tobytes() == ca.tobytes() and db.tobytes() == da.tobytes()
        assert ib.tobytes() == mr.image_of(ta["logodds"], ta["n_obs"], q).astype(np.int8).tobytes()
        b.map_integrate(poses[2])                                      # the frame b held
        tg.run_frame(a, tr.clouds_of(frames[2], tm.TRANS[:3]), PARAMS)
        a.map_integrate(poses[2])
        ta3, ia3, ca3, da3, i3a = states(a)
        tb3, ib3, cb3, db3, i3b = states(b)
        assert ta3.tobytes() != ta.tobytes() and tuple(i3a.anchor) != tuple(info_a.anchor)
        assert tb3.tobytes() == ta3.tobytes() and ib3.tobytes() == ia3.tobytes() and cb3.tobytes() == ca3.tobytes() and db3.tobytes() == da3.tobytes()
        assert tuple(i3b.anchor) == tuple(i3a.anchor) and (i3a.n_frames, i3b.n_frames) == (3, 2) and i3a.sensors_cast == i3b.sensors_cast
        tm.refused(b, b.map_integrate, poses[2], text=b"already integrated")


@pytest.mark.gpu
def test_refusals_of_a_load():
    q = mr.params(0.5, 12, 10)
    n = 120
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        L = cm._lib
        good = np.zeros(n, capi.MAP_DTYPE)
        good["logodds"][:5] = (q["l_min"], q["l_max"], -1, 1, 0)
        good["n_obs"][:5] = 1
        anchor = (C.c_int32 * 2)(3, -4)
        info = capi.MapInfo()
        keep = bytes(info)
        call = lambda t, cells, a, out=None: L.cm_map_load(cm._ctx, t.ctypes.data if t is not None else None, cells, C.byref(a) if a is not None else None, out)
        assert call(good, n, anchor, C.byref(info)) == capi.BAD_ARG and b"cm_map_configure" in L.cm_last_error(cm._ctx) and bytes(info) == keep
        tm.configure(cm, q)
        before = cm.map()[0].tobytes()
        for cells in (n - 1, n + 1, 0):
            assert call(good, cells, anchor, C.byref(info)) == capi.BAD_ARG and b"nx * ny" in L.cm_last_error(cm._ctx)
        for at, v in ((0, q["l_min"] - 1), (n - 1, q["l_max"] + 1), (50, -(1 << 31))):
            bad = good.copy()
            bad["logodds"][at] = v
            assert call(bad, n, anchor, C.byref(info)) == capi.BAD_ARG and b"logodds" in L.cm_last_error(cm._ctx)
        for ax, ay in ((1 << 30, 0), (0, -(1 << 30)), (-(1 << 31), 0)):
            assert call(good, n, (C.c_int32 * 2)(ax, ay), C.byref(info)) == capi.BAD_ARG and b"anchor" in L.cm_last_error(cm._ctx)
        assert call(None, n, anchor) == capi.BAD_ARG and call(good, n, None) == capi.BAD_ARG
        assert bytes(info) == keep and cm.map()[0].tobytes() == before and cm.map()[1].n_frames == 0
        assert call(good, n, (C.c_int32 * 2)((1 << 30) - 1, -(1 << 30) + 1), None) == capi.OK
        assert call(good, n, anchor, C.byref(info)) == capi.OK and tm.info_tuple(info) == ((3, -4), 12, 10, 1, 0, 0)
        assert cm.map()[0].reshape(-1).tobytes() == good.tobytes()
        assert cm.map_occupancy()[0].reshape(-1)[:6].tolist() == [0, 100, -1, -1, -1, -1]
