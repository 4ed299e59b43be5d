"""Every by-product and every map layer in the three regimes the shipped code runs in and the other suites do not: on a caller's
stream (cm_set_stream, the *_device entry points ordered by that stream alone), in the published pipeline with asynchronous
submits (cm_result_publish_async followed by the next frame, the node shell's order of calls), and with four contexts busy on
four threads.

The calls, the scenes and every expected value are tests/regimes.py's: the collections of the other suites held to their
restatements, byte for byte. The guards on the references run before a device output is read; the CPU tests below run them
again with the library's own direction table and hold the scenes apart."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch                                   # torch first: one HIP runtime per process (its bundled one)

from cloud_merger_amd import capi
from tests import regimes as rg
from tests import test_align as al
from tests import test_byproduct_layouts as bl
from tests import test_byproduct_reuse as bu
from tests import test_ndt as nd

F32 = np.float32
DIFFER = ("merged", "grid", "rays", "map", "dist2", "match_volume", "mcl_weights")
# what a host-built table decides: the cost table, the match and localisation tables, the cast layer's directions
TABLE_BOUND = ("match_volume", "mcl_init", "mcl_weights")
TABLE_BOUND_LAYERS = ("cost", "pot", "traj", "cast_rays")
REFUSED = "cannot change stream with a frame in flight"


# ---- CPU: the references, their guards and their differences ---------------------------------------------------------------------
def test_the_scenes_pass_their_guards_and_differ():
    """restated() and layers_restated() assert their vacuity guards while they build a reference (with capi.traj_directions(),
    the library's own table): building all of them is the test. The small scene's seed is the first from 60 on that passes."""
    refs = [rg.scene_ref(seed) for seed in rg.SEEDS] + [rg.scene_ref("small")]
    for name in DIFFER:
        assert len({r.want[name] for r in refs}) == len(refs), name
    for name in ("pot", "traj", "cast_rays"):                    # (the frontiers of two scenes may coincide: the walls are the same)
        assert len({r.want_layers[name] for r in refs}) == len(refs), name
    small = refs[-1]
    assert max(small.counts) <= 300 and small.seed == 61 and len(small.frame.A) < 800 and min(len(r.frame.A) for r in refs[:-1]) > 10000
    with pytest.raises(AssertionError):
        rg.SceneRef(60, rg.SMALL_COUNTS)


def test_the_second_parameter_set_changes_every_table():
    """Scene 42 under the second set against scene 42 under the first: a table shared between two contexts would give one of
    them the other's bytes, and these differ."""
    a, b = rg.scene_ref(42, "a"), rg.scene_ref(42, "b")
    assert a.want["merged"] == b.want["merged"] and a.want["map"] == b.want["map"] and a.want["dist2"] == b.want["dist2"]
    for name in TABLE_BOUND:
        assert a.want[name] != b.want[name], name
    for name in TABLE_BOUND_LAYERS:
        assert a.want_layers[name] != b.want_layers[name], name
    pa, pb = a.pset, b.pset
    assert capi.match_table(bl.CELL, pa["match"]["sigma"], pa["match"]["max_dist"]).tobytes() != \
        capi.match_table(bl.CELL, pb["match"]["sigma"], pb["match"]["max_dist"]).tobytes()
    assert capi.cast_directions(a.lset["range_cells"]).tobytes() != capi.cast_directions(b.lset["range_cells"]).tobytes()
    for k in ("n_particles", "max_beams", "seed", "sigma", "max_dist"):
        assert pa["mcl"][k] != pb["mcl"][k], k


def test_the_lattices_are_restated():
    for step in range(3):
        xyz, tables = rg.lattice_ref(step)
        assert len(tables) == 2 and len({t[0] for t in tables}) == 2
    first = [rg.lattice_ref(step)[1][0] for step in range(3)]
    assert len({t[0] for t in first}) == 3 and first[0][2] != first[1][2]      # the counts of every step, the rays of two


# ---- regime 1: a caller's stream -----------------------------------------------------------------------------------------------------
def torch_cuda():
    assert torch.cuda.is_available()
    return torch


class HipStream:
    """A non-blocking stream made with the runtime's own call, as an integrating node makes it."""

    def __init__(self):
        self.hip, self.handle = rg.hip(), C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(self.handle), 1) == 0 and self.handle.value      # hipStreamNonBlocking

    def close(self):
        assert self.hip.hipStreamSynchronize(self.handle) == 0 and self.hip.hipStreamDestroy(self.handle) == 0


def every_collection(scene_cm, lattice_cm, ref, label, steps=(0, 1)):
    rg.check_scene(scene_cm, ref, label)
    for step in steps:
        res, _ = bu.lattice_frame(lattice_cm, step)
        rg.check_lattice(lattice_cm, res, step, f"{label}, lattice {step}")
    rg.check_shapes(lattice_cm, rg.shapes_frame(lattice_cm), f"{label}, shapes")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hip", "torch"])
def test_every_collection_on_a_callers_stream(kind):
    """The frame with the blocking calls and every collection on a stream the caller made, while that stream always has work
    of the caller's queued: a launch or a wait that went to the context's own stream runs ahead of what it depends on."""
    torch = torch_cuda()
    ref = rg.scene_ref(41)
    raw = HipStream() if kind == "hip" else None
    stream = torch.cuda.ExternalStream(raw.handle.value) if raw else torch.cuda.Stream()
    try:
        with rg.scene_context() as cm, rg.lattice_context() as lm:
            cm.set_stream(stream.cuda_stream)
            lm.set_stream(stream.cuda_stream)
            with rg.BusyStream(stream):
                rg.blocking_frame(cm, ref)
                every_collection(cm, lm, ref, f"{kind} stream")
    finally:
        if raw:
            raw.close()


@pytest.mark.gpu
def test_stream_switches_between_the_frame_and_its_by_products():
    """The frame on stream A, the collections on stream B, then on the context's own stream: the same frame, the tables the
    context kept between the calls used across streams, the same bytes. cm_set_stream(0) is cm_set_stream(NULL); while a frame
    is in flight the call is refused and changes nothing."""
    torch = torch_cuda()
    ref = rg.scene_ref(41)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with rg.scene_context() as cm, rg.lattice_context() as lm:
        cm.set_stream(a.cuda_stream)
        lm.set_stream(a.cuda_stream)
        rg.blocking_frame(cm, ref)
        res, _ = bu.lattice_frame(lm, 1)
        cm.set_stream(b.cuda_stream)
        lm.set_stream(b.cuda_stream)
        with rg.BusyStream(b):
            rg.check_scene(cm, ref, "frame on A, by-products on B")
            rg.check_lattice(lm, res, 1, "frame on A, by-products on B")
            cm.set_stream(None)
            lm.set_stream(None)
            # (B still has work queued: the context's own stream is not ordered behind it, and must not need to be)
            rg.check_settled(cm, ref, "tables made on B, used on the own stream")
            rg.check_scene(cm, ref, "back on the own stream")
            rg.check_lattice(lm, res, 1, "back on the own stream")
        # a null handle by its number: torch.cuda.current_stream().cuda_stream is 0 on torch's default stream
        assert torch.cuda.default_stream().cuda_stream == 0
        # Stream.query() tells whether a stream holds unfinished work: it does with a backlog queued ...
        keep = rg.backlog(torch, b)
        assert not b.query()
        b.synchronize()
        del keep
        # ... and B stays idle while a frame enqueued after set_stream(None) or set_stream(0) is in flight: nothing went to B. (No
        # time is compared: streams may share a hardware queue, so how long the own stream takes says nothing.)
        for handle in (None, 0):
            cm.set_stream(b.cuda_stream)
            cm.set_stream(handle)
            cm.submit_all(rg.scene_ref(42).clouds)
            assert cm.merge_voxelize_async(capi.make_params(bl.PARAMS)) == capi.OK
            idle = b.query()
            assert cm.wait().status == capi.OK
            assert idle, f"set_stream({handle}): the frame went to the caller's stream"
            rg.check_scene(cm, rg.scene_ref(42), f"after set_stream({handle})")
        # a frame in flight: refused with the present text, and the frame finishes on the stream it was enqueued on
        cm.set_stream(a.cuda_stream)
        cm.submit_all(ref.clouds)
        assert cm.merge_voxelize_async(capi.make_params(bl.PARAMS)) == capi.OK
        for handle in (b.cuda_stream, None, 0):
            with pytest.raises(capi.CloudMergeError) as e:
                cm.set_stream(handle)
            assert e.value.status == capi.BAD_ARG and REFUSED in str(e.value)
        assert cm.wait().status == capi.OK and b.query()
        cm.submit_all(rg.scene_ref(44).clouds)
        assert cm.merge_voxelize_async(capi.make_params(bl.PARAMS)) == capi.OK
        idle = b.query()
        assert cm.wait().status == capi.OK
        assert idle, "a refused cm_set_stream moved the context to the stream it named"
        with rg.BusyStream(a):
            rg.check_scene(cm, rg.scene_ref(44), "after the refused calls, still on A")


def device_clouds(hip, ref):
    """One device buffer per sensor holding ref's clouds (at least 16 bytes each)."""
    ptrs = []
    for s in range(len(ref.clouds)):
        raw, p = ref.raw(s), C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(len(raw), 16)) == 0
        if len(raw):
            assert hip.hipMemcpy(p, raw.ctypes.data, len(raw), 1) == 0
        ptrs.append(p)
    return ptrs


@pytest.mark.gpu
def test_device_clouds_ordered_by_the_stream_alone():
    """The device buffers hold scene 42's clouds. On the caller's stream, with no host synchronisation: a few milliseconds of
    matrix products, then the copies of scene 41's clouds (the same sizes) from pinned memory over them, then
    cm_submit_cloud_device for every sensor and the merge. A read that runs ahead of the copies sees scene 42's valid bytes."""
    torch = torch_cuda()
    hip = rg.hip()
    want, other = rg.scene_ref(41), rg.scene_ref(42)
    assert want.counts == other.counts and want.want["merged"] != other.want["merged"]
    stream = torch.cuda.Stream()
    pinned = rg.Pinned()
    ptrs = device_clouds(hip, other)
    try:
        staged = [pinned.of(want.raw(s)) for s in range(len(want.clouds))]
        with rg.scene_context() as cm:
            cm.set_stream(stream.cuda_stream)
            for s, c in enumerate(want.clouds):
                cm.set_transform(s, c.q_xyzw, c.t_xyz)
            keep = rg.backlog(torch, stream)
            for s, c in enumerate(want.clouds):
                if c.n:
                    assert hip.hipMemcpyAsync(ptrs[s], staged[s].ptr, c.n * c.point_step, 1, stream.cuda_stream) == 0
                cm.submit_device(s, ptrs[s].value, c.n, c.point_step, c.off_x, c.off_y, c.off_z, c.off_i)
            res = cm.merge_voxelize(bl.PARAMS)
            assert res.status == capi.OK
            rg.check_result(cm, res, want, cm.result(res.n_out), "device clouds")
            rg.check_scene(cm, want, "device clouds")
            del keep
    finally:
        stream.synchronize()
        for p in ptrs:
            hip.hipFree(p)
        pinned.free()


@pytest.mark.gpu
def test_device_sources_ordered_by_the_stream_alone():
    """cm_result_align_device and cm_result_ndt_align_device: the source buffer holds other points and is overwritten on the
    caller's stream just before the call. The correspondence tables are the restatements' for the points copied last."""
    torch = torch_cuda()
    hip = rg.hip()
    stream = torch.cuda.Stream()
    pinned = rg.Pinned()
    buf = C.c_void_p()
    n = 300
    assert hip.hipMalloc(C.byref(buf), 16 * n) == 0
    try:
        with rg.lattice_context() as cm:
            res, pts = bu.corner_frame(cm, 0)
            src, old = bu.sources(pts, n, seed=11), bu.sources(pts, n, seed=12)
            # the references, by the suites' checkers on the host entry points (one evaluation each)
            want_a = al.check_eval(cm, res, src, 0.75, al.GUESS, k=bu.K)[2]["corr"].tobytes()
            want_n = nd.check_eval(cm, res, src, bu.CORNER_LEAF, nd.GUESS)[2]["corr"].tobytes()
            assert want_a != al.check_eval(cm, res, old, 0.75, al.GUESS, k=bu.K)[2]["corr"].tobytes()
            assert want_n != nd.check_eval(cm, res, old, bu.CORNER_LEAF, nd.GUESS)[2]["corr"].tobytes()
            rec = {}
            for name, p in (("src", src), ("old", old)):
                r = np.zeros((n, 4), F32)
                r[:, :3] = p
                rec[name] = pinned.of(r.view(np.uint8).reshape(-1))
            cm.set_stream(stream.cuda_stream)
            for call in ("align", "ndt"):
                assert hip.hipMemcpy(buf, rec["old"].ptr, 16 * n, 1) == 0
                keep = rg.backlog(torch, stream)
                assert hip.hipMemcpyAsync(buf, rec["src"].ptr, 16 * n, 1, stream.cuda_stream) == 0
                if call == "align":
                    cm.align_device(buf.value, n, 0.75, guess=al.GUESS, max_iterations=0, normals_k=bu.K)
                    assert cm.align_correspondences(n).tobytes() == want_a, "the source was read before the copy on the stream"
                else:
                    cm.ndt_align_device(buf.value, n, guess=nd.GUESS, max_iterations=0)
                    assert cm.ndt_correspondences(n).tobytes() == want_n, "the source was read before the copy on the stream"
                del keep
    finally:
        stream.synchronize()
        hip.hipFree(buf)
        pinned.free()


# ---- regime 2: the published pipeline ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_published_pipeline_over_the_scenes():
    """Scenes 41, small, 42, small, 44 with step_out 16, 32, 16, 32, 16: both buffers of the pair carry a large result and then a
    small one, and the device-side wait on the older publish event is taken from the third frame on."""
    refs = [rg.scene_ref(k) for k in (41, "small", 42, "small", 44)]
    pinned = rg.Pinned()
    try:
        with rg.scene_context() as cm:
            rg.scene_pipeline(cm, refs, pinned, "pipeline")
    finally:
        pinned.free()


@pytest.mark.gpu
def test_the_published_pipeline_over_the_lattices():
    """The centroid by-products between publish_async and the next frame: lattices 0, 1, 2 and 1 again (one tile, two, one, two),
    then the turned shapes for the boxes."""
    pinned = rg.Pinned()
    try:
        with rg.lattice_context() as cm:
            rg.lattice_pipeline(cm, (0, 1, 2, 1, "shapes"), pinned, "pipeline")
    finally:
        pinned.free()


# ---- regime 3: four contexts on four threads ----------------------------------------------------------------------------------------
ROUNDS = 2


@pytest.mark.gpu
def test_four_contexts_on_four_threads():
    """ctypes drops the GIL for every call, so four threads keep four contexts busy in one process. Every thread's outputs are
    held to its own references, all computed before the threads start. Threads 0 and 1 use parameter sets in which every
    host-built table differs; after each round, behind a barrier that both have configured before, they run the producers once
    more with no configure call: a table shared between contexts is then wrong for one of them whatever the interleaving. Then
    both configure the cost and the matching layer 100 times at once with the largest tables, reading them back: a host-side table shared between
    contexts is built by both at the same moments."""
    test_the_second_parameter_set_changes_every_table()
    ref0, ref1 = rg.scene_ref(41, "a"), rg.scene_ref(42, "b")
    storms = [rg.storm_ref(ref0), rg.storm_ref(ref1)]
    assert storms[0]["cost_lut"] != storms[1]["cost_lut"] and storms[0]["match_lut"] != storms[1]["match_lut"]
    refs3 = [rg.scene_ref(k) for k in (44, "small", 47)]
    for r in refs3:
        assert r.oracle[0] == 0
    for step in range(3):
        rg.lattice_ref(step)
    rg.shapes_ref()
    bl.TAB()
    pinned = rg.Pinned()
    start, settled, storm = threading.Barrier(4), threading.Barrier(4), threading.Barrier(2)
    errors, where = {}, {}

    def scene_thread(k, ref):
        with rg.scene_context() as cm:
            start.wait(120)
            for r in range(ROUNDS):
                where[k] = f"round {r}: frame"
                rg.blocking_frame(cm, ref)
                where[k] = f"round {r}: collections"
                rg.check_scene(cm, ref, f"thread {k}, round {r}")
                settled.wait(120)
                where[k] = f"round {r}: producers with no configure call"
                rg.check_settled(cm, ref, f"thread {k}, round {r}")
                storm.wait(120)
                where[k] = f"round {r}: the tables configured over and over"
                rg.table_storm(cm, storms[k], f"thread {k}, round {r}")

    def lattice_thread(k):
        with rg.lattice_context() as cm:
            start.wait(120)
            for r in range(ROUNDS):
                for step in range(3):
                    where[k] = f"round {r}: lattice {step}"
                    res, _ = bu.lattice_frame(cm, step)
                    rg.check_lattice(cm, res, step, f"thread {k}, round {r}, lattice {step}")
                where[k] = f"round {r}: shapes"
                rg.check_shapes(cm, rg.shapes_frame(cm), f"thread {k}, round {r}, shapes")
                settled.wait(120)

    def pipeline_thread(k):
        with rg.scene_context() as cm:
            start.wait(120)
            for r in range(ROUNDS):
                where[k] = f"round {r}: pipeline"
                rg.scene_pipeline(cm, refs3, pinned, f"thread {k}, round {r}", first_step=16 if r == 0 else 32)
                settled.wait(120)

    def guarded(k, f, *a):
        def run():
            try:
                f(k, *a)
            except BaseException as e:                       # kept and raised again below, with the thread and the step
                errors[k] = e
                for b in (start, settled, storm):
                    b.abort()
        return threading.Thread(target=run, daemon=True, name=f"regime-{k}")

    threads = [guarded(0, scene_thread, ref0), guarded(1, scene_thread, ref1), guarded(2, lattice_thread), guarded(3, pipeline_thread)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)                                      # a hang guard, not a measurement
        alive = [t.name for t in threads if t.is_alive()]
        assert not alive, f"still running after 120 s: {alive} at {where}"
        first = [k for k in sorted(errors) if not isinstance(errors[k], threading.BrokenBarrierError)] or sorted(errors)
        if first:
            k = first[0]
            raise AssertionError(f"thread {k} at {where.get(k)}: {type(errors[k]).__name__}: {errors[k]}") from errors[k]
    finally:
        if not any(t.is_alive() for t in threads):
            pinned.free()
