#!/usr/bin/env python3
"""Cost of the registration (cm_result_align_device) on the cfg2 shape: 4 x 1 M points, random SE(3) per sensor, clouds
resident in HBM (cm_submit_cloud_device, like bench.py), min 2 points per voxel, at 5 cm and 50 cm voxels, k = 10, r = 4 leaf.
The frames alternate between the sensors' poses and the same poses shifted by (0.3, -0.2, 0.1) leaf, so that the previous
result — kept in HBM, the source of every call — differs from the current one. For every leaf: the frame with the call never
made (medians of --batches batches of --frames frames, and their spread); the normals call alone; the call with the table held
at max_iterations 0 (front end + one evaluation) and at 30 (with the iterations it took); the per-iteration time from the
two; the first call after a frame, which computes the table itself; and the per-name stage times of one call under
CM_FLAG_PROFILE (a context of its own) with the front end's share. Prints one JSON line (also written to --out).

  python scripts/align_cost.py --out profiles/align_cost_cfg2.json
  python scripts/align_cost.py --frame-only      # only the frame: runs on a tree without the feature, for comparison
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LOOP = ("k_aln_eval", "k_aln_sum", "aln_readback")        # the stages of an evaluation; everything else is the front end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()

    def pose(cm, leaf, moved):
        d = np.array([0.3, -0.2, 0.1]) * leaf if moved else np.zeros(3)
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, tuple(np.asarray(s.t_xyz, float) + d))

    def frame(cm, params):
        t0 = time.perf_counter()
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        res = cm.merge_voxelize(params)
        assert res.status == capi.OK
        return res, time.perf_counter() - t0

    def keep(cm, res):
        """The result as a tensor in HBM: the next frame's source."""
        rec = cm.result(res.n_out)
        return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1)).to(dev), int(res.n_out)

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)
    out = {"shape": f"4 x {a.n} pts, 16-B records, min 2 points per voxel", "frames": a.frames, "batches": a.batches}
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for leaf in (0.05, 0.5):
            params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
            r, kw = 4 * leaf, dict(normals_k=10, trans_eps=1e-6, rot_eps=1e-6)
            pose(cm, leaf, False)
            for _ in range(a.warmup):
                frame(cm, params)
            meds = [ms([frame(cm, params)[1] for _ in range(a.frames)]) for _ in range(a.batches)]
            res, _ = frame(cm, params)
            rec = dict(n_merged=int(res.n_merged), n_out=int(res.n_out), path_flags=int(res.path_flags), frame_ms_batches=meds,
                       frame_ms=round(float(np.median(meds)), 4), frame_ms_spread=round(max(meds) - min(meds), 4))
            if not a.frame_only:
                t = {k: [] for k in ("normals", "eval", "full", "cold", "frame")}
                its, last = [], None
                prev, n_prev = keep(cm, res)
                for f in range(a.warmup + a.frames):
                    pose(cm, leaf, f % 2 == 0)
                    res, t_frame = frame(cm, params)
                    t0 = time.perf_counter()
                    cold = cm.align_device(prev.data_ptr(), n_prev, r, max_iterations=30, **kw)    # computes the table itself
                    t1 = time.perf_counter()
                    cm.normals_device(10)
                    t2 = time.perf_counter()
                    cm.align_device(prev.data_ptr(), n_prev, r, max_iterations=0, **kw)
                    t3 = time.perf_counter()
                    last = cm.align_device(prev.data_ptr(), n_prev, r, max_iterations=30, **kw)
                    t4 = time.perf_counter()
                    assert bytes(memoryview(cold)) == bytes(memoryview(last))
                    if f >= a.warmup:
                        for k, v in zip(("cold", "normals", "eval", "full", "frame"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t_frame)):
                            t[k].append(v)
                        its.append(last.iterations)
                    prev, n_prev = keep(cm, res)
                evals = float(np.median(its)) + 1
                rec.update(r=r, n_src=n_prev, iterations=its[-1], flags=int(last.flags), n_corr=int(last.n_corr), rms=last.rms,
                           translation=[round(last.pose[k], 6) for k in (3, 7, 11)],
                           align_call_ms=ms(t["full"]), align_eval_only_ms=ms(t["eval"]), normals_ms=ms(t["normals"]),
                           align_first_call_ms=ms(t["cold"]), frame_ms_between_calls=ms(t["frame"]),
                           per_iteration_ms=round((ms(t["full"]) - ms(t["eval"])) / max(evals - 1, 1), 4),
                           normals_share_of_first_call=round(ms(t["normals"]) / ms(t["cold"]), 4))
            out[f"leaf_{leaf:g}"] = rec
    if not a.frame_only:
        with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
            for leaf in (0.05, 0.5):
                params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
                pose(cm, leaf, False)
                res, _ = frame(cm, params)
                prev, n_prev = keep(cm, res)
                for _ in range(3):
                    pose(cm, leaf, True)
                    res, _ = frame(cm, params)
                    cm.normals_device(10)
                    got = cm.align_device(prev.data_ptr(), n_prev, 4 * leaf, max_iterations=30, normals_k=10)
                    st = cm.stage_times()
                    pose(cm, leaf, False)
                    res, _ = frame(cm, params)
                    prev, n_prev = keep(cm, res)
                total = sum(v for _, v in st)
                front = sum(v for n, v in st if n not in LOOP)
                out[f"leaf_{leaf:g}"]["stages"] = dict(evaluations=got.iterations + 1, call_ms=round(total, 4),
                                                      front_end_ms=round(front, 4), front_end_share=round(front / total, 4),
                                                      stages_ms=[(n, round(v, 4)) for n, v in st])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
