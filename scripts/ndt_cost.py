#!/usr/bin/env python3
"""Cost of the NDT registration (cm_result_ndt_align_device) on the cfg2 shape, beside the ICP call's (scripts/align_cost.py's
protocol): 4 x 1 M points, random SE(3) per sensor, clouds resident in HBM, min 2 points per voxel, at 5 cm and 50 cm voxels,
neighbourhood 7, the covariance table at {3, 0.01}. The frames alternate between the sensors' poses and the same poses
shifted by (0.3, -0.2, 0.1) leaf, so that the previous result — kept in HBM, the source of every call — differs from the
current one. For every leaf: the frame with the call never made (medians of --batches batches of --frames frames, and their
spread); the covariance call alone; the NDT call with the table held at max_iterations 0 (one evaluation) and at 30 (with the
iterations it took); the per-iteration time from the two; the first call after a frame, which computes the table itself; the
ICP call (r = 4 leaf, k = 10, normals held) on the same frames; and the per-name stage times of one NDT call under
CM_FLAG_PROFILE (a context of its own): k_ndt_eval, k_aln_sum and the readback separately. Prints one JSON line (also written
to --out).

  python scripts/ndt_cost.py --out profiles/ndt_cost_cfg2.json
  python scripts/ndt_cost.py --frame-only      # only the frame: runs on a tree without the feature, for comparison
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COV = dict(cov_min_points=3, cov_eig_mult=0.01)


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
            pose(cm, leaf, False)
            for _ in range(a.warmup):
                frame(cm, params)
            meds = [ms([frame(cm, params)[1] for _ in range(a.frames)]) for _ in range(a.batches)]
            res, _ = frame(cm, params)
            rec = dict(n_merged=int(res.n_merged), n_out=int(res.n_out), path_flags=int(res.path_flags), frame_ms_batches=meds,
                       frame_ms=round(float(np.median(meds)), 4), frame_ms_spread=round(max(meds) - min(meds), 4))
            if not a.frame_only:
                names = ("cold", "cov", "eval", "full", "icp_eval", "icp_full", "frame")
                t = {k: [] for k in names}
                its, icp_its, last, icp, n_last = [], [], None, None, 0
                prev, n_prev = keep(cm, res)
                for f in range(a.warmup + a.frames):
                    pose(cm, leaf, f % 2 == 0)
                    res, t_frame = frame(cm, params)
                    ts = [time.perf_counter()]
                    cold = cm.ndt_align_device(prev.data_ptr(), n_prev, max_iterations=30, **COV)   # computes the table itself
                    ts.append(time.perf_counter())
                    cm.voxel_covariance_device(3, 0.01)
                    ts.append(time.perf_counter())
                    cm.ndt_align_device(prev.data_ptr(), n_prev, max_iterations=0, **COV)
                    ts.append(time.perf_counter())
                    last = cm.ndt_align_device(prev.data_ptr(), n_prev, max_iterations=30, **COV)
                    ts.append(time.perf_counter())
                    assert bytes(memoryview(cold)) == bytes(memoryview(last))
                    cm.normals_device(10)
                    ts.append(time.perf_counter())
                    cm.align_device(prev.data_ptr(), n_prev, 4 * leaf, max_iterations=0, normals_k=10)
                    ts.append(time.perf_counter())
                    icp = cm.align_device(prev.data_ptr(), n_prev, 4 * leaf, max_iterations=30, normals_k=10)
                    ts.append(time.perf_counter())
                    if f >= a.warmup:
                        d = np.diff(ts)
                        for k, v in zip(names, (d[0], d[1], d[2], d[3], d[5], d[6], t_frame)):
                            t[k].append(v)
                        its.append(last.iterations)
                        icp_its.append(icp.iterations)
                    n_last = n_prev                              # the source of `last` and `icp`, before it is replaced
                    prev, n_prev = keep(cm, res)
                evals, icp_evals = float(np.median(its)) + 1, float(np.median(icp_its)) + 1
                rec.update(n_src=n_last, iterations=its[-1], flags=int(last.flags), n_corr=int(last.n_corr), score=last.score,
                           translation=[round(last.pose[k], 6) for k in (3, 7, 11)],
                           ndt_call_ms=ms(t["full"]), ndt_eval_only_ms=ms(t["eval"]), cov_ms=ms(t["cov"]),
                           ndt_first_call_ms=ms(t["cold"]), frame_ms_between_calls=ms(t["frame"]),
                           ndt_per_iteration_ms=round((ms(t["full"]) - ms(t["eval"])) / max(evals - 1, 1), 4),
                           icp=dict(r=4 * leaf, iterations=icp_its[-1], flags=int(icp.flags), n_corr=int(icp.n_corr),
                                    translation=[round(icp.pose[k], 6) for k in (3, 7, 11)],
                                    call_ms=ms(t["icp_full"]), eval_only_ms=ms(t["icp_eval"]),
                                    per_iteration_ms=round((ms(t["icp_full"]) - ms(t["icp_eval"])) / max(icp_evals - 1, 1), 4)))
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
                    cm.voxel_covariance_device(3, 0.01)
                    got = cm.ndt_align_device(prev.data_ptr(), n_prev, max_iterations=30, **COV)
                    st = cm.stage_times()
                    pose(cm, leaf, False)
                    res, _ = frame(cm, params)
                    prev, n_prev = keep(cm, res)
                ev = got.iterations + 1
                out[f"leaf_{leaf:g}"]["stages"] = dict(evaluations=ev, call_ms=round(sum(v for _, v in st), 4),
                                                      stages_ms=[(n, round(v, 4)) for n, v in st],
                                                      per_evaluation_ms={n: round(v / ev, 4) for n, v in st if n != "k_cl_bounds"})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
