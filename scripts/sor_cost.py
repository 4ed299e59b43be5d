#!/usr/bin/env python3
"""Cost of statistical outlier removal (cm_set_statistical_outlier) on the cfg2 shape: 4 x 1 M points, random SE(3) per
sensor, clouds resident in HBM (cm_submit_cloud_device, like bench.py), 5 cm voxels, min 2 points per voxel. For mean_k
10 / 30 / 50, with and without a crop box: the frame alone with the stage on and with it off, and the per-stage times
(CM_FLAG_PROFILE). CM_VERBOSE=1 in the environment prints, per frame, how many points the second search launch took.
Prints one JSON line (also written to --out).

  python scripts/sor_cost.py --frames 20 --out profiles/sor_cost_cfg2.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/sor_cost.py --frames 5      # the kernels from the trace
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--ks", default="10,30,50")
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

    out = {"shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel", "frames": a.frames}
    crops = {"nocrop": {}, "crop": dict(crop_min=(-12.0, -12.0, -3.0), crop_max=(12.0, 12.0, 3.0))}
    for flags, tag in ((0, "wall"), (capi.FLAG_PROFILE, "stages")):
        with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=flags) as cm:
            for k, s in enumerate(sensors):
                cm.set_transform(k, s.q_xyzw, s.t_xyz)

            def frame(params):
                t0 = time.perf_counter()
                for k, s in enumerate(sensors):
                    cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
                res = cm.merge_voxelize(params)
                assert res.status == capi.OK
                return time.perf_counter() - t0, res

            for cname, crop in crops.items():
                params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2, **crop)
                for mk in [0] + [int(v) for v in a.ks.split(",")]:
                    cm.set_statistical_outlier(mk if mk else None, 1.0)
                    ts = []
                    for f in range(a.warmup + a.frames):
                        dt, res = frame(params)
                        if f >= a.warmup:
                            ts.append(dt)
                    key = f"{cname}_k{mk}" if mk else f"{cname}_off"
                    e = out.setdefault(key, {})
                    if tag == "wall":
                        e["frame_ms"] = round(float(np.median(ts)) * 1e3, 4)
                        e["path_flags"] = int(res.path_flags)
                        e["n_merged"] = int(res.n_merged)
                        if mk:
                            st = cm.sor_stats()
                            e.update(n_valid=int(st.n_valid), n_removed=int(st.n_removed), mean=st.mean, stddev=st.stddev,
                                     threshold=st.threshold)
                    else:
                        e["stages_ms"] = {n: round(ms, 4) for n, ms in cm.stage_times() if "sor" in n}
                        e["device_ms"] = round(float(res.device_ms), 4)
            cm.set_statistical_outlier(None)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
