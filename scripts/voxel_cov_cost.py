#!/usr/bin/env python3
"""Cost of the per-voxel covariance table (cm_result_voxel_cov_device / cm_result_voxel_cov) on the cfg2 shape: 4 x 1 M
points, random SE(3) per sensor, clouds resident in HBM (cm_submit_cloud_device, like bench.py), min 2 points per voxel,
at 5 cm and 50 cm voxels. For every leaf: the frame alone, the device table after it (wall clock of the call, which
synchronises), the host call (the table again, then its copy), and the table's size. Prints one JSON line (also written to --out).

  python scripts/voxel_cov_cost.py --frames 30 --out profiles/voxel_cov_cost_cfg2.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/voxel_cov_cost.py --frames 10      # the kernels from the trace
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
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
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

    out = {"shape": f"4 x {a.n} pts, 16-B records, min 2 points per voxel", "frames": a.frames}
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        for leaf in (0.05, 0.5):
            params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
            frame, table, copy = [], [], []
            host = None
            for f in range(a.warmup + a.frames):
                t0 = time.perf_counter()
                for k, s in enumerate(sensors):
                    cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
                res = cm.merge_voxelize(params)
                t1 = time.perf_counter()
                assert res.status == capi.OK
                _, n = cm.voxel_covariance_device()
                t2 = time.perf_counter()
                host = cm.voxel_covariance(res.n_out)
                t3 = time.perf_counter()
                assert n == res.n_out
                if f >= a.warmup:
                    frame.append(t1 - t0); table.append(t2 - t1); copy.append(t3 - t2)
            flags = host["flags"]
            key = f"leaf_{leaf:g}"
            out[key] = {
                "n_merged": int(res.n_merged), "n_out": int(res.n_out), "path_flags": int(res.path_flags),
                "frame_ms": round(float(np.median(frame)) * 1e3, 4),
                "table_device_ms": round(float(np.median(table)) * 1e3, 4),
                "table_host_ms": round(float(np.median(copy)) * 1e3, 4),
                "table_mb": round(res.n_out * 80 / 2 ** 20, 2),
                "valid": int(((flags & capi.COV_VALID) != 0).sum()),
                "inflated": int(((flags & capi.COV_INFLATED) != 0).sum()),
                "max_points_per_voxel": int(host["count"].max()),
            }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
