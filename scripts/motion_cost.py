#!/usr/bin/env python3
"""Cost of ego-motion compensation on the cfg2 shape: 4 x 1 M points in 20-byte records (x, y, z, intensity, time f32 @16),
random SE(3) per sensor, 5 cm voxels, clouds resident in HBM (cm_submit_cloud_device, like bench.py). Times the frame with
compensation off and on (wall clock over back-to-back synchronous frames, and k_motion's own time from a CM_FLAG_PROFILE
context), and prints one JSON line (also written to --out).

  python scripts/motion_cost.py --frames 50 --out profiles/motion_cost.json
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/motion_cost.py --frames 20      # k_motion from the trace
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
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth

    sensors, params = synth.config2(n_per_sensor=a.n, min_pts=0)
    dev = torch.device("cuda", 0)
    clouds = []
    for s in sensors:
        rec = np.zeros((s.n, 20), np.uint8)
        rec[:, :16] = np.ascontiguousarray(s.data).view(np.uint8).reshape(s.n, 16)
        rec[:, 16:20] = np.linspace(0.0, 0.1, s.n, dtype=np.float32).view(np.uint8).reshape(s.n, 4)
        clouds.append(torch.from_numpy(rec.reshape(-1)).to(dev))
    torch.cuda.synchronize()
    t_ref = 1_700_000_000_000_000_000
    motion = capi.make_motion((15.0, 0.5, 0.0), (0.02, 0.01, 0.5), t_ref, [t_ref - 10_000_000 * k for k in range(4)])

    def frames(cm, n, on):
        cm.set_ego_motion(motion if on else None)
        times = []
        for f in range(n):
            t0 = time.perf_counter()
            for k, s in enumerate(sensors):
                cm.submit_device(k, clouds[k].data_ptr(), s.n, 20, 0, 4, 8, 12)
            res = cm.merge_voxelize(params)
            times.append(time.perf_counter() - t0)
            assert res.status == capi.OK and bool(res.path_flags & capi.PATH_MOTION) == on
        return times

    out = {"shape": f"4 x {a.n} pts, 20-B records (time f32 @16), 5 cm", "frames": a.frames}
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4) as cm:
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
            cm.set_time_field(k, 16, capi.TIME_F32_S)
        for on in (False, True, False, True):        # interleaved, warm-up frames dropped each time
            t = frames(cm, a.warmup + a.frames, on)[a.warmup:]
            key = "frame_ms_motion_on" if on else "frame_ms_motion_off"
            out.setdefault(key, []).append(round(float(np.median(t)) * 1e3, 4))
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_PROFILE) as cm:
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
            cm.set_time_field(k, 16, capi.TIME_F32_S)
        for on in (False, True):
            stage = {}
            dev_ms = []
            cm.set_ego_motion(motion if on else None)
            for f in range(a.warmup + a.frames):
                for k, s in enumerate(sensors):
                    cm.submit_device(k, clouds[k].data_ptr(), s.n, 20, 0, 4, 8, 12)
                res = cm.merge_voxelize(params)
                if f >= a.warmup:
                    dev_ms.append(res.device_ms)
                    for name, ms in cm.stage_times():
                        stage.setdefault(name, []).append(ms)
            key = "on" if on else "off"
            out[f"device_ms_{key}"] = round(float(np.median(dev_ms)), 4)
            out[f"stages_ms_{key}"] = {n: round(float(np.median(v)), 4) for n, v in stage.items()}
    out["k_motion_us_event"] = round(out["stages_ms_on"].get("k_motion", float("nan")) * 1e3, 1)
    out["frame_cost_ms"] = round(min(out["frame_ms_motion_on"]) - min(out["frame_ms_motion_off"]), 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
