#!/usr/bin/env python3
"""Cost of the rolling occupancy map (cm_map_integrate) on the cfg2 shape: 4 x 1 M points, random SE(3) per sensor, clouds
resident in HBM (cm_submit_cloud_device, like bench.py), 5 cm voxels, min 2 points per voxel, a window of 1000 x 1000 cells
of 10 cm. One job measures, in this order:
  - the frame on a context with no map configured (medians of --batches batches of --frames frames, and their spread): the
    baseline, which is the parent's frame, since no kernel of cm_merge_voxelize is touched;
  - the frame on a context with a map configured and no frame integrated (the same batches);
  - the frame on a context with a map configured, every frame integrated behind it under a pose that moves 0.37 m per frame
    (the same batches; the integrate call is timed on its own, wall clock of the call, which synchronises);
  - the baseline again, to show the drift of the job;
  - cm_result_grid_rays_device on the same frames over the 1000 x 1000 grid that covers the first window (the yardstick: the
    same mark and cast over a grid that does not move, plus the grid map);
  - the per-stage times of one integrate call and one ray call under CM_FLAG_PROFILE (a context of its own).
Prints one JSON line (also appended to --out).

  python scripts/map_cost.py --out profiles/map_cost.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    half = a.cell * a.size / 2
    grid = ((-half, -half), a.cell, a.size, a.size)

    def context(flags=0):
        cm = capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY | flags)
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        return cm

    def frame(cm):
        t0 = time.perf_counter()
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        res = cm.merge_voxelize(params)
        assert res.status == capi.OK
        return time.perf_counter() - t0

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def pose(k):
        P = np.eye(3, 4, dtype=np.float32)
        P[0, 3], P[1, 3] = 0.37 * k, -0.11 * k
        return P

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def batches(cm, after=None):
        """Medians of the frame per batch (and of `after`, run behind every frame and timed on its own)."""
        for _ in range(a.warmup):
            frame(cm)
            if after:
                after()
        meds, extra = [], []
        for _ in range(a.batches):
            t, u = [], []
            for _ in range(a.frames):
                t.append(frame(cm))
                if after:
                    u.append(timed(after))
            meds.append(ms(t))
            if after:
                extra.append(ms(u))
        rec = {"frame_ms_batches": meds, "frame_ms": round(float(np.median(meds)), 4), "frame_ms_spread": round(max(meds) - min(meds), 4)}
        if after:
            rec.update(call_ms_batches=extra, call_ms=round(float(np.median(extra)), 4), call_ms_spread=round(max(extra) - min(extra), 4))
        return rec

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; window {a.size} x {a.size} cells of {a.cell} m",
           "frames": a.frames, "batches": a.batches}
    with context() as cm:
        out["no_map"] = batches(cm)
    with context() as cm:
        cm.map_configure(a.cell, a.size, a.size)
        out["map_configured"] = batches(cm)
    with context() as cm:
        cm.map_configure(a.cell, a.size, a.size)
        n = [0]

        def integrate():
            n[0] += 1
            cm.map_integrate(pose(n[0]))
        out["with_map"] = batches(cm, integrate)
        table, info = cm.map()
        out["with_map"].update(n_frames=int(info.n_frames), observed_cells=int((table["n_obs"] > 0).sum()),
                               anchor=[int(info.anchor[0]), int(info.anchor[1])])
    with context() as cm:
        out["no_map_again"] = batches(cm)
    with context() as cm:
        out["grid_rays_device"] = batches(cm, lambda: cm.grid_rays_device(*grid))
    with context(capi.FLAG_PROFILE) as cm:
        cm.map_configure(a.cell, a.size, a.size)
        for k in range(3):
            frame(cm)
            cm.map_integrate(pose(k))
        out["profile_map_integrate"] = [(n, round(t, 4)) for n, t in cm.stage_times()]
        for k in range(3):
            frame(cm)
            cm.grid_rays_device(*grid)
        out["profile_grid_rays"] = [(n, round(t, 4)) for n, t in cm.stage_times()]
    for k in ("map_configured", "with_map", "grid_rays_device"):
        out[f"frame_ms_{k}_minus_no_map"] = round(out[k]["frame_ms"] - out["no_map"]["frame_ms"], 4)
    out["largest_batch_spread_ms"] = max(out[k]["frame_ms_spread"] for k in ("no_map", "map_configured", "with_map", "no_map_again"))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
