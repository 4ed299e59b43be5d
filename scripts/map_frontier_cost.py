#!/usr/bin/env python3
"""Cost of the frontier layer behind the plan layer (cm_map_frontier_update). One job measures, in this order:
  - cfg2's frame (4 x 1 M points, random SE(3) per sensor, clouds resident in HBM, 5 cm voxels, min 2 points per voxel) on a
    context with no layer configured (medians of --batches batches of --frames frames, and their spread): the parent's frame,
    since no kernel of cm_merge_voxelize is touched;
  - the same frame on a context with map, cost layer, plan layer and frontier layer configured and never updated;
  - the first series again, to show the drift of the job;
  - for windows of 257 x 255, 1000 x 1000 and 2048 x 2048 cells of 10 cm, a scene with rays: 16 sensors inside the window, each
    with --rays returns scattered around it, integrated once (free rays through an unknown field, the returns occupied). On
    that map cm_map_cost_update (the yardstick: like the frontier update a handful of passes over a few bytes per cell),
    cm_map_plan_update with the goal at the window's centre (weights 1 / 0 with unknown cells allowed, which the range rule
    admits at every size) and cm_map_frontier_update, each the wall clock of the call, which synchronises: --warmup calls, then
    the median and the spread of --reps calls; the info of the frontier update; and the per-stage times of one update of each
    under CM_FLAG_PROFILE (a context of its own, medians over the calls).
Prints one JSON line (also appended to --out).

  python scripts/map_frontier_cost.py --out profiles/map_frontier_cost.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = ((257, 255), (1000, 1000), (2048, 2048))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--rays", type=int, default=200, help="returns per sensor of the scene with rays")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams, xyzi_cloud

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    radii = (0.35, 1.05, 3.0)
    plan = (1, 0, True)
    front = (4, 4096, 252, 1, 1)

    def context():
        cm = capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY)
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

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def batches(cm):
        for _ in range(a.warmup):
            frame(cm)
        meds = [ms([frame(cm) for _ in range(a.frames)]) for _ in range(a.batches)]
        return {"frame_ms_batches": meds, "frame_ms": round(float(np.median(meds)), 4), "frame_ms_spread": round(max(meds) - min(meds), 4)}

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; windows of {a.cell} m cells; radii "
                                      f"{radii[0]} / {radii[1]} m, scaling {radii[2]}; plan {plan[0]} / {plan[1]}, unknown allowed; frontiers "
                                      f"min_cells {front[0]}, max_frontiers {front[1]}", "frames": a.frames, "batches": a.batches, "reps": a.reps}
    with context() as cm:
        out["no_layer"] = batches(cm)
    with context() as cm:
        cm.map_configure(a.cell, 1000, 1000)
        cm.map_cost_configure(*radii)
        cm.map_plan_configure(*plan)
        cm.map_frontier_configure(*front)
        out["configured_not_updated"] = batches(cm)
    with context() as cm:
        out["no_layer_again"] = batches(cm)

    def rays(nx, ny, flags=0):
        """A context whose map of nx x ny cells holds one frame of 16 sensors inside the window with a.rays returns each."""
        cm = capi.CloudMerger(max_points_total=16 * a.rays + 4096, max_sensors=16, flags=flags)
        cm.map_configure(a.cell, nx, ny)
        rng = np.random.default_rng(nx * 7 + ny)
        r = min(nx, ny) / 5.0
        frames = []
        for k in range(16):
            o = np.array([(k % 4 + 0.5) * nx / 4 - nx // 2, (k // 4 + 0.5) * ny / 4 - ny // 2]) * a.cell
            ang, rad = rng.uniform(0, 2 * np.pi, a.rays), rng.uniform(0.3 * r, r, a.rays) * a.cell
            p = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(a.rays)], axis=1)
            frames.append(xyzi_cloud(p.astype(np.float32), np.zeros(a.rays, np.float32), t_xyz=(float(o[0]), float(o[1]), 0.0)))
        cm.submit_all(frames)
        assert cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)).status == capi.OK
        cm.map_integrate(None)
        cm.map_cost_configure(*radii)
        cm.map_plan_configure(*plan)
        cm.map_frontier_configure(*front)
        return cm

    def series(fn):
        for _ in range(a.warmup):
            fn()
        t = [timed(fn) * 1e3 for _ in range(a.reps)]
        return {"ms": round(float(np.median(t)), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}

    out["windows"] = []
    for nx, ny in WINDOWS:
        goal = (0.5 * a.cell, 0.5 * a.cell)
        rec = {"window": [nx, ny]}
        with rays(nx, ny) as cm:
            image = cm.map_occupancy()[0]
            rec["image"] = {"unknown": int((image == -1).sum()), "free": int((image == 0).sum()), "occupied": int((image == 100).sum())}
            rec["cost_update"] = series(cm.map_cost_update)
            sweeps = []
            rec["plan_update"] = series(lambda: sweeps.append(int(cm.map_plan_update(*goal).n_sweeps)))
            rec["plan_sweeps"] = sweeps[-1]
            rec["frontier_update"] = series(cm.map_frontier_update)
            i = cm.map_frontier_update()
            rec["frontier_info"] = {"n_frontier_cells": i.n_frontier_cells, "n_components": i.n_components, "n_frontiers": i.n_frontiers,
                                    "n_written": i.n_written, "best": i.best, "best_score": i.best_score}
            rec["frontier_ms_over_cost_update_ms"] = round(rec["frontier_update"]["ms"] / rec["cost_update"]["ms"], 4)
        with rays(nx, ny, capi.FLAG_PROFILE) as cm:
            prof = {"cost_update": [], "plan_update": [], "frontier_update": []}
            for _ in range(a.warmup + 8):
                cm.map_cost_update()
                prof["cost_update"].append(cm.stage_times())
                cm.map_plan_update(*goal)
                prof["plan_update"].append(cm.stage_times())
                cm.map_frontier_update()
                prof["frontier_update"].append(cm.stage_times())
            for name, runs in prof.items():
                rec[f"profile_{name}"] = [(n, round(float(np.median([s[j][1] for s in runs[a.warmup:]])), 4)) for j, (n, _) in enumerate(runs[-1])]
        out["windows"].append(rec)
    out["frame_ms_configured_minus_no_layer"] = round(out["configured_not_updated"]["frame_ms"] - out["no_layer"]["frame_ms"], 4)
    out["largest_batch_spread_ms"] = max(out[k]["frame_ms_spread"] for k in ("no_layer", "configured_not_updated", "no_layer_again"))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
