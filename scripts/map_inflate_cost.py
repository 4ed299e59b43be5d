#!/usr/bin/env python3
"""Cost of the cost layer over the occupancy map (cm_map_cost_update) on the cfg2 shape: 4 x 1 M points, random SE(3) per
sensor, clouds resident in HBM (cm_submit_cloud_device, like bench.py), 5 cm voxels, min 2 points per voxel, a window of
1000 x 1000 cells of 10 cm, the pose moving 0.37 m per frame, radii 0.35 / 1.05 m, scaling 3. One job measures, in this order:
  - the frame on a context with no layer configured (medians of --batches batches of --frames frames, and their spread): the
    parent's frame, since no kernel of cm_merge_voxelize is touched;
  - the frame on a context with a map, every frame integrated behind it (the integrate call timed on its own, wall clock of the
    call, which synchronises): the yardstick for an update is this integrate call;
  - the frame on a context with map and layer, integrate and update behind every frame, each call timed on its own;
  - the first series again, to show the drift of the job;
  - the per-stage times of one update and one integrate call under CM_FLAG_PROFILE (a context of its own);
  - R = 256 (an inflation radius of 25.6 m), once: medians of one batch of updates of the same image;
  - the 2048 x 2048 window with a single obstacle in one corner, once: the worst case of the row pass's outward scan.
Prints one JSON line (also appended to --out).

  python scripts/map_inflate_cost.py --out profiles/map_inflate_cost.txt
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
    from cloud_merger_amd.types import MergeParams, xyzi_cloud

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    radii = (0.35, 1.05, 3.0)

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

    def batches(cm, after=()):
        """Medians of the frame per batch, and of every call of `after` ((name, fn) pairs, run behind every frame in order and
        timed on their own)."""
        for _ in range(a.warmup):
            frame(cm)
            for _, fn in after:
                fn()
        meds, extra = [], {name: [] for name, _ in after}
        for _ in range(a.batches):
            t, u = [], {name: [] for name, _ in after}
            for _ in range(a.frames):
                t.append(frame(cm))
                for name, fn in after:
                    u[name].append(timed(fn))
            meds.append(ms(t))
            for name in u:
                extra[name].append(ms(u[name]))
        rec = {"frame_ms_batches": meds, "frame_ms": round(float(np.median(meds)), 4), "frame_ms_spread": round(max(meds) - min(meds), 4)}
        for name, v in extra.items():
            rec.update({f"{name}_ms_batches": v, f"{name}_ms": round(float(np.median(v)), 4), f"{name}_ms_spread": round(max(v) - min(v), 4)})
        return rec

    def integrator(cm):
        n = [0]

        def integrate():
            n[0] += 1
            cm.map_integrate(pose(n[0]))
        return integrate

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; window {a.size} x {a.size} cells of "
                                      f"{a.cell} m; radii {radii[0]} / {radii[1]} m, scaling {radii[2]}", "frames": a.frames, "batches": a.batches}
    with context() as cm:
        out["no_layer"] = batches(cm)
    with context() as cm:
        cm.map_configure(a.cell, a.size, a.size)
        out["map_only"] = batches(cm, [("integrate", integrator(cm))])
    with context() as cm:
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        out["map_and_layer"] = batches(cm, [("integrate", integrator(cm)), ("update", cm.map_cost_update)])
        image, info = cm.map_occupancy()
        cost, dist2, _ = cm.map_cost()
        real = dist2[dist2 != capi.MAP_DIST_NONE]
        out["map_and_layer"].update(n_frames=int(info.n_frames), occupied_cells=int((image == 100).sum()), free_cells=int((image == 0).sum()),
                                    inflated_cells=int(((cost > 0) & (cost < 253)).sum()), largest_dist2=int(real.max()) if len(real) else None,
                                    median_dist2=float(np.median(real)) if len(real) else None)
        # R = 256 over the same image, once
        cm.map_cost_configure(0.35, 25.6, 0.25)
        cm.map_cost_update()
        out["r256_update_ms"] = ms([timed(cm.map_cost_update) for _ in range(a.frames)])
        out["r256_table_entries"] = int(len(cm.map_cost_table()))
    with context() as cm:
        out["no_layer_again"] = batches(cm)
    with context(capi.FLAG_PROFILE) as cm:
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        stages = []
        for k in range(8):
            frame(cm)
            cm.map_integrate(pose(k))
            if k == 7:
                out["profile_map_integrate"] = [(n, round(t, 4)) for n, t in cm.stage_times()]
            cm.map_cost_update()
            stages.append(cm.stage_times())
        out["profile_cost_update"] = [(n, round(float(np.median([s[j][1] for s in stages[3:]])), 4)) for j, (n, _) in enumerate(stages[-1])]
    # the worst case of the outward scan: 2048 x 2048, one obstacle in a corner (a frame of one point, the sensor outside)
    with capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
        n, cell = 2048, 0.02
        cm.map_configure(cell, n, n)
        cm.map_cost_configure(0.1, 0.5, 2.0)
        t = (100.0, 0.0, 0.0)
        p = np.array([[(-(n // 2) + n - 1 + 0.5) * cell - t[0], (-(n // 2) + 0.5) * cell, 0.0]], np.float32)
        cm.submit_all([xyzi_cloud(p, np.zeros(1, np.float32), t_xyz=t)])
        assert cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)).status == capi.OK
        cm.map_integrate(None)
        cm.map_cost_update()
        image, _ = cm.map_occupancy()
        assert int((image == 100).sum()) == 1 and image[0, n - 1] == 100
        out["corner_2048_update_ms"] = ms([timed(cm.map_cost_update) for _ in range(10)])
        out["corner_2048_profile"] = [(n_, round(t_, 4)) for n_, t_ in cm.stage_times()]
        out["corner_2048_largest_dist2"] = int(cm.map_cost()[1].max())
    out["update_ms_over_integrate_ms"] = round(out["map_and_layer"]["update_ms"] / out["map_and_layer"]["integrate_ms"], 4)
    for k in ("map_only", "map_and_layer"):
        out[f"frame_ms_{k}_minus_no_layer"] = round(out[k]["frame_ms"] - out["no_layer"]["frame_ms"], 4)
    out["largest_batch_spread_ms"] = max(out[k]["frame_ms_spread"] for k in ("no_layer", "map_only", "map_and_layer", "no_layer_again"))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
