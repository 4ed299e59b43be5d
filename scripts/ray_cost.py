#!/usr/bin/env python3
"""Cost of the free-space ray casting (cm_result_grid_rays_device) on the cfg2 shape: 4 x 1 M points, random SE(3) per sensor,
clouds resident in HBM (cm_submit_cloud_device, like bench.py), 5 cm voxels, min 2 points per voxel, a crop box of +-25 m so that
the frames after the first take the quantile pass. Measures the frame with the call never made (medians of --batches batches of
--frames frames, and their spread; --tree measures another commit's built checkout, and --alternate N runs this tree and
--tree in turn, N times each, in child processes), the call after a frame (wall clock of the call, which synchronises) on a
100 m x 100 m grid at 10 cm and at 50 cm cells, without and with ground removal, beside cm_result_grid_map_device of the same
job (the ratio is reported, never gated on), and under CM_FLAG_PROFILE (a context of its own) the per-stage times of one call
with each ray kernel's share of it. Prints one JSON line (also appended to --out).

  python scripts/ray_cost.py --out profiles/ray_cost.txt
  python scripts/ray_cost.py --frame-only [--tree <checkout>]       # only the frame; --tree: another commit's built checkout
  python scripts/ray_cost.py --alternate 3 --tree <parent checkout>  # the frame on this tree and on the parent, in turn
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_ground.py's slabs (proceedFront's five), for every sensor
FRONT = [(30.0, 30.0, 2.5), (19.0, 11.0, 2.0), (4.0, 15.0, 1.5), (-4.0, 8.0, 0.3), (-15.0, 11.0, 0.5)]
GRIDS = {"cell_0.1": (0.1, 1000), "cell_0.5": (0.5, 200)}
ORIGIN = (-50.0, -50.0)
RAY_STAGES = ("ray_clear", "k_ray_mark", "k_ray_cast", "k_ray_finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--alternate", type=int, default=0, help="rounds of (this tree, --tree) frame-only child processes")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def emit(out):
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.alternate:
        runs = []
        for r in range(a.alternate):
            for label, tree in (("this", ROOT), ("parent", os.path.abspath(a.tree))):
                cmd = [sys.executable, os.path.abspath(__file__), "--frame-only", "--tree", tree, "--label", f"{label}#{r}",
                       "--frames", str(a.frames), "--batches", str(a.batches), "--warmup", str(a.warmup), "--n", str(a.n)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(p.stdout + p.stderr)
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        emit({"label": a.label, "alternating_frame_only": [{"label": r["label"], "frame_ms": r["frame"]["frame_ms"],
                                                              "spread": r["frame"]["frame_ms_spread"]} for r in runs]})
        return

    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2, crop_min=(-25.0,) * 3, crop_max=(25.0,) * 3)

    def frame(cm):
        t0 = time.perf_counter()
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        res = cm.merge_voxelize(params)
        assert res.status == capi.OK
        return res, time.perf_counter() - t0

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def context(flags, ground):
        cm = capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=flags)
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        if ground:
            cm.set_ground_removal(capi.make_ground_params([FRONT] * 4))
        return cm

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel, crop +-25 m",
           "frames": a.frames, "batches": a.batches, "sensor_translations": [[round(float(v), 3) for v in s.t_xyz] for s in sensors]}
    with context(capi.FLAG_OCCUPANCY, False) as cm:
        for _ in range(a.warmup):
            frame(cm)
        meds = [ms([frame(cm)[1] for _ in range(a.frames)]) for _ in range(a.batches)]
        res, _ = frame(cm)
        out["frame"] = dict(n_out=int(res.n_out), path_flags=int(res.path_flags), frame_ms_batches=meds,
                            frame_ms=round(float(np.median(meds)), 4), frame_ms_spread=round(max(meds) - min(meds), 4))
    if a.frame_only:
        emit(out)
        return
    for gname, ground in (("no_ground_removal", False), ("ground_removal", True)):
        rec = {}
        with context(capi.FLAG_OCCUPANCY, ground) as cm:
            t = {g: [] for g in GRIDS}
            tg = {g: [] for g in GRIDS}
            for f in range(a.warmup + a.frames):
                frame(cm)
                for g, (cell, n) in GRIDS.items():
                    dg = timed(lambda: cm.grid_map_device(ORIGIN, cell, n, n))[1]
                    dt = timed(lambda: cm.grid_rays_device(ORIGIN, cell, n, n))[1]
                    if f >= a.warmup:
                        tg[g].append(dg)
                        t[g].append(dt)
            for g in GRIDS:
                rec[g] = {"call_ms": ms(t[g]), "grid_map_call_ms": ms(tg[g]), "call_over_grid_map": round(ms(t[g]) / ms(tg[g]), 3)}
        with context(capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE, ground) as cm:
            for _ in range(3):
                frame(cm)
            for g, (cell, n) in GRIDS.items():
                for _ in range(3):
                    cm.grid_rays_device(ORIGIN, cell, n, n)
                st = [(name, round(tm, 4)) for name, tm in cm.stage_times()]
                total = sum(tm for _, tm in st)
                table = cm.grid_rays(ORIGIN, cell, n, n)
                image = cm.grid_ray_occupancy()
                base = cm.grid_occupancy()
                rec[g].update(stages_ms=st, share={name: round(sum(tm for nm, tm in st if nm == name) / total, 3) if total else None
                                                   for name in RAY_STAGES},
                              rays=int(table["n_end"].sum()), steps=int(table["n_pass"].sum(dtype=np.uint64)),
                              largest_n_pass=int(table["n_pass"].max()), cells_crossed=int((table["n_pass"] > 0).sum()),
                              cells_cleared=int(((base == -1) & (image == 0)).sum()), cells_unknown_left=int((image == -1).sum()))
        out[gname] = rec
    emit(out)


if __name__ == "__main__":
    main()
