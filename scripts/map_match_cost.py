#!/usr/bin/env python3
"""Cost of the scan matching layer behind the cost layer (cm_map_match_evaluate) in the workload of scripts/map_traj_cost.py:
cfg2's frame (4 x 1 M points, random SE(3) per sensor, clouds resident in HBM, 5 cm voxels, min 2 points per voxel), a window of
1024 x 1024 cells of 10 cm, the pose moving 0.37 m per frame, radii 0.35 / 1.05 m, scaling 3; a field of sigma 0.1 m cut at 0.5 m;
21 angles x 21 x 21 shifts and 61 angles x 41 x 41 shifts, two heading-table entries (0.18 degrees) apart, the prior off the
integration's pose by (+3, -2) cells.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps, in this order:
  frame        the frame on a context with no layer configured (medians of --batches batches of --frames frames, and their
               spread): the parent's frame, since no kernel of cm_merge_voxelize is touched;
  match        per candidate volume: the frame on a context with map, cost and matching layer, and behind every frame
               cm_map_match_evaluate (from the second frame on), cm_map_integrate and cm_map_cost_update, each timed on its own
               (wall clock of the call, which synchronises): integrate is the yardstick. Then the same sequence on a context with
               CM_FLAG_PROFILE for the per-stage times of an evaluate and of an integrate: k_match_mark beside k_map_mark is
               what reading each point once for all angles is judged against;
  frame        the first step again, to show the drift of the job.
Prints one JSON line (also appended to --out).

  python scripts/map_match_cost.py --out profiles/map_match_cost.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUMES = {"21x21x21": (10, 10, 10), "61x41x41": (30, 20, 20)}      # n_a, wx, wy
A_STRIDE, SIGMA, MAX_DIST = 2, 0.1, 0.5
OFF = (3, -2)                                        # cells the prior is off by


def step(a):
    """One GPU step in this process; prints its JSON record."""
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
    radii = (0.35, 1.05, 3.0)
    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def context(flags=0):
        cm = capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY | flags)
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        return cm

    def frame(cm):
        t0 = time.perf_counter()
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        assert cm.merge_voxelize(params).status == capi.OK
        return time.perf_counter() - t0

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def pose(k, off=(0, 0)):
        P = np.eye(3, 4, dtype=np.float32)
        P[0, 3], P[1, 3] = 0.37 * k + off[0] * a.cell, -0.11 * k + off[1] * a.cell
        return P

    def layers(cm, vol):
        n_a, wx, wy = VOLUMES[vol]
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        cm.map_match_configure(SIGMA, MAX_DIST, n_a, A_STRIDE, wx, wy, True)

    def sequence(cm, n_frames, stages=None):
        """frame, evaluate (from the second frame on), integrate, cost update; the wall times of each."""
        t = {"frame": [], "match_evaluate": [], "integrate": [], "cost_update": []}
        res = None
        for k in range(n_frames):
            t["frame"].append(frame(cm))
            if k:
                box = []
                t["match_evaluate"].append(timed(lambda: box.append(cm.map_match(pose(k, OFF)))))
                res = box[0]
                if stages is not None:
                    stages["evaluate"].append(cm.stage_times())
            t["integrate"].append(timed(lambda: cm.map_integrate(pose(k))))
            if stages is not None:
                stages["integrate"].append(cm.stage_times())
            t["cost_update"].append(timed(cm.map_cost_update))
        return t, res

    out = {"step": a.step, "volume": a.volume}
    if a.step == "frame":
        with context() as cm:
            for _ in range(a.warmup):
                frame(cm)
            meds = [ms([frame(cm) for _ in range(a.frames)]) for _ in range(a.batches)]
            out.update({"frame_ms_batches": meds, "frame_ms": round(float(np.median(meds)), 4), "frame_ms_spread": round(max(meds) - min(meds), 4)})
    elif a.step == "match":
        with context() as cm:
            layers(cm, a.volume)
            sequence(cm, a.warmup + 1)
            per = {}
            for _ in range(a.batches):
                layers(cm, a.volume)                             # (a fresh map: the poses start over)
                t, res = sequence(cm, a.frames)
                for name, v in t.items():
                    per.setdefault(name, []).append(ms(v))
            for name, v in per.items():
                out.update({f"{name}_ms_batches": v, f"{name}_ms": round(float(np.median(v)), 4), f"{name}_ms_spread": round(max(v) - min(v), 4)})
            out["last_match"] = {"k": res.k, "i": res.i, "j": res.j, "score": res.score, "n_cells": res.n_cells, "max_score": res.max_score,
                                 "sub": [res.sub[0], res.sub[1]]}
            cm.map_match(pose(a.frames - 1, OFF))                # (the volume is stale behind the last cost update)
            out["match_copy_ms"] = ms([timed(cm.map_match_scores) for _ in range(5)])
        with context(capi.FLAG_PROFILE) as cm:
            layers(cm, a.volume)
            stages = {"evaluate": [], "integrate": []}
            sequence(cm, 12, stages)
            for name, s in stages.items():
                s = s[3:]
                out[f"profile_{name}"] = [(n, round(float(np.median([x[j][1] for x in s])), 4)) for j, (n, _) in enumerate(s[-1])]
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a GPU step may take")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--volume", default=None, help="(internal) the candidate volume of that step")
    a = ap.parse_args()
    if a.step:
        return step(a)

    plan = [("frame", None)] + [("match", v) for v in VOLUMES] + [("frame", None)]
    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; window {a.size} x {a.size} cells of {a.cell} m; "
                                      f"radii 0.35 / 1.05 m, scaling 3; field sigma {SIGMA} m cut at {MAX_DIST} m; a_stride {A_STRIDE}; sub-cell on; "
                                      f"prior off by {OFF} cells", "frames": a.frames, "batches": a.batches, "steps": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("frames", "batches", "warmup", "n", "cell", "size")]
    for name, vol in plan:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name] + passed + (["--volume", vol] if vol else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": name, "volume": vol, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            break
        out["steps"].append(json.loads(lines[-1][len("RESULT "):]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
