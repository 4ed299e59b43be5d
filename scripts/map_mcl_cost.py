#!/usr/bin/env python3
"""Cost of the localisation layer behind the cost layer (cm_map_mcl_predict, cm_map_mcl_update) in the walls
scene of scripts/map_match_search_cost.py: a window of 1024 x 1024 cells of 10 cm, radii 0.35 / 1.05 m, scaling 3, a field of
sigma 0.1 m cut at 0.5 m; one sensor, the walls of a 60 m x 44 m hall with inner walls and doorways, points every 2.5 cm up to
2 m height. The map holds that frame integrated under the identity; the particles start around the true pose (sd 0.3 m, 0.3 m,
0.1 rad) and every round is one predict (no motion, sd 0.03 / 0.03 / 0.02: the frame stays the same) and one update of that frame.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps:
  update    per (n_particles, max_beams) of 4096 / 16384 / 65536 x 256 / 4096: the per-stage times of an update and of a
            predict (CM_FLAG_PROFILE, medians over --rounds rounds after two warm-up rounds), the wall clock of the two
            synchronising calls, the beams the update used and the lookups per second of k_mcl_score (n_particles x n_beams
            over its time);
  resample  at 65536 x 256 the update with CM_MCL_RESAMPLE_ALWAYS and with resample_frac 0: k_mcl_resample with the gather and
            without it;
  match     for scale, cm_map_match_evaluate on the same map and frame: 5 angles, shifts of +-10 cells, wall clock and stages.
Prints one JSON line (also appended to --out).

  python scripts/map_mcl_cost.py --out profiles/map_mcl_cost.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, MAX_DIST, TAU, RANGE_CELLS = 0.1, 0.5, 8.0, 512
SHAPES = [(n, b) for n in (4096, 16384, 65536) for b in (256, 4096)]


def step(a):
    """One GPU step in this process; prints its JSON record."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi
    from cloud_merger_amd.types import MergeParams, xyzi_cloud
    from map_match_search_cost import walls

    w = walls(np)
    sensors = [xyzi_cloud(w, np.ones(len(w), np.float32), t_xyz=(0.0, 0.0, 0.0))]
    n_total = sum(s.n for s in sensors)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    med = lambda runs: [(n, round(float(np.median([x[j][1] for x in runs])), 4)) for j, (n, _) in enumerate(runs[-1])]
    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    cm = capi.CloudMerger(max_points_total=n_total, max_sensors=1, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE)
    cm.set_transform(0, sensors[0].q_xyzw, sensors[0].t_xyz)
    cm.submit_device(0, clouds[0].data_ptr(), sensors[0].n, 16, 0, 4, 8, 12)
    assert cm.merge_voxelize(params).status == capi.OK
    cm.map_configure(a.cell, a.size, a.size)
    cm.map_cost_configure(0.35, 1.05, 3.0)
    cm.map_integrate(None)
    cm.map_cost_update()

    def rounds(n, beams, frac, always):
        cm.map_mcl_configure(n, beams, RANGE_CELLS, SIGMA, MAX_DIST, TAU, frac, always, 1)
        cm.map_mcl_init_pose(0.0, 0.0, 0.0, 0.3, 0.3, 0.1)
        pred, upd, wall_p, wall_u, info = [], [], [], [], None
        for _ in range(a.rounds + 2):
            wall_p.append(timed(lambda: cm.map_mcl_predict(0.0, 0.0, 0.0, 0.03, 0.03, 0.02)))
            pred.append(cm.stage_times())
            t0 = time.perf_counter()
            info = cm.map_mcl_update()
            wall_u.append(time.perf_counter() - t0)
            upd.append(cm.stage_times())
        stages = med(upd[2:])
        score = dict(stages)["k_mcl_score"]
        return {"n_particles": n, "max_beams": beams, "n_cells": info.n_cells, "stride": info.stride, "n_beams": info.n_beams, "update_stages_ms": stages,
                "predict_stages_ms": med(pred[2:]), "update_wall_ms": ms(wall_u[2:]), "predict_wall_ms": ms(wall_p[2:]), "resampled_last": info.resampled,
                "n_eff_last": round(info.n_eff, 1), "lookups_per_s": round(n * info.n_beams / (score * 1e-3)) if score > 0 else None}

    out = {"step": a.step, "points": n_total}
    if a.step == "update":
        out["shapes"] = [rounds(n, b, 0.5, False) for n, b in SHAPES]
    elif a.step == "resample":
        out["always"] = rounds(65536, 256, 1.0, True)
        out["never"] = rounds(65536, 256, 0.0, False)
    elif a.step == "match":
        cm.map_match_configure(SIGMA, MAX_DIST, 2, 2, 10, 10, True)
        P = np.eye(3, 4, dtype=np.float32)
        runs, wall = [], []
        for _ in range(a.rounds + 2):
            wall.append(timed(lambda: cm.map_match(P)))
            runs.append(cm.stage_times())
        out["match_evaluate"] = {"stages_ms": med(runs[2:]), "wall_ms": ms(wall[2:]), "candidates": 5 * 21 * 21}
    cm.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a GPU step may take")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    a = ap.parse_args()
    if a.step:
        return step(a)

    out = {"label": a.label, "shape": f"window {a.size} x {a.size} cells of {a.cell} m; radii 0.35 / 1.05 m, scaling 3; field sigma {SIGMA} m cut at {MAX_DIST} m; "
                                      f"tau {TAU}, range_cells {RANGE_CELLS}; walls scene; predict + update per round",
           "rounds": a.rounds, "steps": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("rounds", "cell", "size")]
    for name in ("update", "resample", "match"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name] + passed
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": name, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
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
