#!/usr/bin/env python3
"""Cost of the localisation layer's hypotheses and recovery (cm_map_mcl_hyp_configure, k_mcl_hyp_*) in the walls
scene of scripts/map_mcl_cost.py (§29) at its smallest and its largest shape, 4096 particles x 249 beams and 65536 x 2358: a
window of 1024 x 1024 cells of 10 cm, radii 0.35 / 1.05 m, scaling 3; one sensor, the walls of a 60 m x 44 m hall, the map
holding that frame integrated under the identity. Every round is one predict and one update of that frame. Two beliefs:
  spread      the particles start uniformly over the free cells and the bins are 1/16 m and 256 headings wide: nearly every
              particle is a bin and a component of its own, the table's worst load and the pick's longest search;
  converged   the particles start on the true pose with no spread and do not move: one bin, one component, every lane of every
              wave adds to one record.
The mode: bin_q 512 (64 in the spread belief), heading_bits 5 (8), max_hyp 8 (64), inject_max n / 4, alpha 0.05 / 0.5.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps, each over the two shapes and the two beliefs, medians over --rounds rounds after two warm-up rounds:
  off     the mode off: the update's stages and wall clock, the yardstick of §29;
  on      the mode on: the same, the stages of the mode summed, the counts of the last update;
  noagg   the mode on with CM_MCL_HYP_NO_AGG=1 (every lane sends its own atomics), the converged belief only: what the
          per-wave aggregation buys.
The on and noagg steps hash the hypotheses of their last update; the hashes of the converged belief must agree.
Prints one JSON line (also appended to --out).

  python scripts/map_mcl_hyp_cost.py --out profiles/map_mcl_hyp_cost.txt
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA, MAX_DIST, TAU, RANGE_CELLS = 0.1, 0.5, 8.0, 512
SHAPES = [(4096, 256), (65536, 4096)]
STEPS = {"off": None, "on": {}, "noagg": {"CM_MCL_HYP_NO_AGG": "1"}}
HYP = {"spread": dict(bin_m=0.0625, heading_bits=8, max_hyp=64), "converged": dict(bin_m=0.5, heading_bits=5, max_hyp=8)}


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

    cm = capi.CloudMerger(max_points_total=n_total, max_sensors=1, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE)
    cm.set_transform(0, sensors[0].q_xyzw, sensors[0].t_xyz)
    cm.submit_device(0, clouds[0].data_ptr(), sensors[0].n, 16, 0, 4, 8, 12)
    assert cm.merge_voxelize(params).status == capi.OK
    cm.map_configure(a.cell, a.size, a.size)
    cm.map_cost_configure(0.35, 1.05, 3.0)
    cm.map_integrate(None)
    cm.map_cost_update()

    def rounds(n, beams, belief):
        # resample_frac 0 keeps the belief as it started: the step measures the same work in every round
        cm.map_mcl_configure(n, beams, RANGE_CELLS, SIGMA, MAX_DIST, TAU, 0.0, False, 1)
        if a.step != "off":
            cm.map_mcl_hyp_configure(inject_max=n // 4, alpha_slow=0.05, alpha_fast=0.5, **HYP[belief])
        if belief == "spread":
            cm.map_mcl_init_uniform()
        else:
            cm.map_mcl_init_pose(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        upd, wall_u, info = [], [], None
        for _ in range(a.rounds + 2):
            cm.map_mcl_predict(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
            t0 = time.perf_counter()
            info = cm.map_mcl_update()
            wall_u.append(time.perf_counter() - t0)
            upd.append(cm.stage_times())
        stages = med(upd[2:])
        row = {"n_particles": n, "max_beams": beams, "n_beams": info.n_beams, "belief": belief, "update_stages_ms": stages, "update_wall_ms": ms(wall_u[2:]),
               "resampled": info.resampled}
        if a.step == "off":
            return row
        hyps, hi = cm.map_mcl_hypotheses()
        own = [v for k, v in stages if "hyp" in k or k in ("k_mcl_free_bits",)] + [v for k, v in stages[9:] if k == "k_mcl_compact"]
        row.update(hyp_stages_ms=round(sum(own), 4), n_bins=hi.n_bins, n_components=hi.n_components, n_hyp=hi.n_hyp, n_kld=hi.n_kld, n_inject=hi.n_inject,
                   n_free=hi.n_free, hyp_sha1=hashlib.sha1(b"".join(bytes(h) for h in hyps) + bytes(hi)).hexdigest())
        return row

    beliefs = ("converged",) if a.step == "noagg" else ("spread", "converged")
    out = {"step": a.step, "points": n_total, "no_agg": os.environ.get("CM_MCL_HYP_NO_AGG", "0"),
           "shapes": [rounds(n, b, belief) for n, b in SHAPES for belief in beliefs]}
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
                                      f"tau {TAU}, range_cells {RANGE_CELLS}; hypotheses {HYP}; inject_max n / 4; walls scene; predict + update per round",
           "rounds": a.rounds, "steps": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("rounds", "cell", "size")]
    for name, env in STEPS.items():
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name] + passed
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": name, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            break
        out["steps"].append(json.loads(lines[-1][len("RESULT "):]))
    by = {s["step"]: {(r["n_particles"], r["belief"]): r.get("hyp_sha1") for r in s["shapes"]} for s in out["steps"]}
    out["same_bytes_with_and_without_aggregation"] = "noagg" in by and all(by["on"][k] == v for k, v in by["noagg"].items())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 1 if "failed" in out or not out["same_bytes_with_and_without_aggregation"] else 0


if __name__ == "__main__":
    sys.exit(main())
