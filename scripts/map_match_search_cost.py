#!/usr/bin/env python3
"""Cost of the search layer behind the cost layer (cm_map_match_search, branch-and-bound scan matching over wide windows) beside
the exhaustive layer (cm_map_match_evaluate), in the workload of scripts/map_match_cost.py: a window of 1024 x 1024 cells of
10 cm, radii 0.35 / 1.05 m, scaling 3, a field of sigma 0.1 m cut at 0.5 m, 2 n_a + 1 = 5 angles two heading-table entries apart.
Two scenes, and every record says which one it is:
  cfg2   cfg2's frame (4 x 1 M points, random SE(3) per sensor, 5 cm voxels, min 2 points per voxel). Its random cloud makes the
         map a smear: the bound has little to prune.
  walls  one sensor, a synthetic building outline: the walls of a 60 m x 44 m hall with inner walls every 12 m, doorways in them,
         points every 2.5 cm up to 2 m height. Here the field has structure and the bound can prune.
The map holds one frame integrated under the identity; the same frame is then matched with the prior off by (0.45 w, -0.3 w)
cells, w the window's half-width, so that the answer lies well inside the range and far from the prior.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps, per scene:
  compare   both layers on one context at wx = wy = 64 (the exhaustive layer's cap): wall clock of the synchronising calls
            (medians of --batches batches of --evals evaluates), the two results compared byte for byte, the search's info;
  scale     the search at +-128 (depth 5), +-256 (depth 6) and +-512 (depth 7) cells with the info's per-level counts (a
            capacity overflow is recorded, not an error);
  stages    the per-stage times (CM_FLAG_PROFILE, a context of its own) of the search at +-64 and +-512 and of the exhaustive
            layer at +-64.
Prints one JSON line (also appended to --out).

  python scripts/map_match_search_cost.py --out profiles/map_match_search_cost.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_A, A_STRIDE, SIGMA, MAX_DIST = 2, 2, 0.1, 0.5
SCALES = {128: 5, 256: 6, 512: 7}                    # half-width: depth
MAX_NODES, MAX_CELLS = 1 << 22, 1 << 18


def walls(np):
    """(n, 3) points of the hall's walls in the vehicle frame, the vehicle at (3.1, -2.3) off its centre."""
    segs = [((-30, -22), (30, -22)), ((-30, 22), (30, 22)), ((-30, -22), (-30, 22)), ((30, -22), (30, 22))]
    for x in (-18, -6, 6, 18):
        segs += [((x, -22), (x, -3)), ((x, 1), (x, 22))]             # a doorway of 4 m in every inner wall
    for y in (-10, 12):
        segs += [((-30, y), (-8, y)), ((-4, y), (14, y)), ((18, y), (30, y))]
    pts = []
    for (x0, y0), (x1, y1) in segs:
        n = int(max(abs(x1 - x0), abs(y1 - y0)) / 0.025) + 1
        t = np.linspace(0.0, 1.0, n)
        for z in np.arange(0.05, 2.0, 0.1):
            pts.append(np.stack([x0 + (x1 - x0) * t + 3.1, y0 + (y1 - y0) * t - 2.3, np.full(n, z)], axis=1))
    return np.concatenate(pts).astype(np.float32)


def step(a):
    """One GPU step in this process; prints its JSON record."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams, xyzi_cloud

    if a.scene == "cfg2":
        sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    else:
        w = walls(np)
        sensors = [xyzi_cloud(w, np.ones(len(w), np.float32), t_xyz=(0.0, 0.0, 0.0))]
    n_total = sum(s.n for s in sensors)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def context(flags=0):
        cm = capi.CloudMerger(max_points_total=n_total, max_sensors=len(sensors), flags=capi.FLAG_OCCUPANCY | flags)
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        assert cm.merge_voxelize(params).status == capi.OK
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(0.35, 1.05, 3.0)
        cm.map_integrate(None)
        cm.map_cost_update()
        return cm

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    def prior(w):
        P = np.eye(3, 4, dtype=np.float32)
        P[0, 3], P[1, 3] = int(0.45 * w) * a.cell, -int(0.3 * w) * a.cell
        return P

    def info_of(i):
        return {"bound": i.bound, "n_roots": i.n_roots, "scored": list(i.scored), "live": list(i.live), "n_probe": i.n_probe, "overflow_level": i.overflow_level}

    def result_of(r):
        return {"k": r.k, "i": r.i, "j": r.j, "score": r.score, "n_cells": r.n_cells, "max_score": r.max_score}

    def search(cm, w, depth):
        """Configure and run once: (result or None, info)."""
        cm.map_match_search_configure(SIGMA, MAX_DIST, N_A, A_STRIDE, w, w, depth, MAX_NODES, MAX_CELLS, True)
        try:
            return cm.map_match_search(prior(w))
        except capi.CloudMergeError as e:
            if e.status != capi.CAPACITY:
                raise
            return None, e.info

    def batches(fn):
        slow = timed(fn) > 0.25                      # (a call of a quarter second and more: one batch of two, to keep the step short)
        meds = [ms([timed(fn) for _ in range(2 if slow else a.evals)]) for _ in range(1 if slow else a.batches)]
        return {"ms_batches": meds, "ms": round(float(np.median(meds)), 4), "ms_spread": round(max(meds) - min(meds), 4)}

    out = {"step": a.step, "scene": a.scene, "points": n_total}
    if a.step == "compare":
        with context() as cm:
            cm.map_match_configure(SIGMA, MAX_DIST, N_A, A_STRIDE, 64, 64, True)
            res, info = search(cm, 64, 4)
            ex = cm.map_match(prior(64))
            out["exhaustive"] = dict(batches(lambda: cm.map_match(prior(64))), result=result_of(ex))
            if res is None:
                out["search"] = {"capacity": info_of(info)}
            else:
                out["search"] = dict(batches(lambda: cm.map_match_search(prior(64))), result=result_of(res), info=info_of(info), depth=4,
                                     equal_bytes=bytes(res) == bytes(ex))
    elif a.step == "scale":
        with context() as cm:
            out["search"] = {}
            for w, depth in SCALES.items():
                res, info = search(cm, w, depth)
                rec = {"depth": depth, "info": info_of(info)}
                if res is not None:
                    rec.update(batches(lambda: cm.map_match_search(prior(w))), result=result_of(res))
                out["search"][str(w)] = rec
    elif a.step == "stages":
        with context(capi.FLAG_PROFILE) as cm:
            med = lambda runs: [(n, round(float(np.median([x[j][1] for x in runs])), 4)) for j, (n, _) in enumerate(runs[-1])]
            cm.map_match_configure(SIGMA, MAX_DIST, N_A, A_STRIDE, 64, 64, True)
            runs = []
            for _ in range(7):
                cm.map_match(prior(64))
                runs.append(cm.stage_times())
            out["exhaustive_64"] = med(runs[2:])
            for w, depth in ((64, 4), (512, 7)):
                res, info = search(cm, w, depth)
                if res is None:
                    out[f"search_{w}"] = {"capacity": info_of(info)}
                    continue
                runs = []
                for _ in range(7):
                    cm.map_match_search(prior(w))
                    runs.append(cm.stage_times())
                out[f"search_{w}"] = med(runs[2:])
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=10)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor of cfg2")
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--scenes", default="walls,cfg2")
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds a GPU step may take")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--scene", default=None, help="(internal) the scene of that step")
    a = ap.parse_args()
    if a.step:
        return step(a)

    plan = [(s, sc) for sc in a.scenes.split(",") for s in ("compare", "scale", "stages")]
    out = {"label": a.label, "shape": f"window {a.size} x {a.size} cells of {a.cell} m; radii 0.35 / 1.05 m, scaling 3; field sigma {SIGMA} m cut at {MAX_DIST} m; "
                                      f"n_a {N_A}, a_stride {A_STRIDE}; sub-cell on; max_nodes {MAX_NODES}, max_cells {MAX_CELLS}; prior off by (0.45 w, -0.3 w) cells",
           "evals": a.evals, "batches": a.batches, "steps": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("evals", "batches", "n", "cell", "size")]
    for name, scene in plan:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--scene", scene] + passed
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": name, "scene": scene, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
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
