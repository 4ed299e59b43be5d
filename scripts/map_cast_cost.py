#!/usr/bin/env python3
"""Cost of the cast layer behind the cost layer (cm_map_cast_evaluate) in the walls scene of
scripts/map_match_search_cost.py: a window of 1024 x 1024 cells of 10 cm, radii 0.35 / 1.05 m, scaling 3; one sensor, the walls
of a 60 m x 44 m hall with inner walls and doorways. The map holds that frame integrated under the identity. The poses are
drawn once, uniformly over the hall with any heading; the bearings are evenly spaced.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. One step per range_cells of 256 and 1024; in it, per (poses, bearings) of 1 x 360, 4096 x 64, 4096 x 360 and
65536 x 64 and per mode (the default walk, which skips by the distance field, and CM_CAST_PLAIN): the per-stage times of an
evaluate (CM_FLAG_PROFILE, medians over --rounds rounds after two warm-up rounds; k_cast_steps runs only in the first evaluate
after a cost update and is reported from a round of its own), the wall clock of the synchronising call and the rays by status;
the two modes' rays are compared byte for byte. Then, on the CPU, the cell reads per ray of both walks counted by the
restatement (tests/cast_ref.py) over the first 256 poses x 64 bearings, the skip walk capped at 255 steps as the device's table.
Prints one JSON line (also appended to --out).

  python scripts/map_cast_cost.py --out profiles/map_cast_cost.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 360), (4096, 64), (4096, 360), (65536, 64)]


def step(a):
    """One GPU step in this process; prints its JSON record."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi
    from cloud_merger_amd.types import MergeParams, xyzi_cloud
    from map_match_search_cost import walls
    from tests import cast_ref as kr

    w = walls(np)
    sensors = [xyzi_cloud(w, np.ones(len(w), np.float32), t_xyz=(0.0, 0.0, 0.0))]
    n_total = sum(s.n for s in sensors)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    med = lambda runs: [(n, round(float(np.median([dict(x)[n] for x in runs])), 4)) for n, _ in runs[-1]]
    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    cm = capi.CloudMerger(max_points_total=n_total, max_sensors=1, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE)
    cm.set_transform(0, sensors[0].q_xyzw, sensors[0].t_xyz)
    cm.submit_device(0, clouds[0].data_ptr(), sensors[0].n, 16, 0, 4, 8, 12)
    assert cm.merge_voxelize(params).status == capi.OK
    cm.map_configure(a.cell, a.size, a.size)
    cm.map_cost_configure(0.35, 1.05, 3.0)
    cm.map_integrate(None)
    cm.map_cost_update()

    rng = np.random.default_rng(1)
    n_max = max(n for n, _ in SHAPES)
    poses = np.zeros(n_max, capi.CAST_POSE_DTYPE)
    poses["x"], poses["y"] = rng.uniform(-29.5, 29.5, n_max), rng.uniform(-21.5, 21.5, n_max)
    poses["h"] = rng.integers(0, 1 << 32, n_max, dtype=np.uint64)
    R = a.range_cells

    def rounds(n, nb, plain):
        cm.map_cast_configure(n, nb, R, plain)
        runs, wall, info = [], [], None
        for _ in range(a.rounds + 2):
            t0 = time.perf_counter()
            info = cm.map_cast(poses[:n])
            wall.append(time.perf_counter() - t0)
            runs.append(cm.stage_times())
        rec = {"stages_ms": med(runs[2:]), "wall_ms": ms(wall[2:]), "n_max": info.n_max, "n_hit": info.n_hit, "n_off_map": info.n_off_map,
               "n_no_origin": info.n_no_origin}
        if not plain:
            rec["k_cast_steps_ms"] = round(dict(runs[0])["k_cast_steps"], 4)
        stage = dict(rec["stages_ms"])["k_cast_rays"]
        rec["rays_per_s"] = round(n * nb / (stage * 1e-3)) if stage > 0 else None
        return rec, cm.map_cast_rays()[0].tobytes()

    out = {"step": a.step, "range_cells": R, "points": n_total, "shapes": []}
    for n, nb in SHAPES:
        skip, rays_skip = rounds(n, nb, False)
        plain, rays_plain = rounds(n, nb, True)
        out["shapes"].append({"poses": n, "bearings": nb, "default": skip, "plain": plain, "equal_bytes": rays_skip == rays_plain})
    image, minfo = cm.map_occupancy()
    dist2 = cm.map_cost()[1].astype(np.int64)
    dist2[dist2 == capi.MAP_DIST_NONE] = kr.DIST_NONE
    tab = capi.traj_directions()
    cm.close()
    # the cell reads of both walks, by the restatement, on a sample
    sample, nb = poses[:256], 64
    ox, oy, ok = kr.origin_cells(sample, a.cell, tuple(minfo.anchor), a.size, a.size)
    E = kr.directions(R, tab).astype(np.int64)[kr.entries(sample["h"], kr.even_bearings(nb))]
    sel = np.flatnonzero(np.repeat(ok, nb))
    args = (np.repeat(ox, nb)[sel], np.repeat(oy, nb)[sel], E[..., 0].reshape(-1)[sel], E[..., 1].reshape(-1)[sel])
    plain, skip = kr.walk_plain(image, *args), kr.walk_skip(image, dist2, *args, cap=255)
    assert all((p == s).all() for p, s in zip(plain[:4], skip[:4]))
    out["reads_per_ray"] = {"rays": int(len(sel)), "plain": round(float(plain[4].mean()), 2), "default": round(float(skip[4].mean()), 2),
                            "mean_k": round(float(plain[0].mean()), 2)}
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=200, help="seconds a GPU step may take")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--range-cells", type=int, default=256, help="(internal) the step's range_cells")
    a = ap.parse_args()
    if a.step:
        return step(a)

    out = {"label": a.label, "shape": f"window {a.size} x {a.size} cells of {a.cell} m; radii 0.35 / 1.05 m, scaling 3; walls scene; poses uniform over the hall, "
                                      f"evenly spaced bearings; one evaluate per round", "rounds": a.rounds, "steps": []}
    passed = [f"--{k}={getattr(a, k)}" for k in ("rounds", "cell", "size")]
    for R in (256, 1024):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", f"range{R}", f"--range-cells={R}"] + passed
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": f"range{R}", "returncode": r.returncode, "stderr": r.stderr[-2000:]}
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
