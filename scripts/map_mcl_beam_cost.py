#!/usr/bin/env python3
"""Cost of the localisation layer's beam model (cm_map_mcl_beam_configure, k_mcl_beam) in the walls scene and on
the six particle x beam shapes of scripts/map_mcl_cost.py (§29): a window of 1024 x 1024 cells of 10 cm, radii 0.35 / 1.05 m,
scaling 3; one sensor, the walls of a 60 m x 44 m hall, the map holding that frame integrated under the identity; the particles
start around the true pose (sd 0.3 m, 0.3 m, 0.1 rad) and every round is one predict (no motion, sd 0.03 / 0.03 / 0.02) and
one update of that frame. The beam model: over_cells 8, sigma 0.1 m, z 0.75 / 0.125 / 0.125.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps, each over the six shapes, medians over --rounds rounds after two warm-up rounds:
  off       the field score (the mode off): k_mcl_score and the update's wall clock, the yardstick of §29;
  beam      the default walk (it jumps by the skip bytes), two rays per lane in flight: k_mcl_beam, k_mcl_steps of the first
            update, the update's wall clock, rays per second (n_particles x n_beams over k_mcl_beam's time), the outcome counts;
  plain     CM_MCL_BEAM_PLAIN, cell by cell through the image;
  walks1, walks4   the default walk with one and with four rays per lane in flight (CM_MCL_BEAM_WALKS in the environment);
  reads     on the CPU, the cells both walks read per ray, counted by the restatement (tests/mcl_beam_ref.py) over the first 32
            particles x the beams of the 4096 x 256 shape.
The four beam steps hash the weight table of their last update per shape; the hashes must agree (the same bytes in every mode).
Prints one JSON line (also appended to --out).

  python scripts/map_mcl_beam_cost.py --out profiles/map_mcl_beam_cost.txt
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
SHAPES = [(n, b) for n in (4096, 16384, 65536) for b in (256, 4096)]
BEAM = dict(over_cells=8, sigma=0.1, z_hit=0.75, z_short=0.125, z_rand=0.125)
STEPS = {"off": None, "beam": {}, "plain": {}, "walks1": {"CM_MCL_BEAM_WALKS": "1"}, "walks4": {"CM_MCL_BEAM_WALKS": "4"}, "reads": {}}


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

    def rounds(n, beams):
        cm.map_mcl_configure(n, beams, RANGE_CELLS, SIGMA, MAX_DIST, TAU, 0.5, False, 1)
        if a.step != "off":
            cm.map_mcl_beam_configure(plain=a.step == "plain", **BEAM)
        cm.map_mcl_init_pose(0.0, 0.0, 0.0, 0.3, 0.3, 0.1)
        upd, wall_u, info, first = [], [], None, None
        for _ in range(a.rounds + 2):
            cm.map_mcl_predict(0.0, 0.0, 0.0, 0.03, 0.03, 0.02)
            t0 = time.perf_counter()
            info = cm.map_mcl_update()
            wall_u.append(time.perf_counter() - t0)
            upd.append(cm.stage_times())
            first = first or dict(upd[0])
        stages = med(upd[2:])
        row = {"n_particles": n, "max_beams": beams, "n_beams": info.n_beams, "update_stages_ms": stages, "update_wall_ms": ms(wall_u[2:])}
        if a.step == "off":
            row["k_mcl_score_ms"] = dict(stages)["k_mcl_score"]
            return row
        kernel = dict(stages)["k_mcl_beam"]
        bi = cm.map_mcl_beam_info()
        row.update(k_mcl_beam_ms=kernel, k_mcl_steps_first_ms=first.get("k_mcl_steps"), rays=int(bi.n_rays),
                   rays_per_s=round(bi.n_rays / (kernel * 1e-3)) if kernel > 0 else None,
                   counts={f: int(getattr(bi, f)) for f, _ in capi.MclBeamInfo._fields_[1:]},
                   weights_sha1=hashlib.sha1(cm.map_mcl_weights()[0].tobytes()).hexdigest())
        return row

    out = {"step": a.step, "points": n_total, "walks": os.environ.get("CM_MCL_BEAM_WALKS", "2")}
    if a.step == "reads":
        from tests import mcl_beam_ref as br
        from tests import mcl_ref as mr
        from tests import map_ref as mpr
        n, beams = SHAPES[0]
        cm.map_mcl_configure(n, beams, RANGE_CELLS, SIGMA, MAX_DIST, TAU, 0.5, False, 1)
        cm.map_mcl_init_pose(0.0, 0.0, 0.0, 0.3, 0.3, 0.1)
        parts = cm.map_mcl_particles()[:32]
        image, minfo = cm.map_occupancy()
        _, dist2, _ = cm.map_cost()
        mq = mpr.params(a.cell, a.size, a.size)
        q = dict(mr.params(), n_particles=n, max_beams=beams, range_cells=RANGE_CELLS)
        A = cm.merged(n_total)
        bm = mr.beams(np.stack([A["x"], A["y"], A["z"], A["intensity"]], axis=1), mq, q)
        b = dict(br.params(), **BEAM)
        S, counts, reads = br.scores(parts, bm, image, mq, tuple(minfo.anchor), capi.traj_directions(), b)
        # the same rays by the skip bytes: the origins and the lines as scores() forms them, through its own cell arithmetic
        steps = br.steps_of(dist2.astype(np.int64))
        rays = br.rays_of(parts, bm, mq, tuple(minfo.anchor), capi.traj_directions(), image.shape)[:4]
        cls_p, idx_p, reads_p = br.walk_plain_many(image, *rays, b["over_cells"])
        cls_s, idx_s, reads_s = br.walk_skip_many(steps, *rays, b["over_cells"])
        assert (cls_p == cls_s).all() and (idx_p == idx_s).all() and int(reads_p.sum()) == reads
        out["reads_per_ray"] = {"rays": int(len(rays[0])), "plain": round(float(reads_p.mean()), 2), "default": round(float(reads_s.mean()), 2),
                                "mean_line_steps": round(float(np.maximum(np.abs(rays[2]), np.abs(rays[3])).mean()), 1), "counts": counts}
    else:
        out["shapes"] = [rounds(n, b) for n, b in SHAPES]
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
                                      f"tau {TAU}, range_cells {RANGE_CELLS}; beam model {BEAM}; walls scene; predict + update per round",
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
    hashes = [[row["weights_sha1"] for row in s["shapes"]] for s in out["steps"] if s["step"] in ("beam", "plain", "walks1", "walks4")]
    out["same_bytes_in_every_mode"] = bool(hashes) and all(h == hashes[0] for h in hashes)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 1 if "failed" in out or not out["same_bytes_in_every_mode"] else 0


if __name__ == "__main__":
    sys.exit(main())
