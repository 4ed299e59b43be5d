#!/usr/bin/env python3
"""Cost of the rollout layer behind the plan layer (cm_map_traj_evaluate) in the workload of scripts/map_plan_cost.py: cfg2's
frame (4 x 1 M points, random SE(3) per sensor, clouds resident in HBM, 5 cm voxels, min 2 points per voxel), a window of
1000 x 1000 cells of 10 cm, the pose moving 0.37 m per frame, radii 0.35 / 1.05 m, scaling 3, navfn's 50 / 205 with unknown cells
allowed, the goal 40 m ahead of the vehicle; 33 x 65 velocity samples, 40 steps of 0.1 s, v in 0.5 .. 8 m/s, w in +-0.8 rad/s, a
footprint of 4.5 m x 1.9 m (1 m behind the centre, 3.5 m ahead) on the node's lattice, which the cap coarsens to 24 x 10 points.

One job. Every GPU step is a child process of this script under a time limit of its own, and the job ends at the first step
that fails. The steps, in this order:
  frame        the frame on a context with no layer configured (medians of --batches batches of --frames frames, and their
               spread): the parent's frame, since no kernel of cm_merge_voxelize is touched;
  layers       the frame on a context with map, cost, plan and rollout layer, and behind every frame cm_map_integrate,
               cm_map_cost_update, cm_map_plan_update, cm_map_plan_path and cm_map_traj_evaluate, each timed on its own (wall
               clock of the call, which synchronises): cost update and path are the yardsticks. cfg2's vehicle stands inside its
               cloud, so most samples end at an early pose; the step therefore also measures, once, an open field (no obstacle,
               unknown allowed), where every sample runs all its steps: the most a call can cost at these parameters;
  profile      the per-stage times of an evaluate under CM_FLAG_PROFILE, in both scenes;
  variants     `layers` (open field only) and `profile` again on every variant library found beside the shipped one: --build
               compiles them first (on the machine that has the compiler, before the job): the heading table staged in LDS
               (CM_TRAJ_DIRS_LDS 1) and the step batch at another size (CM_TRAJ_STEP_BATCH 2 and 8);
  frame        the first step again, to show the drift of the job.
Prints one JSON line (also appended to --out).

  python scripts/map_traj_cost.py --build
  python scripts/map_traj_cost.py --out profiles/map_traj_cost.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "cloud_merger_amd", "lib")
VARIANTS = {"dirs_lds": ["-DCM_TRAJ_DIRS_LDS=1"], "batch2": ["-DCM_TRAJ_STEP_BATCH=2"], "batch8": ["-DCM_TRAJ_STEP_BATCH=8"]}
SAMPLES, STEPS, DT, V, W = (33, 65), 40, 0.1, (0.5, 8.0), (-0.8, 0.8)
FOOT = (-1.0, 3.5, 0.95)


def variant_path(name):
    return os.path.join(LIB_DIR, f"libcloudmerge_hip_traj_{name}.so")


def build_variants():
    sys.path.insert(0, ROOT)
    from cloud_merger_amd import build as b
    os.makedirs(LIB_DIR, exist_ok=True)
    for name, defines in VARIANTS.items():
        cmd = [b.hipcc()] + b.FLAGS + ["-Wl,--version-script=" + b.VERSION_SCRIPT, "-I", b.CSRC, "-o", variant_path(name)] + defines + \
              [os.path.join(b.CSRC, s) for s in b.SOURCES]
        subprocess.run(cmd, cwd=b.CSRC, check=True)
        print(variant_path(name))


def lattice(x_back, x_front, half_width, cell, cap=256):
    """The node's footprint lattice (traj_footprint_lattice in host/merger_node.cpp)."""
    import math
    import numpy as np
    n_x, n_y = math.ceil((x_front - x_back) / (0.5 * cell)) + 1, math.ceil(2 * half_width / (0.5 * cell)) + 1
    if n_x * n_y > cap:
        scale = math.sqrt(cap / (n_x * n_y))
        n_x, n_y = max(1, int(n_x * scale)), max(1, int(n_y * scale))
        n_x = min(n_x, cap)
        n_y = min(n_y, cap // n_x)
    xs = np.linspace(x_back, x_front, n_x) if n_x > 1 else np.array([0.5 * (x_back + x_front)])
    ys = np.linspace(-half_width, half_width, n_y) if n_y > 1 else np.array([0.0])
    return np.array([(x, y) for x in xs for y in ys], np.float32), (n_x, n_y)


def step(a):
    """One GPU step in this process; prints its JSON record."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams, xyzi_cloud
    if a.lib:
        capi.LIB_PATH = variant_path(a.lib)          # a variant build of the same sources

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()
    params = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=2)
    radii, plan = (0.35, 1.05, 3.0), (50, 205, True)
    foot, foot_n = lattice(*FOOT, a.cell)
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

    def pose(k):
        P = np.eye(3, 4, dtype=np.float32)
        P[0, 3], P[1, 3] = 0.37 * k, -0.11 * k
        return P

    def batches(cm, after=()):
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

    class Calls:
        def __init__(self, cm):
            self.cm, self.k, self.info = cm, 0, None

        def integrate(self):
            self.k += 1
            self.cm.map_integrate(pose(self.k))

        def plan_update(self):
            P = pose(self.k)
            self.cm.map_plan_update(float(P[0, 3]) + a.goal_ahead, float(P[1, 3]))

        def path(self):
            P = pose(self.k)
            self.cm.map_path(float(P[0, 3]), float(P[1, 3]))

        def evaluate(self):
            P = pose(self.k)
            self.info = self.cm.map_traj_evaluate(float(P[0, 3]), float(P[1, 3]), 0.0, V, W, DT)

    def layers(cm):
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        cm.map_plan_configure(*plan)
        cm.map_traj_configure(*SAMPLES, STEPS, foot, 100, 1, True)

    def summary(cm):
        s, info = cm.map_traj()
        bad = s["bad_step"][s["status"] != capi.TRAJ_VALID]
        return {"statuses": np.bincount(s["status"], minlength=4).tolist(), "best": int(info.best), "n_valid": int(info.n_valid),
                "bad_step_median": float(np.median(bad)) if len(bad) else None,
                "poses_checked": int(np.where(s["status"] == capi.TRAJ_VALID, STEPS, s["bad_step"]).sum())}

    def open_field():
        """A map of the same window without an obstacle (one point far outside, the sensor outside), cost and plan updated."""
        cm = capi.CloudMerger(max_points_total=4096, max_sensors=1, flags=capi.FLAG_PROFILE)
        layers(cm)
        t = (float(a.size) * a.cell + 100.0, 0.0, 0.0)
        cm.submit_all([xyzi_cloud(np.array([[50.0, 0.0, 0.0]], np.float32), np.zeros(1, np.float32), t_xyz=t)])
        assert cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)).status == capi.OK
        cm.map_integrate(None)
        cm.map_cost_update()
        cm.map_plan_update(a.goal_ahead, 0.0)
        return cm

    def open_field_record():
        with open_field() as cm:
            ev = lambda: cm.map_traj_evaluate(0.0, 0.0, 0.0, V, W, DT)
            for _ in range(a.warmup):
                ev()
            meds, stages = [], []
            for _ in range(a.batches):
                t = []
                for _ in range(a.frames):
                    t.append(timed(ev))
                    stages.append(cm.stage_times())
                meds.append(ms(t))
            rec = {"evaluate_ms_batches": meds, "evaluate_ms": round(float(np.median(meds)), 4), "evaluate_ms_spread": round(max(meds) - min(meds), 4),
                   "profile": [(n, round(float(np.median([s[j][1] for s in stages])), 4)) for j, (n, _) in enumerate(stages[-1])]}
            rec.update(summary(cm))
            return rec

    out = {"step": a.step, "lib": a.lib or "shipped", "footprint_points": len(foot), "footprint_lattice": list(foot_n)}
    if a.step == "frame":
        with context() as cm:
            out.update(batches(cm))
    elif a.step == "layers":
        if not a.lib:
            with context() as cm:
                layers(cm)
                c = Calls(cm)
                out.update(batches(cm, [("integrate", c.integrate), ("cost_update", cm.map_cost_update), ("plan_update", c.plan_update), ("path", c.path),
                                        ("traj_evaluate", c.evaluate)]))
                out["cfg2_scene"] = summary(cm)
                out["traj_copy_ms"] = ms([timed(cm.map_traj) for _ in range(10)])
        out["open_field"] = open_field_record()
    elif a.step == "profile":
        with context(capi.FLAG_PROFILE) as cm:
            layers(cm)
            c = Calls(cm)
            stages = []
            for k in range(12):
                frame(cm)
                c.integrate()
                cm.map_cost_update()
                c.plan_update()
                c.evaluate()
                stages.append(cm.stage_times())
            out["profile_cfg2"] = [(n, round(float(np.median([s[j][1] for s in stages[3:]])), 4)) for j, (n, _) in enumerate(stages[-1])]
            out["cfg2_scene"] = summary(cm)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--goal-ahead", type=float, default=40.0)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a GPU step may take")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--build", action="store_true", help="compile the variant libraries and stop")
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--lib", default=None, help="(internal) the variant library of that step")
    a = ap.parse_args()
    if a.build:
        return build_variants()
    if a.step:
        return step(a)

    plan = [("frame", None), ("layers", None), ("profile", None)]
    for name in VARIANTS:
        if os.path.exists(variant_path(name)):
            plan += [("layers", name), ("profile", name)]
    plan.append(("frame", None))
    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; window {a.size} x {a.size} cells of {a.cell} m; "
                                      f"radii 0.35 / 1.05 m, scaling 3; neutral 50, factor 205 / 256, unknown allowed; goal {a.goal_ahead} m ahead; "
                                      f"{SAMPLES[0]} x {SAMPLES[1]} samples, {STEPS} steps of {DT} s, v {V}, w {W}, footprint {FOOT}",
           "frames": a.frames, "batches": a.batches, "steps": []}
    passed = [f"--{k}={getattr(a, k.replace('-', '_'))}" for k in ("frames", "batches", "warmup", "n", "cell", "size", "goal-ahead")]
    for name, lib in plan:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name] + passed + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                 # the first failure ends the job: nothing more is started on the GPU
            out["failed"] = {"step": name, "lib": lib, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
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
