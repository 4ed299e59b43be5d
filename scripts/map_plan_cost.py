#!/usr/bin/env python3
"""Cost of the plan layer behind the cost layer (cm_map_plan_update, cm_map_plan_path) in the workload of
scripts/map_inflate_cost.py: cfg2's frame (4 x 1 M points, random SE(3) per sensor, clouds resident in HBM, 5 cm voxels, min 2
points per voxel), a window of 1000 x 1000 cells of 10 cm, the pose moving 0.37 m per frame, radii 0.35 / 1.05 m, scaling 3,
navfn's 50 / 205 with unknown cells allowed, the goal 40 m ahead of the vehicle, the start at the vehicle cell. One job
measures, in this order:
  - the frame on a context with no layer configured (medians of --batches batches of --frames frames, and their spread): the
    parent's frame, since no kernel of cm_merge_voxelize is touched;
  - the frame on a context with map, cost layer and plan layer, and behind every frame cm_map_integrate, cm_map_cost_update,
    cm_map_plan_update and cm_map_plan_path, each timed on its own (wall clock of the call, which synchronises), with the
    sweeps of every update: integrate and cost update are the yardsticks;
  - the first series again, to show the drift of the job;
  - the per-stage times of one plan update and one path call under CM_FLAG_PROFILE (a context of its own);
  - a maze, once: walls across the whole window every --maze-pitch rows with gaps at alternating ends, the goal at one end and
    the start at the other (the worst case for sweeps over tiles: the path re-enters every tile row by row);
  - the largest square window step 5 of the semantics admits for 50 / 205, without obstacles, the goal in a corner, once.
Prints one JSON line (also appended to --out).

  python scripts/map_plan_cost.py --out profiles/map_plan_cost.txt
"""
import argparse
import json
import math
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
    ap.add_argument("--goal-ahead", type=float, default=40.0)
    ap.add_argument("--maze-pitch", type=int, default=20)
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
    plan = (50, 205, True)

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

    class Calls:
        """The four calls behind a frame; the pose moves with every integration, the goal stays goal_ahead in front of it."""
        def __init__(self, cm):
            self.cm, self.k, self.sweeps, self.cells, self.status = cm, 0, [], [], []

        def integrate(self):
            self.k += 1
            self.cm.map_integrate(pose(self.k))

        def plan_update(self):
            P = pose(self.k)
            self.sweeps.append(int(self.cm.map_plan_update(float(P[0, 3]) + a.goal_ahead, float(P[1, 3])).n_sweeps))

        def path(self):
            P = pose(self.k)
            cells, info = self.cm.map_path(float(P[0, 3]), float(P[1, 3]))
            self.cells.append(int(info.n_cells))
            self.status.append(int(info.status))

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, 5 cm voxels, min 2 points per voxel; window {a.size} x {a.size} cells of "
                                      f"{a.cell} m; radii {radii[0]} / {radii[1]} m, scaling {radii[2]}; neutral {plan[0]}, factor {plan[1]} / 256, "
                                      f"unknown allowed; goal {a.goal_ahead} m ahead", "frames": a.frames, "batches": a.batches}
    with context() as cm:
        out["no_layer"] = batches(cm)
    with context() as cm:
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        cm.map_plan_configure(*plan)
        c = Calls(cm)
        rec = batches(cm, [("integrate", c.integrate), ("cost_update", cm.map_cost_update), ("plan_update", c.plan_update), ("path", c.path)])
        pot, info = cm.map_plan()
        cost, _, info_map = cm.map_cost()
        timed_part = slice(a.warmup, None)
        rec.update(n_frames=c.k, sweeps_median=float(np.median(c.sweeps[timed_part])), sweeps_min=min(c.sweeps[timed_part]),
                   sweeps_max=max(c.sweeps[timed_part]), path_cells_median=float(np.median(c.cells[timed_part])),
                   path_status_counts=np.bincount(c.status[timed_part], minlength=3).tolist(),
                   passable_cells=int(((cost < 253) | (cost == 255)).sum()), reachable_cells=int((pot != capi.PLAN_UNREACHABLE).sum()),
                   largest_pot=int(pot[pot != capi.PLAN_UNREACHABLE].max()))
        # the vehicle stands inside cfg2's cloud (an impassable cell, so its path is empty): the longest path of the same
        # potential, from the reachable cell with the largest value, once
        iy, ix = np.unravel_index(int(np.argmax(np.where(pot == capi.PLAN_UNREACHABLE, 0, pot))), pot.shape)
        far = ((info_map.anchor[0] + ix + 0.5) * a.cell, (info_map.anchor[1] + iy + 0.5) * a.cell)
        cells, pinfo = cm.map_path(*far)
        rec.update(path_far_cells=int(pinfo.n_cells), path_far_status=int(pinfo.status), path_far_ms=ms([timed(lambda: cm.map_path(*far)) for _ in range(10)]))
        out["map_and_plan"] = rec
    with context() as cm:
        out["no_layer_again"] = batches(cm)
    with context(capi.FLAG_PROFILE) as cm:
        cm.map_configure(a.cell, a.size, a.size)
        cm.map_cost_configure(*radii)
        cm.map_plan_configure(*plan)
        c = Calls(cm)
        ups, paths = [], []
        for k in range(8):
            frame(cm)
            c.integrate()
            cm.map_cost_update()
            c.plan_update()
            ups.append(cm.stage_times())
            c.path()
            paths.append(cm.stage_times())
        out["profile_plan_update"] = [(n, round(float(np.median([s[j][1] for s in ups[3:]])), 4)) for j, (n, _) in enumerate(ups[-1])]
        out["profile_plan_path"] = [(n, round(float(np.median([s[j][1] for s in paths[3:]])), 4)) for j, (n, _) in enumerate(paths[-1])]
        out["profile_sweeps"] = c.sweeps[3:]

    def designed(n, cell, cells_xy):
        """A context whose map of n x n cells holds exactly the wanted obstacle cells (one point each, the sensor outside)."""
        cm = capi.CloudMerger(max_points_total=max(4096, len(cells_xy)), max_sensors=1, flags=capi.FLAG_PROFILE)
        cm.map_configure(cell, n, n)
        t = (float(n) * cell + 100.0, 0.0, 0.0)
        xy = np.asarray(cells_xy, np.float64).reshape(-1, 2)
        p = np.stack([(-(n // 2) + xy[:, 0] + 0.5) * cell - t[0], (-(n // 2) + xy[:, 1] + 0.5) * cell, np.zeros(len(xy))], axis=1)
        if len(xy) == 0:
            p = np.array([[50.0, 0.0, 0.0]])
        cm.submit_all([xyzi_cloud(p.astype(np.float32), np.zeros(len(p), np.float32), t_xyz=t)])
        assert cm.merge_voxelize(MergeParams(leaf=(0.5,) * 3, min_points_per_voxel=0)).status == capi.OK
        cm.map_integrate(None)
        assert int((cm.map_occupancy()[0] == 100).sum()) == len(xy)
        return cm

    centre = lambda n, cell, ix, iy: ((-(n // 2) + ix + 0.5) * cell, (-(n // 2) + iy + 0.5) * cell)
    # the maze, once
    n, cell = a.size, a.cell
    walls = [(x, y) for k, y in enumerate(range(a.maze_pitch // 2, n, a.maze_pitch)) for x in (range(0, n - 2) if k % 2 else range(2, n))]
    with designed(n, cell, walls) as cm:
        cm.map_cost_configure(0.0, 0.0, 3.0)
        cm.map_cost_update()
        cm.map_plan_configure(*plan)
        goal, start = centre(n, cell, n // 2, 0), centre(n, cell, n // 2, n - 1)
        info = cm.map_plan_update(*goal)
        t_up = [timed(lambda: cm.map_plan_update(*goal)) for _ in range(3)]
        prof = cm.stage_times()
        cells, pinfo = cm.map_path(*start)
        t_path = [timed(lambda: cm.map_path(*start)) for _ in range(3)]
        out["maze"] = {"window": n, "pitch": a.maze_pitch, "walls": len(walls), "sweeps": int(info.n_sweeps), "plan_update_ms": ms(t_up),
                       "profile_plan_update": [(s, round(t, 4)) for s, t in prof], "path_cells": int(pinfo.n_cells), "path_status": int(pinfo.status),
                       "pot_start": int(pinfo.pot_start), "path_ms": ms(t_path), "profile_plan_path": [(s, round(t, 4)) for s, t in cm.stage_times()]}
    # the largest square window of step 5 for 50 / 205, once
    w_max = plan[0] + ((252 * plan[1]) >> 8)
    n = min(2048, math.isqrt(0xFFFFFFFE // (7 * w_max) + 1))
    with designed(n, 0.05, []) as cm:
        cm.map_cost_configure(0.0, 0.0, 3.0)
        cm.map_cost_update()
        cm.map_plan_configure(*plan)
        goal, start = centre(n, 0.05, 0, 0), centre(n, 0.05, n - 1, n - 1)
        info = cm.map_plan_update(*goal)
        t_up = [timed(lambda: cm.map_plan_update(*goal)) for _ in range(5)]
        prof = cm.stage_times()
        cells, pinfo = cm.map_path(*start)
        t_path = [timed(lambda: cm.map_path(*start)) for _ in range(5)]
        out["largest_window"] = {"window": n, "sweeps": int(info.n_sweeps), "plan_update_ms": ms(t_up), "profile_plan_update": [(s, round(t, 4)) for s, t in prof],
                                 "path_cells": int(pinfo.n_cells), "pot_start": int(pinfo.pot_start), "pot_start_closed_form": 7 * w_max * (n - 1),
                                 "path_ms": ms(t_path), "profile_plan_path": [(s, round(t, 4)) for s, t in cm.stage_times()]}
    r = out["map_and_plan"]
    out["plan_update_ms_over_integrate_ms"] = round(r["plan_update_ms"] / r["integrate_ms"], 4)
    out["plan_update_ms_over_cost_update_ms"] = round(r["plan_update_ms"] / r["cost_update_ms"], 4)
    out["frame_ms_map_and_plan_minus_no_layer"] = round(r["frame_ms"] - out["no_layer"]["frame_ms"], 4)
    out["largest_batch_spread_ms"] = max(out[k]["frame_ms_spread"] for k in ("no_layer", "map_and_plan", "no_layer_again"))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
