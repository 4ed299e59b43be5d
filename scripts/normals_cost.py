#!/usr/bin/env python3
"""Cost of the normal estimation (cm_result_normals_device / cm_result_normals) on the cfg2 shape: 4 x 1 M points, random
SE(3) per sensor, clouds resident in HBM (cm_submit_cloud_device, like bench.py), min 2 points per voxel, at 5 cm and 50 cm
voxels, k = 10 and 30, one frame at a time. For every leaf: the frame with the call never made (medians of --batches batches
of --frames frames, and their spread); for every k the device call after a frame (wall clock of the call, which
synchronises), the host call (the table again, then its copy), the per-stage times of one call under CM_FLAG_PROFILE (a
context of its own) with the number of centroids the second search launch took — for the default search cell and two explicit
ones — and for scale the time the host restatement (tests/normals_ref.py: table, the kd-tree one) takes on the same result.
Prints one JSON line (also written to --out).

  python scripts/normals_cost.py --out profiles/normals_cost_cfg2.json
  python scripts/normals_cost.py --frame-only      # only the frame: runs on a tree without the feature, for comparison
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/normals_cost.py --frames 10 --batches 1 --no-host-ref
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000, help="points per sensor")
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams

    sensors, _ = synth.config2(n_per_sensor=a.n, min_pts=2)
    dev = torch.device("cuda", 0)
    clouds = [torch.from_numpy(np.ascontiguousarray(s.data).view(np.uint8).reshape(-1)).to(dev) for s in sensors]
    torch.cuda.synchronize()

    def frame(cm, params):
        t0 = time.perf_counter()
        for k, s in enumerate(sensors):
            cm.submit_device(k, clouds[k].data_ptr(), s.n, 16, 0, 4, 8, 12)
        res = cm.merge_voxelize(params)
        assert res.status == capi.OK
        return res, time.perf_counter() - t0

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)
    out = {"shape": f"4 x {a.n} pts, 16-B records, min 2 points per voxel", "frames": a.frames, "batches": a.batches}
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        for leaf in (0.05, 0.5):
            params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
            rec = {}
            # the frame alone, the call never made on this context so far for this leaf's first batches
            for _ in range(a.warmup):
                frame(cm, params)
            meds = []
            for _ in range(a.batches):
                meds.append(ms([frame(cm, params)[1] for _ in range(a.frames)]))
            res, _ = frame(cm, params)
            rec.update(n_merged=int(res.n_merged), n_out=int(res.n_out), path_flags=int(res.path_flags), frame_ms_batches=meds,
                       frame_ms=round(float(np.median(meds)), 4), frame_ms_spread=round(max(meds) - min(meds), 4))
            for kk in (() if a.frame_only else (10, 30)):
                call, host, after = [], [], []
                table = None
                for f in range(a.warmup + a.frames):
                    res, t_frame = frame(cm, params)
                    t1 = time.perf_counter()
                    cm.normals_device(kk)
                    t2 = time.perf_counter()
                    table = cm.normals(kk)
                    t3 = time.perf_counter()
                    if f >= a.warmup:
                        call.append(t2 - t1); host.append(t3 - t2); after.append(t_frame)
                r = dict(normals_device_ms=ms(call), normals_host_ms=ms(host), frame_ms_between_calls=ms(after),
                         valid=int((table["flags"] == 1).sum()), table_mb=round(table.nbytes / 2 ** 20, 2))
                if not a.no_host_ref:
                    from tests import normals_ref as nr
                    rr = cm.result(res.n_out)
                    xyz = np.stack([rr["x"], rr["y"], rr["z"]], axis=1)
                    t0 = time.perf_counter()
                    want, _ = nr.table(xyz, kk)
                    r["host_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    r["neighbourhoods_equal_to_restatement"] = bool(all(table[f].tobytes() == want[f].tobytes()
                                                                        for f in ("n_neighbors", "r2_k", "last", "flags")))
                rec[f"k_{kk}"] = r
            out[f"leaf_{leaf:g}"] = rec
    if not a.frame_only:
        with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
            for k, s in enumerate(sensors):
                cm.set_transform(k, s.q_xyzw, s.t_xyz)
            for leaf in (0.05, 0.5):
                params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
                for kk in (10, 30):
                    default = leaf * kk ** (1.0 / 3.0)
                    for name, cell in (("default", 0.0), ("half", default / 2), ("double", default * 2)):
                        for _ in range(3):
                            res, _ = frame(cm, params)
                            cm.normals_device(kk, search_cell=cell)
                        st = cm.stage_times()
                        rings = [int(m.group(1)) for m in (re.fullmatch(r"k_nrm_rings n=(\d+)", n) for n, _ in st) if m]
                        out[f"leaf_{leaf:g}"][f"k_{kk}"][f"stages_{name}"] = dict(
                            search_cell=round(cell or default, 4), second_launch=rings[0] if rings else 0,
                            second_launch_share=round((rings[0] if rings else 0) / max(int(res.n_out), 1), 5),
                            call_ms=round(sum(t for _, t in st), 4), stages_ms=[(n, round(t, 4)) for n, t in st])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
