#!/usr/bin/env python3
"""Cost of the oriented boxes of the clusters (cm_result_cluster_boxes_device) on the cfg2 shape: 4 x 1 M points, random
SE(3) per sensor, clouds resident in HBM (cm_submit_cloud_device, like bench.py), min 2 points per voxel, at 5 cm and 50 cm
voxels, tolerance = 2 x leaf, 90 headings, one frame at a time. For every leaf: the frame with the call never made (medians
of --batches batches of --frames frames, and their spread), cm_result_clusters_device alone after a frame (the yardstick),
the box call under each criterion (wall clock of the call, which synchronises), and the per-stage times of one call of each
under CM_FLAG_PROFILE (a context of its own) with the share of the k_box_* stages. Then one frame that a single cluster
dominates (a 40 x 40 x 40 block of voxels 0.5 m apart beside 3072 singletons): the call with the library's split between
the one-workgroup fit and the chunk-wise launches in force, and with the split set above the block (CM_BOX_SPLIT), on
contexts of their own. Prints one JSON line (also appended to --out).

  python scripts/box_cost.py --out profiles/box_cost.txt
  python scripts/box_cost.py --frame-only [--tree <checkout>]   # only the frame; --tree: another commit's built checkout
  python scripts/box_cost.py --clusters-only --tree <checkout>  # the frame and cm_result_clusters_device alone: the yardstick
"""
import argparse
import json
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
    ap.add_argument("--angles", type=int, default=90)
    ap.add_argument("--frame-only", action="store_true")
    ap.add_argument("--clusters-only", action="store_true", help="the frame and cm_result_clusters_device alone: runs on a tree without the feature")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    import numpy as np
    import torch                                     # (before the library: torch's HIP runtime serves the process)
    from cloud_merger_amd import capi, synth
    from cloud_merger_amd.types import MergeParams, xyzi_cloud

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

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    ms = lambda v: round(float(np.median(v)) * 1e3, 4)

    def stages(cm):
        st = [(n, round(t, 4)) for n, t in cm.stage_times()]
        box = sum(t for n, t in st if n.startswith("k_box_"))
        return {"stages_ms": st, "k_box_ms": round(box, 4), "all_stages_ms": round(sum(t for _, t in st), 4)}

    out = {"label": a.label, "shape": f"4 x {a.n} pts, 16-B records, min 2 points per voxel, tolerance 2 x leaf, {a.angles} headings",
           "frames": a.frames, "batches": a.batches}
    with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY) as cm:
        for k, s in enumerate(sensors):
            cm.set_transform(k, s.q_xyzw, s.t_xyz)
        for leaf in (0.05, 0.5):
            params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
            tol = 2 * leaf
            rec = {}
            for _ in range(a.warmup):
                frame(cm, params)
            meds = [ms([frame(cm, params)[1] for _ in range(a.frames)]) for _ in range(a.batches)]
            res, _ = frame(cm, params)
            rec.update(n_out=int(res.n_out), path_flags=int(res.path_flags), frame_ms_batches=meds,
                       frame_ms=round(float(np.median(meds)), 4), frame_ms_spread=round(max(meds) - min(meds), 4))
            if a.clusters_only:
                t_cl = []
                for f in range(a.warmup + a.frames):
                    frame(cm, params)
                    dt = timed(lambda: cm.clusters_device(tol))[1]
                    if f >= a.warmup:
                        t_cl.append(dt)
                rec.update(tolerance=tol, clusters_device_ms=ms(t_cl))
            elif not a.frame_only:
                t_cl, t_box = [], {capi.BOX_AREA: [], capi.BOX_CLOSENESS: []}
                for f in range(a.warmup + a.frames):
                    frame(cm, params)
                    (*_, nc, nm), dt = timed(lambda: cm.clusters_device(tol))
                    got = {c: timed(lambda: cm.cluster_boxes_device(tol, n_angles=a.angles, criterion=c))[1] for c in t_box}
                    if f >= a.warmup:
                        t_cl.append(dt)
                        for c in t_box:
                            t_box[c].append(got[c])
                _, table, _ = cm.clusters(tol)
                rec.update(tolerance=tol, n_clusters=int(nc), n_clustered=int(nm), largest=int(table["n_voxels"].max()),
                           above_split=int((table["n_voxels"] > 1024).sum()), clusters_device_ms=ms(t_cl),
                           boxes_area_ms=ms(t_box[capi.BOX_AREA]), boxes_closeness_ms=ms(t_box[capi.BOX_CLOSENESS]))
                rec["area_over_clusters"] = round(rec["boxes_area_ms"] / rec["clusters_device_ms"], 3)
                rec["closeness_over_clusters"] = round(rec["boxes_closeness_ms"] / rec["clusters_device_ms"], 3)
            out[f"leaf_{leaf:g}"] = rec
    if not a.frame_only and not a.clusters_only:
        with capi.CloudMerger(max_points_total=4 * a.n, max_sensors=4, flags=capi.FLAG_OCCUPANCY | capi.FLAG_PROFILE) as cm:
            for k, s in enumerate(sensors):
                cm.set_transform(k, s.q_xyzw, s.t_xyz)
            for leaf in (0.05, 0.5):
                params = MergeParams(leaf=(leaf,) * 3, min_points_per_voxel=2)
                for name, crit in (("area", capi.BOX_AREA), ("closeness", capi.BOX_CLOSENESS)):
                    for _ in range(3):
                        frame(cm, params)
                        cm.cluster_boxes_device(2 * leaf, n_angles=a.angles, criterion=crit)
                    out[f"leaf_{leaf:g}"][f"profile_{name}"] = stages(cm)
                # no cluster above the split (max_size 1000) among more clustered voxels than the split: the three chunk-wise
                # launches are made and every workgroup of theirs leaves at once
                for _ in range(3):
                    frame(cm, params)
                    _, nb = cm.cluster_boxes_device(2 * leaf, 2, 1000, n_angles=a.angles)
                out[f"leaf_{leaf:g}"]["profile_closeness_max_size_1000"] = dict(stages(cm), n_boxes=int(nb))
        # one cluster that holds most of the voxels: tests/test_cluster.py's block
        k = np.arange(40, dtype=np.float32) * np.float32(0.5)
        block = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
        s = np.arange(16, dtype=np.float32) * np.float32(3.0)
        singles = np.stack(np.meshgrid(s + 30, s, s[:12], indexing="ij"), axis=-1).reshape(-1, 3)
        xyz = np.concatenate([block, singles]).astype(np.float32)
        big = {}
        tables = {}
        for name, split in (("split_1024", None), ("split_above_the_block", "100000")):
            os.environ.pop("CM_BOX_SPLIT", None)
            if split:
                os.environ["CM_BOX_SPLIT"] = split
            with capi.CloudMerger(max_points_total=len(xyz), max_sensors=1, flags=capi.FLAG_PROFILE) as cm:
                rec = {}
                for cname, crit in (("area", capi.BOX_AREA), ("closeness", capi.BOX_CLOSENESS)):
                    t = []
                    for f in range(8):
                        cm.submit(0, xyzi_cloud(xyz, np.ones(len(xyz), np.float32)))
                        res = cm.merge_voxelize(MergeParams(leaf=(0.25,) * 3, min_points_per_voxel=1))
                        assert res.status == capi.OK and res.n_out == len(xyz)
                        t.append(timed(lambda: cm.cluster_boxes_device(0.625, n_angles=a.angles, criterion=crit))[1])
                    rec[f"boxes_{cname}_ms"] = ms(t[3:])
                    rec[f"profile_{cname}"] = stages(cm)
                    tables[(name, cname)] = cm.cluster_boxes(0.625, n_angles=a.angles, criterion=crit).tobytes()
                big[name] = rec
            os.environ.pop("CM_BOX_SPLIT", None)
        big["same_bytes_on_both_routes"] = all(tables[("split_1024", c)] == tables[("split_above_the_block", c)] for c in ("area", "closeness"))
        out["block_64000"] = big
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
