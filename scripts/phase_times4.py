"""Where a k4_hist workgroup's time goes (CM_PHASE_TIMING=1 build; cfg2, one frame alone). Thread 0 of every workgroup adds up
the 100 MHz ticks of each phase over its tiles; the timed build waits for a half-tile's loads before it stamps, so "loads
back" is the wait the product build overlaps with the search of the half before."""
import sys, os, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cloud_merger_amd import capi, synth
sensors, params = synth.config2(min_pts=2)
L = capi.load()
buf = (ctypes.c_ulonglong * (16 * 4096))()
with capi.CloudMerger(max_points_total=4_000_000, max_sensors=4, flags=capi.FLAG_PROFILE) as cm:
    for it in range(6):
        cm.submit_all(sensors)
        res = cm.merge_voxelize(params)
        L.cm_debug_phases4(buf, 1)
    assert res.path_flags & capi.PATH_QUANTILE, res.path_flags
    a = np.frombuffer(buf, dtype=np.uint64).reshape(4096, 16).astype(np.float64)
    used = a[:, 15] > 0
    wgs, tiles = int(used.sum()), float(a[:, 15].sum())
    names = ["set-up: tree, clears, first loads issued", "loads back (both halves)", "transform, keys, min/max, next loads issued",
             "search, counters, bucket ids", "reductions + barrier", "counter row + record written"]
    v = a[used, :6].sum(axis=0)
    print(f"workgroups {wgs}, tiles {int(tiles)} ({tiles / wgs:.2f} per workgroup), ticks (10 ns) per workgroup {v.sum() / wgs:.0f}")
    for k, nm in enumerate(names):
        print(f"{nm:46s} {v[k] / wgs:8.0f} ticks per workgroup {v[k] / tiles:8.0f} per tile {100 * v[k] / v.sum():5.1f} %")
    two = a[:, 15] > 1
    if two.any():
        print(f"workgroups with two or more tiles: {int(two.sum())}, ticks per workgroup {a[two, :6].sum() / two.sum():.0f}; "
              f"with one: {a[used & ~two, :6].sum() / max(1, (used & ~two).sum()):.0f}")
    print({n_: round(ms * 1e3, 1) for n_, ms in cm.stage_times()})
