"""What the kernels that read a frame's raw clouds in place see, restated on the host: k_grid_bin, k_ray_mark, k_map_mark,
k_match_mark and k_mcl_mark (and k_merged behind cm_merged_copy) share one front end: the sensor of the tile, load_point with
the sensor's layout, step and offsets, xf_point, point_valid, then the masks. This module is that front end without the
masks, from the SensorClouds as they were submitted: tests/layouts.py's unpack for the loader, tests/motion_ref.py's
transform and valid for the fp32 transform ((m0 x + m1 y) + m2 z) + m3 and the finite-value and crop-box rule, and the matrix
cm_set_sensor_transform makes of q_xyzw and t_xyz. It needs no GPU and no library; tests/test_frame_host.py holds it against
the oracle, bit for bit, on every layout of the catalogue.

The by-product tests take their expected input from here and not from cm.merged(): that comes from k_merged, which shares the
loader with the kernels under test, so a shared mistake would cancel out."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from tests import layouts as wl
from tests import motion_ref as mo

F = np.float32


def matrix_of(q_xyzw, t_xyz):
    """quat_to_rows of cm_api.cpp: the doubles rounded to fp32 first, every product and sum rounded to fp32 on its own."""
    x, y, z, w = (F(v) for v in q_xyzw)
    tx, ty, tz = F(2) * x, F(2) * y, F(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = F(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy, F(t_xyz[0])],
                     [txy + twz, one - (txx + tzz), tyz - twx, F(t_xyz[1])],
                     [txz - twy, tyz + twx, one - (txx + tyy), F(t_xyz[2])]], F)


@dataclass
class Frame:
    A: np.ndarray                     # (n, 4) float32: the fused cloud in (sensor, point) order, bit patterns kept
    sensor: np.ndarray                # (n,) int64: the descriptor sensor of every row of A
    translations: np.ndarray          # (n_sensors, 3) float32: the sensors' translations (the ray origins)
    index: np.ndarray                 # (n,) int64: the row's index in its sensor's cloud
    n_in: int                         # points submitted, valid or not


def moved_points(cloud, motion=None):
    """(n, 4) float32 of one cloud before the validity rule: the transformed points, or with motion = (tau, dt0, v, w) the
    compensated ones (motion_ref.compensate; tau: per-point seconds or None). The intensity's bits pass through."""
    rec = wl.unpack(cloud)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    m = matrix_of(cloud.q_xyzw, cloud.t_xyz)
    out = np.empty((cloud.n, 4), F)
    with np.errstate(all="ignore"):
        if motion is None:
            q = mo.transform(xyz, m)
            for a in range(3):
                out[:, a] = q[a]
        else:
            out[:] = mo.compensate(xyz, m, *motion)
    out[:, 3].view(np.uint32)[:] = rec["intensity"].view(np.uint32)
    return out


def fuse(sensors, crop_min=None, crop_max=None, motions: Optional[list] = None) -> Frame:
    """The frame of `sensors` (one SensorCloud per descriptor sensor, in any layout of tests/layouts.py, empty ones included)
    under the crop box of the merge parameters. motions: per sensor None or moved_points' motion tuple."""
    rows, tags, index = [], [], []
    for s, cloud in enumerate(sensors):
        p = moved_points(cloud, None if motions is None else motions[s])
        ok = mo.valid(p, crop_min, crop_max)
        rows.append(p[ok])
        tags.append(np.full(int(ok.sum()), s, np.int64))
        index.append(np.flatnonzero(ok))
    A = np.concatenate(rows) if rows else np.zeros((0, 4), F)
    trans = np.array([[F(v) for v in c.t_xyz] for c in sensors], F).reshape(len(sensors), 3)
    return Frame(A=A, sensor=np.concatenate(tags) if tags else np.zeros(0, np.int64), translations=trans,
                 index=np.concatenate(index) if index else np.zeros(0, np.int64), n_in=sum(c.n for c in sensors))


def bounds(frame: Frame):
    """(min xyz, max xyz, count) of the frame's points, as cm_local_bounds reports them (+inf / -inf for none)."""
    if not len(frame.A):
        return np.full(3, np.inf, F), np.full(3, -np.inf, F), 0
    return frame.A[:, :3].min(axis=0), frame.A[:, :3].max(axis=0), len(frame.A)
