"""Oriented boxes of the clusters restated in numpy, twice (include/cloudmerge.h, "oriented bounding boxes of the clusters").

boxes_vectorised works on a (members, angles) array per cluster, the chunk's sequential sum as np.cumsum along the members;
boxes_loop walks member by member with scalars, as the definition reads. Both take the direction table (what
cm_box_directions returns: the table is the definition, no libm is consulted here) and the cluster tables as inputs, and
return a (n_clusters,) BOX_DTYPE array whose bytes are the answer. Every fp32 / fp64 operation is one numpy operation on
arrays or scalars of that type: rounded on its own, never contracted."""
import numpy as np

F32, F64 = np.float32, np.float64
BOX_DTYPE = np.dtype([("center", "<f4", (3,)), ("size", "<f4", (3,)), ("yaw", "<f4"), ("angle", "<u4"), ("score", "<f8"),
                      ("flags", "<u4"), ("_pad", "<u4")])
MAX_ANGLES, CHUNK, MAX_EXTENT = 180, 256, F32(1.0e6)
AREA, CLOSENESS = 0, 1
VALID = 1
HALF_PI = F64(1.5707963267948966)


def directions_numpy(n):
    """The direction table with numpy's cos / sin: what cm_box_directions is compared with, within 1 ulp."""
    th = np.arange(n, dtype=F64) * (HALF_PI / F64(n))
    return np.stack([np.cos(th).astype(F32), np.sin(th).astype(F32)], axis=1)


def invalid_entry():
    e = np.zeros((), BOX_DTYPE)
    e["center"] = e["size"] = e["yaw"] = F32(np.nan)
    e["score"] = F64(np.nan)
    return e


def is_valid(mn, mx):
    with np.errstate(over="ignore", invalid="ignore"):
        ex, ey, ez = F32(mx[0]) - F32(mn[0]), F32(mx[1]) - F32(mn[1]), F32(mx[2]) - F32(mn[2])
    return bool(np.isfinite(ex) and np.isfinite(ey) and np.isfinite(ez) and ex < MAX_EXTENT and ey < MAX_EXTENT)


def entry(mn, mx, a, ca, sa, u0, u1, v0, v1, score, n_angles):
    """Step 6: the outputs at the chosen angle, in fp32 scalars."""
    mn, mx = [F32(v) for v in mn], [F32(v) for v in mx]
    ca, sa, u0, u1, v0, v1 = F32(ca), F32(sa), F32(u0), F32(u1), F32(v0), F32(v1)
    su, sv, ez = F32(u1 - u0), F32(v1 - v0), F32(mx[2] - mn[2])
    uc, vc = F32(u0 + F32(su * F32(0.5))), F32(v0 + F32(sv * F32(0.5)))
    e = np.zeros((), BOX_DTYPE)
    e["center"] = [F32(mn[0] + F32(F32(uc * ca) - F32(vc * sa))), F32(mn[1] + F32(F32(uc * sa) + F32(vc * ca))),
                   F32(mn[2] + F32(ez * F32(0.5)))]
    e["size"] = [su, sv, ez]
    e["yaw"] = F32(F64(a) * (HALF_PI / F64(n_angles)))
    e["angle"] = a
    e["score"] = F64(score)
    e["flags"] = VALID
    return e


def boxes_vectorised(xyz, table, indices, dirs, criterion=CLOSENESS, d_min=0.01):
    xyz, dirs = np.asarray(xyz, F32), np.asarray(dirs, F32)
    n_angles = len(dirs)
    ca, sa = dirs[None, :, 0], dirs[None, :, 1]
    out = np.zeros(len(table), BOX_DTYPE)
    for k, cl in enumerate(table):
        mn, mx = cl["min"], cl["max"]
        if not is_valid(mn, mx):
            out[k] = invalid_entry()
            continue
        j = indices[int(cl["first"]): int(cl["first"]) + int(cl["n_voxels"])]
        dx, dy = (xyz[j, 0] - mn[0])[:, None], (xyz[j, 1] - mn[1])[:, None]
        u = dx * ca + dy * sa
        v = dy * ca - dx * sa
        assert u.dtype == F32 and v.dtype == F32
        u0, u1, v0, v1 = u.min(axis=0), u.max(axis=0), v.min(axis=0), v.max(axis=0)
        if criterion == AREA:
            score = -((u1 - u0) * (v1 - v0)).astype(F64)
        else:
            d = np.maximum(np.minimum(np.minimum(u1 - u, u - u0), np.minimum(v1 - v, v - v0)), F32(d_min))
            term = F64(1.0) / d.astype(F64)
            score = np.zeros(n_angles, F64)
            for p0 in range(0, len(j), CHUNK):
                score = score + np.cumsum(term[p0:p0 + CHUNK], axis=0)[-1]
        a = int(np.argmax(score))                                   # the first of the largest
        out[k] = entry(mn, mx, a, dirs[a, 0], dirs[a, 1], u0[a], u1[a], v0[a], v1[a], score[a], n_angles)
    return out


def boxes_loop(xyz, table, indices, dirs, criterion=CLOSENESS, d_min=0.01):
    xyz, dirs = np.asarray(xyz, F32), np.asarray(dirs, F32)
    n_angles = len(dirs)
    d_min = F32(d_min)
    out = np.zeros(len(table), BOX_DTYPE)
    for k, cl in enumerate(table):
        mn, mx = cl["min"], cl["max"]
        if not is_valid(mn, mx):
            out[k] = invalid_entry()
            continue
        members = [int(j) for j in indices[int(cl["first"]): int(cl["first"]) + int(cl["n_voxels"])]]
        best = None
        for a in range(n_angles):
            ca, sa = dirs[a, 0], dirs[a, 1]
            uv = []
            for j in members:
                dx, dy = F32(xyz[j, 0] - mn[0]), F32(xyz[j, 1] - mn[1])
                uv.append((F32(F32(dx * ca) + F32(dy * sa)), F32(F32(dy * ca) - F32(dx * sa))))
            u0, u1 = min(u for u, _ in uv), max(u for u, _ in uv)
            v0, v1 = min(v for _, v in uv), max(v for _, v in uv)
            if criterion == AREA:
                score = -F64(F32(F32(u1 - u0) * F32(v1 - v0)))
            else:
                score = F64(0.0)
                for p0 in range(0, len(uv), CHUNK):
                    s = F64(0.0)
                    for u, v in uv[p0:p0 + CHUNK]:
                        d = max(min(min(F32(u1 - u), F32(u - u0)), min(F32(v1 - v), F32(v - v0))), d_min)
                        s = F64(s + F64(1.0) / F64(d))
                    score = F64(score + s)
            if best is None or score > best[0]:                     # strictly: the smallest angle keeps a tie
                best = (score, a, u0, u1, v0, v1)
        score, a, u0, u1, v0, v1 = best
        out[k] = entry(mn, mx, a, dirs[a, 0], dirs[a, 1], u0, u1, v0, v1, score, n_angles)
    return out


def tables_of(xyz, groups):
    """Cluster tables (CLUSTER_DTYPE of tests/cluster_ref.py, indices) for hand-made clusters: groups is a list of index
    lists, each taken in ascending order; the box is the members' own."""
    from tests.cluster_ref import CLUSTER_DTYPE
    xyz = np.asarray(xyz, F32)
    table = np.zeros(len(groups), CLUSTER_DTYPE)
    indices = []
    for k, g in enumerate(groups):
        g = sorted(int(j) for j in g)
        table[k]["first"], table[k]["n_voxels"] = len(indices), len(g)
        table[k]["min"], table[k]["max"] = xyz[g].min(axis=0), xyz[g].max(axis=0)
        indices += g
    return table, np.array(indices, np.uint32)


def heading_error_deg(yaw, truth):
    """Between two headings of a rectangle, which are the same 90 degrees apart."""
    d = (np.degrees(float(yaw)) - np.degrees(float(truth))) % 90.0
    return min(d, 90.0 - d)
