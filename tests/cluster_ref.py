"""Euclidean cluster extraction restated twice (include/cloudmerge.h), independently of each other.

clusters_brute: the O(n^2) fp32 predicate matrix, a plain union-find and plain loops for rules 3-5 (n up to a few thousand).
clusters_tree: scipy's kd-tree in fp64 with an enlarged radius for candidates, the fp32 predicate on the candidates,
scipy.sparse.csgraph.connected_components, then rules 3-5 in numpy (any n).

Both return (labels, clusters, indices): labels (n,) uint32, NONE where the size filter dropped the voxel's component;
clusters (n_clusters,) CLUSTER_DTYPE; indices (n_clustered,) uint32."""
import numpy as np

NONE = 0xFFFFFFFF
CLUSTER_DTYPE = np.dtype([("first", "<u4"), ("n_voxels", "<u4"), ("n_points", "<u4"), ("_pad", "<u4"),
                          ("min", "<f4", (3,)), ("max", "<f4", (3,))])


def tol2_of(tol):
    t = np.float32(tol)
    return np.float32(t * t)


def near(a, b, tol2):
    """The edge predicate on rows of fp32 xyz (broadcasting): (dx*dx + dy*dy) + dz*dz < tol2, every operation rounded to fp32."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz < tol2


def ordered(f):
    """Order-preserving uint32 image of fp32 values (-0 below +0) and back: min / max are taken on the images."""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unordered(o):
    o = np.asarray(o, np.uint32)
    return np.where(o >> 31 != 0, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def clusters_brute(xyz, tol, min_size=1, max_size=NONE, counts=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    adj = near(xyz[:, None, :], xyz[None, :, :], tol2_of(tol))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(adj, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    members = {}
    for i in range(n):                                        # ascending i: a component's list starts with its smallest member
        members.setdefault(find(i), []).append(i)
    labels = np.full(n, NONE, np.uint32)
    table, indices = [], []
    img = ordered(xyz)
    for lst in sorted(members.values(), key=lambda m: m[0]):
        if not (min_size <= len(lst) <= max_size):
            continue
        labels[lst] = len(table)
        e = np.zeros((), CLUSTER_DTYPE)
        e["first"], e["n_voxels"] = len(indices), len(lst)
        e["n_points"] = 0 if counts is None else sum(int(counts[i]) for i in lst) & 0xFFFFFFFF
        e["min"] = unordered(img[lst].min(axis=0))
        e["max"] = unordered(img[lst].max(axis=0))
        table.append(e)
        indices.extend(lst)
    return labels, np.array(table, CLUSTER_DTYPE).reshape(-1), np.array(indices, np.uint32)


def components_tree(xyz, tol):
    """(component number per point, number of components) of the fp32 tolerance graph."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    n = len(xyz)
    finite = np.isfinite(xyz.astype(np.float64)).all() and np.isfinite(np.float64(tol))
    ext = float(np.ptp(xyz.astype(np.float64), axis=0).max()) if n else 0.0
    if not finite or ext > 1e30 or n < 2:
        i, j = np.nonzero(np.triu(near(xyz[:, None, :], xyz[None, :, :], tol2_of(tol)), 1)) if n >= 2 else (np.zeros(0, int),) * 2
    else:
        pairs = cKDTree(xyz.astype(np.float64)).query_pairs(float(np.float32(tol)) * (1.0 + 1e-3), output_type="ndarray")
        ok = near(xyz[pairs[:, 0]], xyz[pairs[:, 1]], tol2_of(tol))
        i, j = pairs[ok, 0], pairs[ok, 1]
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    k, comp = connected_components(g, directed=False)
    return comp, k


def clusters_tree(xyz, tol, min_size=1, max_size=NONE, counts=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    comp, k = components_tree(xyz, tol)
    size = np.bincount(comp, minlength=k)
    smallest = np.full(k, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    kept = (size >= min_size) & (size <= max_size)
    order = np.argsort(smallest, kind="stable")
    order = order[kept[order]]                                # kept components by ascending smallest member
    number = np.full(k, NONE, np.int64)
    number[order] = np.arange(len(order))
    lab = number[comp]
    labels = lab.astype(np.uint32)
    inside = np.nonzero(lab != NONE)[0]
    indices = inside[np.argsort(lab[inside], kind="stable")].astype(np.uint32)
    table = np.zeros(len(order), CLUSTER_DTYPE)
    table["n_voxels"] = size[order]
    table["first"] = np.concatenate([[0], np.cumsum(size[order])[:-1]]) if len(order) else 0
    if counts is not None:
        pts = np.zeros(len(order), np.uint64)
        np.add.at(pts, lab[inside], np.asarray(counts, np.uint64)[inside])
        table["n_points"] = (pts & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    img = ordered(xyz)
    lo = np.full((len(order), 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((len(order), 3), np.uint32)
    np.minimum.at(lo, lab[inside], img[inside])
    np.maximum.at(hi, lab[inside], img[inside])
    table["min"], table["max"] = unordered(lo), unordered(hi)
    return labels, table, indices


def n_components(xyz, tol):
    return components_tree(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), tol)[1]


def same(a, b):
    """Exact equality of two (labels, clusters, indices) triples, the float fields bit for bit."""
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
