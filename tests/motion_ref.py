"""numpy restatement of the ego-motion compensation (include/cloudmerge.h, cm_set_ego_motion): fp32, round-to-nearest,
no contraction, every operation in the order the kernel (cm_kernels_motion.hip) does it. numpy evaluates float32 array
expressions one rounded operation at a time, which is exactly that."""
import numpy as np

F = np.float32


def dt0_s(stamp_ns, t_ref_ns):
    """(float)((double)(stamp - t_ref) * 1e-9), the difference taken modulo 2^64 and read as a signed 64-bit integer"""
    d = (int(stamp_ns) - int(t_ref_ns)) & (2 ** 64 - 1)
    return F(float(d - 2 ** 64 if d >= 2 ** 63 else d) * 1e-9)


def valid(pts, crop_min=None, crop_max=None):
    """point_valid of cm_common.hpp as a mask over (n, >= 3) points: every coordinate finite and, with a crop box, no
    coordinate below its minimum or above its maximum."""
    xyz = np.asarray(pts, F)[:, :3]
    ok = np.isfinite(xyz).all(axis=1)
    if crop_min is not None:
        with np.errstate(invalid="ignore"):
            ok &= ~((xyz < np.asarray(crop_min, F)) | (xyz > np.asarray(crop_max, F))).any(axis=1)
    return ok


def cross(a, b):
    """a x b componentwise in fp32 (x = ay bz - az by, ...); a and b: tuples of three scalars or arrays."""
    ax, ay, az = a
    bx, by, bz = b
    return (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)


def transform(xyz, m):
    """The path's transform: ((m0 x + m1 y) + m2 z) + m3 per row, fp32."""
    m = np.asarray(m, F).reshape(3, 4)
    x, y, z = (np.asarray(xyz, F)[:, a] for a in range(3))
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]


def time_of(tau, type_):
    """tau as the kernel reads it: f32 seconds as stored, u32 nanoseconds -> (float)u * 1e-9f, none -> 0."""
    if type_ == 0 or tau is None:
        return None
    if type_ == 1:
        return np.asarray(tau, F)
    return np.asarray(tau, np.uint32).astype(F) * F(1e-9)


def compensate(xyz, m, tau, dt0, v, w, intensity=None):
    """(n,4) float32 x,y,z,intensity: q = M p moved to the reference instant. tau: per-point seconds (float32) or None."""
    q = transform(xyz, m)
    n = len(q[0])
    v = tuple(F(a) for a in v)
    w = tuple(F(a) for a in w)
    k = cross(w, v)
    out = np.empty((n, 4), F)
    with np.errstate(invalid="ignore", over="ignore"):       # (non-finite points stay non-finite, as on the device)
        dt = np.full(n, F(dt0), F) if tau is None else F(dt0) + np.asarray(tau, F)
        h = F(0.5) * (dt * dt)
        c = cross(w, q)
        e = cross(w, c)
        for a in range(3):
            out[:, a] = q[a] + ((dt * (c[a] + v[a])) + (h * (e[a] + k[a])))
    out[:, 3] = 0 if intensity is None else np.asarray(intensity, F)
    return out
