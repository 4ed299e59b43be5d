// cm_kernels_motion.hip — ego-motion compensation (deskew) of the sensor clouds before the merge, for gfx950.
//
//   k_motion   one launch over the padded point index space of the frame (a workgroup's 2048 slots lie in one tile,
//              so in one sensor): read the raw point through the loaders of cm_common.hpp (the unaligned generic layout
//              included) and its time field, q = M_s p with the path's own transform (xf_row), then the second-order
//              expansion of exp(dt xi) q for the constant body twist xi = (v, w):
//                  dt = dt0_s + tau,  h = 0.5 (dt dt),  c = w x q,  e = w x c,  k = w x v
//                  out = q + ((dt (c + v)) + (h (e + k)))
//              every operation rounded on its own (no contraction), in this order. Written as 16-byte x,y,z,intensity
//              records at the point's padded index: the frame descriptor is then pointed at them (cm_launch.cpp build_frame),
//              with identity matrices, and every route runs unchanged on the compensated points.  [raw read, 16 B/pt write]
// A non-finite coordinate or time leaves the record non-finite (NaN / inf propagate through every term that holds them):
// the point is dropped downstream exactly as an uncompensated one would be.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"

namespace {

// a x b, componentwise: x = ay bz - az by, y = az bx - ax bz, z = ax by - ay bx
__device__ __forceinline__ void cross_rn(float ax, float ay, float az, float bx, float by, float bz, float& x, float& y, float& z) {
    x = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
    y = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
    z = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
}

__global__ __launch_bounds__(CM_BLOCK) void k_motion(const CmMotionDev md, cm_v4f* __restrict__ out) {
    constexpr uint32_t WG = CM_BLOCK * CM_MOTION_ITEMS;
    const uint32_t first = blockIdx.x * WG;
    // the sensor whose tile-aligned range holds this workgroup (an empty cloud shares its base with the next one: the last
    // sensor that starts at or before `first` is the one)
    uint32_t k = 0;
    for (uint32_t q = 1; q < md.n_sensors; ++q) k += first >= md.s[q].base ? 1u : 0u;
    const CmSensorDev& sd = md.s[k];
    const uint32_t n = sd.n;
    if (first - sd.base >= n) return;                    // padding behind the cloud (or an empty cloud): nothing to write
    const uint32_t i0 = first - sd.base + threadIdx.x;
    const unsigned char* __restrict__ data = sd.data;
    const uint32_t layout = sd.layout, step = sd.point_step;
    const uint32_t ttype = md.time_type[k], toff = md.time_off[k];
    Pt p[CM_MOTION_ITEMS];
    float tau[CM_MOTION_ITEMS];
    // every load issued before the first use; slots past the end of the cloud read its last point and are not written
#pragma unroll
    for (int r = 0; r < CM_MOTION_ITEMS; ++r) {
        const uint32_t i = i0 + r * CM_BLOCK;
        const uint32_t ii = i < n ? i : n - 1;
        p[r] = load_point(data, layout, step, sd.off_x, sd.off_y, sd.off_z, sd.off_i, ii);
        tau[r] = 0.0f;
        if (ttype != CM_DEV_TIME_NONE) {
            cm_gptr q = (cm_gptr)data + static_cast<size_t>(ii) * step + toff;
            if (ttype == CM_DEV_TIME_F32_S) {
                tau[r] = load_f32_unaligned(q);
            } else {
                uint32_t u;
                __builtin_memcpy(&u, (const void*)q, 4);
                tau[r] = __fmul_rn(__uint2float_rn(u), 1e-9f);
            }
        }
    }
    const float* m = sd.m;
    const float dt0 = md.dt0[k];
    const float vx = md.v[0], vy = md.v[1], vz = md.v[2];
    const float wx = md.w[0], wy = md.w[1], wz = md.w[2];
    const float kx = md.k[0], ky = md.k[1], kz = md.k[2];
    cm_v4f* __restrict__ dst = out + sd.base;
#pragma unroll
    for (int r = 0; r < CM_MOTION_ITEMS; ++r) {
        const uint32_t i = i0 + r * CM_BLOCK;
        // (the three rows written out, not xf_point: through the helper this kernel takes 78 VGPRs instead of 70, 6 waves/SIMD for 7)
        const float qx = xf_row(m[0], m[1], m[2], m[3], p[r].x, p[r].y, p[r].z);
        const float qy = xf_row(m[4], m[5], m[6], m[7], p[r].x, p[r].y, p[r].z);
        const float qz = xf_row(m[8], m[9], m[10], m[11], p[r].x, p[r].y, p[r].z);
        const float dt = __fadd_rn(dt0, tau[r]);
        const float h = __fmul_rn(0.5f, __fmul_rn(dt, dt));
        float cx, cy, cz, ex, ey, ez;
        cross_rn(wx, wy, wz, qx, qy, qz, cx, cy, cz);
        cross_rn(wx, wy, wz, cx, cy, cz, ex, ey, ez);
        cm_v4f o;
        o.x = __fadd_rn(qx, __fadd_rn(__fmul_rn(dt, __fadd_rn(cx, vx)), __fmul_rn(h, __fadd_rn(ex, kx))));
        o.y = __fadd_rn(qy, __fadd_rn(__fmul_rn(dt, __fadd_rn(cy, vy)), __fmul_rn(h, __fadd_rn(ey, ky))));
        o.z = __fadd_rn(qz, __fadd_rn(__fmul_rn(dt, __fadd_rn(cz, vz)), __fmul_rn(h, __fadd_rn(ez, kz))));
        o.w = p[r].i;
        if (i < n) dst[i] = o;                            // dwordx4, default cache policy: the next kernel reads it back
    }
}

}  // namespace

void cmk_motion(hipStream_t s, const CmMotionDev& md, void* out, uint32_t n_padded) {
    const uint32_t wg = CM_BLOCK * CM_MOTION_ITEMS;
    if (n_padded) hipLaunchKernelGGL(k_motion, dim3(n_padded / wg), dim3(CM_BLOCK), 0, s, md, reinterpret_cast<cm_v4f*>(out));
}
