// cm_kernels_map.hip — the rolling log-odds occupancy map accumulated over frames (per-cell log-odds and observation count,
// the three-valued image), for gfx950.
//
// Computed on request after a frame (cm_map_integrate), from the frame's clouds in place exactly as k_ray_mark reads them,
// the caller's pose and the map's previous state; it writes buffers of the map only (the semantics are in
// include/cloudmerge.h). Between the two kernels here runs cm_kernels_rays.hip's k_ray_cast, unchanged, on the E bitmaps.
//
//   k_map_mark    one workgroup per tile of 4096 raw points: k_ray_mark's front end and both masks, then the world cell of
//                 the point under the pose (world_axis is cm_search.hpp's) instead of the grid's cell. A counted point of
//                 descriptor sensor s in window cell c sets bit c of sensor s's E bitmap, and of its H bitmap too when the
//                 point is in A. The H bitmaps lie behind the E bitmaps, n_sensors of each. A word only grows, so the
//                 atomicOr is skipped where a plain read shows the bit.
//   k_map_update  one thread per cell of the new window: the old state at the shifted index ({0, 0} outside the old window),
//                 the evidence from n_pass and the cell's bit of every sensor's E and H word (the 32 cells of a word are 32
//                 neighbouring lanes), the clamped sum into the other state buffer, the image byte. Scroll, update and image
//                 are one pass over 8-byte records.
//
// Every quantity is an integer over sets: which way an atomicOr went cannot show in the bytes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cm_common.hpp"
#include "cm_device.h"
#include "cm_kernels.h"
#include "cm_search.hpp"

namespace {

// bits: 2 * n_sensors bitmaps of `words` words each (E of every sensor, then H of every sensor), zero before the launch.
__global__ __launch_bounds__(CM_BLOCK) void k_map_mark(const CmFrameDev* __restrict__ fd, CmMapDev g,
                                                       const unsigned char* __restrict__ keep,
                                                       const unsigned char* __restrict__ ground,
                                                       uint32_t* __restrict__ bits, uint32_t words, uint32_t n_sensors) {
    const uint32_t tile = blockIdx.x;
    const uint32_t s = sensor_of_tile(fd, tile);
    const CmSensorDev& sd = fd->s[s];
    const uint32_t first = tile * CM_TILE - sd.base;
    uint32_t* map_e = bits + static_cast<size_t>(s) * words;
    uint32_t* map_h = bits + (static_cast<size_t>(n_sensors) + s) * words;
    for (int r = 0; r < CM_ITEMS; ++r) {
        const uint32_t i = first + r * CM_BLOCK + threadIdx.x;
        if (i >= sd.n) continue;
        const Pt p = load_point(sd.data, sd.layout, sd.point_step, sd.off_x, sd.off_y, sd.off_z, sd.off_i, i);
        float x, y, z;
        xf_point(sd.m, p, x, y, z);
        if (!point_valid(x, y, z, fd->crop_enable, fd->crop_min, fd->crop_max)) continue;
        const uint32_t slot = tile * CM_TILE + r * CM_BLOCK + threadIdx.x;
        const bool in_a = !keep || keep[slot];
        const bool in_g = ground && ground[slot];
        if (!in_a && !in_g) continue;
        if (!(g.z_min <= z && z <= g.z_max)) continue;
        int gx, gy;
        if (!world_axis(xf_row(g.p[0], g.p[1], g.p[2], g.p[3], x, y, z), g.inv, &gx) ||
            !world_axis(xf_row(g.p[4], g.p[5], g.p[6], g.p[7], x, y, z), g.inv, &gy)) continue;
        // (|g| < 2^30 and |anchor| < 2^30 + 2^21: the difference needs 33 bits)
        const long long ix = static_cast<long long>(gx) - g.ax, iy = static_cast<long long>(gy) - g.ay;
        if (ix < 0 || ix >= static_cast<long long>(g.nx) || iy < 0 || iy >= static_cast<long long>(g.ny)) continue;
        const uint32_t cell = static_cast<uint32_t>(ix) + static_cast<uint32_t>(iy) * g.nx;
        const uint32_t m = 1u << (cell & 31u);
        uint32_t* w = map_e + (cell >> 5);
        if (!(ld_agent(w) & m)) atomicOr(w, m);
        if (in_a) {
            w = map_h + (cell >> 5);
            if (!(ld_agent(w) & m)) atomicOr(w, m);
        }
    }
}

// prev / next: the two state buffers, nx * ny records of (logodds, n_obs); rays: k_ray_cast's finished (n_pass, n_end);
// bits: k_map_mark's finished bitmaps; image: one byte per cell.
__global__ __launch_bounds__(256) void k_map_update(const uint2* __restrict__ prev, uint2* __restrict__ next,
                                                    const uint32_t* __restrict__ rays, const uint32_t* __restrict__ bits,
                                                    uint32_t words, CmMapUpdateDev u, signed char* __restrict__ image) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= u.nx * u.ny) return;
    const uint32_t ix = c % u.nx, iy = c / u.nx;
    // the cell's place in the old window: the same absolute cell, seen from the old anchor
    const int px = static_cast<int>(ix) + u.sx, py = static_cast<int>(iy) + u.sy;
    uint2 st = make_uint2(0u, 0u);
    if (u.carry && px >= 0 && px < static_cast<int>(u.nx) && py >= 0 && py < static_cast<int>(u.ny))
        st = prev[static_cast<size_t>(px) + static_cast<size_t>(py) * u.nx];
    const uint32_t w = c >> 5, b = c & 31u;
    uint32_t n_hit = 0u, n_ground = 0u;
    for (uint32_t s = 0; s < u.n_sensors; ++s) {
        const uint32_t e = (bits[static_cast<size_t>(s) * words + w] >> b) & 1u;
        const uint32_t h = (bits[(static_cast<size_t>(u.n_sensors) + s) * words + w] >> b) & 1u;
        n_hit += h;
        n_ground += e & ~h;
    }
    const long long n_miss = static_cast<long long>(rays[static_cast<size_t>(c) * 2u]) + n_ground;
    const long long d = n_hit ? static_cast<long long>(u.l_hit) * n_hit : -static_cast<long long>(u.l_miss) * n_miss;
    int logodds = static_cast<int>(st.x);
    uint32_t n_obs = st.y;
    if (d != 0) {
        long long v = static_cast<long long>(logodds) + d;
        v = v < u.l_min ? u.l_min : v;
        v = v > u.l_max ? u.l_max : v;
        logodds = static_cast<int>(v);
        n_obs += n_obs != 0xFFFFFFFFu;
    }
    next[c] = make_uint2(static_cast<uint32_t>(logodds), n_obs);
    signed char v = -1;
    if (n_obs) v = logodds >= u.l_occ ? 100 : logodds <= u.l_free ? 0 : -1;
    image[c] = v;
}

// Step 8 alone, for a state table that was loaded (cm_map_load): k_map_update's last three lines.
__global__ __launch_bounds__(256) void k_map_image(const uint2* __restrict__ state, uint32_t n_cells, int l_free, int l_occ,
                                                   signed char* __restrict__ image) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const uint2 st = state[c];
    const int logodds = static_cast<int>(st.x);
    signed char v = -1;
    if (st.y) v = logodds >= l_occ ? 100 : logodds <= l_free ? 0 : -1;
    image[c] = v;
}

}  // namespace

void cmk_map_image(hipStream_t s, const void* state, uint32_t n_cells, int l_free, int l_occ, void* image) {
    if (n_cells)
        hipLaunchKernelGGL(k_map_image, dim3((n_cells + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint2*>(state), n_cells, l_free, l_occ,
                           reinterpret_cast<signed char*>(image));
}

void cmk_map_mark(hipStream_t s, const CmFrameDev* fd, const CmMapDev& g, const unsigned char* keep, const unsigned char* ground,
                  uint32_t* bits, uint32_t words, uint32_t n_sensors, uint32_t n_tiles) {
    if (n_tiles) hipLaunchKernelGGL(k_map_mark, dim3(n_tiles), dim3(CM_BLOCK), 0, s, fd, g, keep, ground, bits, words, n_sensors);
}

void cmk_map_update(hipStream_t s, const void* prev, void* next, const void* rays, const uint32_t* bits, uint32_t words,
                    const CmMapUpdateDev& u, void* image) {
    const uint32_t n_cells = u.nx * u.ny;
    hipLaunchKernelGGL(k_map_update, dim3((n_cells + 255) / 256), dim3(256), 0, s, reinterpret_cast<const uint2*>(prev),
                       reinterpret_cast<uint2*>(next), reinterpret_cast<const uint32_t*>(rays), bits, words, u,
                       reinterpret_cast<signed char*>(image));
}
