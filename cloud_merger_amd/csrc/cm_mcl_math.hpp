// cm_mcl_math.hpp — the draws of the localisation layer (cm_map_mcl_*, cm_mcl_draws; step 2 of its semantics in
// include/cloudmerge.h): the ground stage's splitmix64 restated (cm_kernels_ground.hip keeps its own copy, so
// that file's code does not move), the draw of a particle and a slot, and the noise integer of a draw. Plain C++ for the host
// (cm_mcl_draws, the resampling offset) and, with CM_MCL_FN set to __device__ __forceinline__, for cm_kernels_mcl.hip: integer
// arithmetic only, the same bits on both sides. tests/mcl_ref.py restates it.
#pragma once
#include <stdint.h>

#ifndef CM_MCL_FN
#define CM_MCL_FN inline
#endif

CM_MCL_FN unsigned long long cm_mcl_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// base of a call: splitmix64(seed + gen), wrapping.
CM_MCL_FN unsigned long long cm_mcl_base(unsigned long long seed, unsigned long long gen) { return cm_mcl_splitmix64(seed + gen); }

// draw(p, i), i < 256.
CM_MCL_FN unsigned long long cm_mcl_draw(unsigned long long base, uint32_t p, uint32_t i) {
    return cm_mcl_splitmix64(base ^ (static_cast<unsigned long long>(p) << 8) ^ static_cast<unsigned long long>(i));
}

// n(u): the sum of the draw's four 16-bit fields minus 131070, in [-131070, 131070]; mean 0, variance (2^32 - 1) / 3.
CM_MCL_FN int32_t cm_mcl_noise(unsigned long long u) {
    return static_cast<int32_t>((u & 0xFFFFull) + ((u >> 16) & 0xFFFFull) + ((u >> 32) & 0xFFFFull) + (u >> 48)) - 131070;
}
