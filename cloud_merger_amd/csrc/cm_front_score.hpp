// cm_front_score.hpp — step 6 of the frontier layer (cm_map_frontier_update): the score of a table entry in 64
// bits without a wrap. Plain C++; k_front_best includes it with CM_FRONT_FN set to a device function, and
// tests/test_map_frontier.py builds it with g++ into a stand-alone driver under the sanitizers and compares it with the
// restatement's integers.
//
//   cm_front_score = pot_scale * min_pot - gain_scale * n_cells. Both products fit 64 unsigned bits (each factor is below
//   2^32); the difference is taken on the side where it is not negative, so no intermediate overflows; a value above INT64_MAX
//   is INT64_MAX. A window has at most 2^22 cells, so the library's scores stay above -2^54; for arguments beyond that a value
//   below -INT64_MAX is INT64_MIN.
#pragma once
#include <stdint.h>

#ifndef CM_FRONT_FN
#define CM_FRONT_FN inline
#endif

CM_FRONT_FN int64_t cm_front_score(uint32_t pot_scale, uint32_t gain_scale, uint32_t min_pot, uint32_t n_cells) {
    const uint64_t a = static_cast<uint64_t>(pot_scale) * min_pot;
    const uint64_t b = static_cast<uint64_t>(gain_scale) * n_cells;
    if (a >= b) return a - b > static_cast<uint64_t>(INT64_MAX) ? INT64_MAX : static_cast<int64_t>(a - b);
    return b - a > static_cast<uint64_t>(INT64_MAX) ? INT64_MIN : -static_cast<int64_t>(b - a);
}
