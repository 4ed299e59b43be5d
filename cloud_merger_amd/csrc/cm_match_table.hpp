// cm_match_table.hpp — the scan matching layer's field table (cm_map_match_configure, cm_match_table; step 1 of its semantics
// in include/cloudmerge.h): the likelihood byte of a window cell as a function of its squared distance in cells to the nearest
// occupied cell, a Gaussian of the metric distance cut at max_dist, with the exponential of cm_ndt_math.hpp. Plain C++ with no
// HIP, like cm_cost_table.hpp; tests/match_ref.py restates it. Build without contraction (-ffp-contract=off), as the library is.
//
// All three parameters are fp32 values widened to double; every operation below is one IEEE double operation rounded once.
#pragma once
#include <cmath>
#include <cstdint>

#include "cm_ndt_math.hpp"

// What is wrong with the parameters, or nullptr: the refusals that do not need a context. On success
// *R = (uint32_t)ceil(max_dist / cell), the radius of the table in cells.
inline const char* cm_match_refusal(float cell, float sigma, float max_dist, uint32_t max_radius_cells, uint32_t* R) {
    if (!std::isfinite(cell) || !(cell > 0.0f)) return "cell must be finite and > 0";
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return "sigma must be finite and > 0";
    if (!std::isfinite(max_dist) || !(max_dist > 0.0f)) return "max_dist must be finite and > 0";
    const double r = std::ceil(static_cast<double>(max_dist) / static_cast<double>(cell));
    if (!(r <= static_cast<double>(max_radius_cells))) return "max_dist exceeds CM_MATCH_MAX_RADIUS_CELLS cells";
    *R = static_cast<uint32_t>(r);
    return nullptr;
}

// The R * R + 1 entries into lut.
inline void cm_match_table_build(float cell, float sigma, float max_dist, uint32_t R, uint8_t* lut) {
    const double c = cell, sg = sigma, md = max_dist;
    const double two_s2 = (2.0 * sg) * sg;
    lut[0] = 255;
    for (uint32_t d2 = 1; d2 <= R * R; ++d2) {
        const double m = std::sqrt(static_cast<double>(d2)) * c;
        lut[d2] = m > md ? static_cast<uint8_t>(0) : static_cast<uint8_t>(std::floor(255.0 * cm_exp_neg((m * m) / two_s2)));
    }
}
