// cm_cost_table.hpp — the cost layer's table (cm_map_cost_configure, step 3 of its semantics in include/cloudmerge.h): the
// inflated cost of a free cell as a function of its squared distance in cells to the nearest obstacle, which is
// costmap_2d::InflationLayer::computeCost with the exponential replaced by cm_ndt_math.hpp's. Plain C++ with no HIP, so that
// the library's host code and a CPU program compute the same bytes; tests/cost_ref.py restates it and tests/test_map_cost.py
// builds it with g++ into a stand-alone driver and compares the two byte for byte. Build without contraction
// (-ffp-contract=off), as the library is.
//
// All four parameters are fp32 values widened to double; every operation below is one IEEE double operation rounded once.
#pragma once
#include <cmath>
#include <cstdint>

#include "cm_ndt_math.hpp"

// What is wrong with the parameters, or nullptr: the refusals of cm_map_cost_configure that do not need a context. On success
// *R = (uint32_t)ceil(inflation_radius / cell), the radius of the table in cells.
inline const char* cm_cost_refusal(float cell, float inscribed_radius, float inflation_radius, float cost_scaling, uint32_t max_radius_cells,
                                   uint32_t* R) {
    if (!std::isfinite(inscribed_radius) || inscribed_radius < 0.0f) return "inscribed_radius must be finite and >= 0";
    if (!std::isfinite(inflation_radius) || inflation_radius < 0.0f) return "inflation_radius must be finite and >= 0";
    if (!std::isfinite(cost_scaling) || cost_scaling < 0.0f) return "cost_scaling must be finite and >= 0";
    if (inflation_radius < inscribed_radius) return "inflation_radius is below inscribed_radius";
    const double r = std::ceil(static_cast<double>(inflation_radius) / static_cast<double>(cell));
    if (!(r <= static_cast<double>(max_radius_cells))) return "the inflation radius exceeds CM_COST_MAX_RADIUS_CELLS cells";
    *R = static_cast<uint32_t>(r);
    return nullptr;
}

// Entry d2 >= 1 of the table.
inline uint8_t cm_cost_entry(uint32_t d2, double cell, double inscribed_radius, double inflation_radius, double cost_scaling) {
    const double m = std::sqrt(static_cast<double>(d2)) * cell;
    if (m <= inscribed_radius) return 253;
    if (m > inflation_radius) return 0;
    return static_cast<uint8_t>(std::floor(252.0 * cm_exp_neg(cost_scaling * (m - inscribed_radius))));
}

// The R * R + 1 entries into lut.
inline void cm_cost_table(float cell, float inscribed_radius, float inflation_radius, float cost_scaling, uint32_t R, uint8_t* lut) {
    const double c = cell, ri = inscribed_radius, ro = inflation_radius, k = cost_scaling;
    lut[0] = 254;
    for (uint32_t d2 = 1; d2 <= R * R; ++d2) lut[d2] = cm_cost_entry(d2, c, ri, ro, k);
}
