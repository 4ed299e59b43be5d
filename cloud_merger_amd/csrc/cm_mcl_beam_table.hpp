// cm_mcl_beam_table.hpp — the beam model's table of the localisation layer (cm_map_mcl_beam_configure, cm_mcl_beam_table;
// step 6 of its semantics in include/cloudmerge.h): the byte a ray adds to its particle's score as a function
// of where its first occupied cell lies against the measured end, with the exponential of cm_ndt_math.hpp. Plain C++ with no
// HIP, like cm_match_table.hpp; tests/mcl_beam_ref.py restates it. Build without contraction (-ffp-contract=off), as the
// library is.
//
// Every parameter is an fp32 value widened to double; every operation below is one IEEE double operation rounded once.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/cloudmerge.h"
#include "cm_ndt_math.hpp"

// What is wrong with the parameters, or nullptr: the refusals that do not need a context.
inline const char* cm_mcl_beam_refusal(const cm_mcl_beam_params& q, float cell) {
    if (!std::isfinite(cell) || !(cell > 0.0f)) return "cell must be finite and > 0";
    if (q.over_cells > CM_MCL_BEAM_MAX_OVER) return "over_cells must lie in 0..CM_MCL_BEAM_MAX_OVER";
    if (!std::isfinite(q.sigma) || !(q.sigma > 0.0f)) return "sigma must be finite and > 0";
    if (!std::isfinite(q.z_hit) || !std::isfinite(q.z_short) || !std::isfinite(q.z_rand)) return "z_hit, z_short and z_rand must be finite";
    if (!(q.z_hit > 0.0f)) return "z_hit must be > 0";
    if (!(q.z_short >= 0.0f) || !(q.z_rand >= 0.0f)) return "z_short and z_rand must be >= 0";
    if (!((static_cast<double>(q.z_hit) + static_cast<double>(q.z_short)) + static_cast<double>(q.z_rand) <= 1.0)) return "z_hit + z_short + z_rand must be <= 1";
    if (q.flags & ~CM_MCL_BEAM_PLAIN) return "unknown flag bits";
    return nullptr;
}

// The 2 * over_cells + 3 entries into tab: a hit at e = -E .. E (index e + E), then beyond, then off.
inline void cm_mcl_beam_table_build(const cm_mcl_beam_params& q, float cell, uint8_t* tab) {
    const int E = static_cast<int>(q.over_cells);
    const double sc = static_cast<double>(q.sigma) / static_cast<double>(cell);
    const double two_s2 = (2.0 * sc) * sc;
    const double zh = q.z_hit, zs = q.z_short, zr = q.z_rand;
    for (int e = -E; e <= E; ++e) {
        double v = zh * cm_exp_neg(static_cast<double>(e * e) / two_s2);
        v = v + (e > 0 ? zs : 0.0);
        v = v + zr;
        tab[e + E] = static_cast<uint8_t>(std::rint(255.0 * (v < 1.0 ? v : 1.0)));
    }
    tab[2 * E + 1] = static_cast<uint8_t>(std::rint(255.0 * (zs + zr)));
    tab[2 * E + 2] = static_cast<uint8_t>(std::rint(255.0 * zr));
}
