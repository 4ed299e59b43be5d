// layers_tests.cpp — the state machine of the layers behind the occupancy map (csrc/cm_map_layers.hpp) on the CPU: every
// layer through every cause of a refusal, each text compared with a literal. The literals below are the strings the library
// carried one by one before the table existed; none of them is put together by the code under test.
// The "since" phrases handed to layers_mark_below and layer_mark_stale here are this program's own literals: the phrases
// cm_byproducts.cpp hands over at its call sites are held by tests/test_map_layer_texts.py, which compares whole texts on the GPU.
//   layers_tests <tmpdir>
#include "../csrc/cm_map_layers.hpp"
#include "test_support.hpp"

using namespace cloudmerge;

namespace {

const char* const IN_FLIGHT = "a frame is in flight (cm_wait first)";
const char* const ABSENT[LAYER_COUNT] = {
    "no occupancy map (cm_map_configure first)",
    "no cost layer (cm_map_cost_configure first)",
    "no plan layer (cm_map_plan_configure first)",
    "no rollout layer (cm_map_traj_configure first)",
    "no frontier layer (cm_map_frontier_configure first)",
    "no matching layer (cm_map_match_configure first)",
    "no search layer (cm_map_match_search_configure first)",
    "no localisation layer (cm_map_mcl_configure first)",
    "no cast layer (cm_map_cast_configure first)",
};
const char* const SINCE_CONFIGURE[LAYER_COUNT] = {
    nullptr,
    "the cost tables are stale: no cm_map_cost_update since cm_map_cost_configure",
    "the potential is stale: no cm_map_plan_update since cm_map_plan_configure",
    "the scores are stale: no cm_map_traj_evaluate since cm_map_traj_configure",
    "the frontiers are stale: no cm_map_frontier_update since cm_map_frontier_configure",
    "the match is stale: no cm_map_match_evaluate since cm_map_match_configure",
    "the search is stale: no cm_map_match_search since cm_map_match_search_configure",
    "the weights are stale: no cm_map_mcl_update since cm_map_mcl_configure",
    "the rays are stale: no cm_map_cast_evaluate since cm_map_cast_configure",
};
const char* const SINCE_LAST_INTEGRATE[LAYER_COUNT] = {
    nullptr,
    "the cost tables are stale: no cm_map_cost_update since the last cm_map_integrate",
    "the potential is stale: no cm_map_plan_update since the last cm_map_integrate",
    "the scores are stale: no cm_map_traj_evaluate since the last cm_map_integrate",
    "the frontiers are stale: no cm_map_frontier_update since the last cm_map_integrate",
    "the match is stale: no cm_map_match_evaluate since the last cm_map_integrate",
    "the search is stale: no cm_map_match_search since the last cm_map_integrate",
    "the weights are stale: no cm_map_mcl_update since the last cm_map_integrate",
    "the rays are stale: no cm_map_cast_evaluate since the last cm_map_integrate",
};
// (the cost layer's own text names the integration after a load as well)
const char* const SINCE_LOAD[LAYER_COUNT] = {
    nullptr,
    "the cost tables are stale: no cm_map_cost_update since the last cm_map_integrate",
    "the potential is stale: no cm_map_plan_update since the last cm_map_load",
    "the scores are stale: no cm_map_traj_evaluate since the last cm_map_load",
    "the frontiers are stale: no cm_map_frontier_update since the last cm_map_load",
    "the match is stale: no cm_map_match_evaluate since the last cm_map_load",
    "the search is stale: no cm_map_match_search since the last cm_map_load",
    "the weights are stale: no cm_map_mcl_update since the last cm_map_load",
    "the rays are stale: no cm_map_cast_evaluate since the last cm_map_load",
};
const char* const SINCE_COST_UPDATE[LAYER_COUNT] = {
    nullptr,
    nullptr,
    "the potential is stale: no cm_map_plan_update since the last cm_map_cost_update",
    "the scores are stale: no cm_map_traj_evaluate since the last cm_map_cost_update",
    "the frontiers are stale: no cm_map_frontier_update since the last cm_map_cost_update",
    "the match is stale: no cm_map_match_evaluate since the last cm_map_cost_update",
    "the search is stale: no cm_map_match_search since the last cm_map_cost_update",
    "the weights are stale: no cm_map_mcl_update since the last cm_map_cost_update",
    "the rays are stale: no cm_map_cast_evaluate since the last cm_map_cost_update",
};
const char* const SINCE_PLAN_UPDATE[LAYER_COUNT] = {
    nullptr, nullptr, nullptr,
    "the scores are stale: no cm_map_traj_evaluate since the last cm_map_plan_update",
    "the frontiers are stale: no cm_map_frontier_update since the last cm_map_plan_update",
    nullptr, nullptr, nullptr, nullptr,
};
const char* const SINCE_MERGE[LAYER_COUNT] = {
    nullptr, nullptr, nullptr, nullptr, nullptr,
    "the match is stale: no cm_map_match_evaluate since the last merge",
    "the search is stale: no cm_map_match_search since the last merge",
    "the weights are stale: no cm_map_mcl_update since the last merge",
    nullptr,
};
const char* const FAILED[LAYER_COUNT] = {
    nullptr, nullptr,
    "the potential is stale: the last cm_map_plan_update failed",
    "the scores are stale: the last cm_map_traj_evaluate failed",
    "the frontiers are stale: the last cm_map_frontier_update failed",
    "the match is stale: the last cm_map_match_evaluate failed",
    "the search is stale: the last cm_map_match_search failed",
    "the weights are stale: the last cm_map_mcl_update failed",
    "the rays are stale: the last evaluate of the cast layer failed",
};
const char* const MCL_SINCE[3][2] = {
    {"the last cm_map_mcl_init_pose", "the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_init_pose"},
    {"the last cm_map_mcl_init_uniform", "the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_init_uniform"},
    {"the last cm_map_mcl_predict", "the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_predict"},
};
// the tree, stated a second time: who hangs below whom
const int PARENT[LAYER_COUNT] = {-1, LAYER_MAP, LAYER_COST, LAYER_PLAN, LAYER_PLAN, LAYER_COST, LAYER_COST, LAYER_COST, LAYER_COST};

bool below(int l, int node) {
    for (int p = PARENT[l]; p >= 0; p = PARENT[p])
        if (p == node) return true;
    return false;
}

// What the library does around the state: a context's words beside the layers, and the calls that move them.
struct Model {
    MapLayers m;
    bool pending = false, has_frames = false;
    uint64_t frame_serial = 0;
    std::string ask(int l, bool read) const { return layer_refusal(m, pending, frame_serial, l, read, has_frames); }
    void configure(int l) {                 // everything below goes, the layer is there and stale since this call
        for (int k = 0; k < LAYER_COUNT; ++k)
            if (below(k, l)) layer_reset(m, k);
        layer_reset(m, l);
        m[l].on = true;
    }
    void all_on() {
        for (int l = 0; l < LAYER_COUNT; ++l) configure(l);
    }
    void all_fresh() {
        for (int l = 1; l < LAYER_COUNT; ++l) layer_mark_fresh(m, l, frame_serial);
    }
};

#define CHECK_TEXT(got, want) do { const std::string g__ = (got); if (g__ != (want)) { \
    std::printf("FAIL %s:%d: \"%s\" is not \"%s\"\n", __FILE__, __LINE__, g__.c_str(), (want)); ++cloudmerge::failures; } } while (0)

void absent_and_order() {
    // nothing configured: every layer names the map; then one more ancestor at a time, root first
    for (int l = 0; l < LAYER_COUNT; ++l) {
        Model s;
        int chain[LAYER_COUNT], n = 0;
        for (int k = l; k >= 0; k = PARENT[k]) chain[n++] = k;
        for (int d = n; d-- > 0;) {
            for (const bool read : {false, true}) CHECK_TEXT(s.ask(l, read), ABSENT[chain[d]]);
            CHECK_TEXT(layer_configure_refusal(s.m, false, l, false), d > 0 ? ABSENT[chain[d]] : "");
            CHECK_TEXT(layer_configure_refusal(s.m, false, l, true), "");
            s.pending = true;                // in flight before any ancestor
            for (const bool read : {false, true}) CHECK_TEXT(s.ask(l, read), IN_FLIGHT);
            CHECK_TEXT(layer_configure_refusal(s.m, true, l, false), IN_FLIGHT);
            CHECK_TEXT(layer_configure_refusal(s.m, true, l, true), IN_FLIGHT);
            s.pending = false;
            s.configure(chain[d]);
        }
        CHECK_TEXT(s.ask(l, false), "");
    }
    // a missing ancestor in the middle hides what is below it, and a stale text never comes before a missing layer
    Model s;
    s.all_on();
    s.m[LAYER_COST].on = false;
    for (int l = LAYER_PLAN; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), ABSENT[LAYER_COST]);
    s.m[LAYER_COST].on = true;
    s.m[LAYER_PLAN].on = false;
    CHECK_TEXT(s.ask(LAYER_TRAJ, true), ABSENT[LAYER_PLAN]);
    CHECK_TEXT(s.ask(LAYER_FRONT, true), ABSENT[LAYER_PLAN]);
    CHECK_TEXT(s.ask(LAYER_MATCH, false), "");
}

void causes() {
    Model s;
    s.all_on();
    CHECK_TEXT(s.ask(LAYER_MAP, true), "");
    // since its own configure call; a call that is no read does not ask
    for (int l = 1; l < LAYER_COUNT; ++l) {
        CHECK_TEXT(s.ask(l, true), SINCE_CONFIGURE[l]);
        CHECK_TEXT(s.ask(l, false), "");
    }
    // fresh
    s.all_fresh();
    for (int l = 0; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), "");
    // an integration, a load: everything behind the map
    s.has_frames = true;
    layers_mark_below(s.m, LAYER_MAP, "the last cm_map_integrate");
    for (int l = 1; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), SINCE_LAST_INTEGRATE[l]);
    CHECK_TEXT(s.ask(LAYER_MAP, true), "");
    s.all_fresh();
    layers_mark_below(s.m, LAYER_MAP, "the last cm_map_load");
    for (int l = 1; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), SINCE_LOAD[l]);
    // a cost update: the cost layer fresh, everything behind it stale
    s.all_fresh();
    layers_mark_below(s.m, LAYER_COST, "the last cm_map_cost_update");
    CHECK_TEXT(s.ask(LAYER_COST, true), "");
    for (int l = LAYER_PLAN; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), SINCE_COST_UPDATE[l]);
    // a plan update: the two layers behind the plan layer and nothing else
    s.all_fresh();
    layers_mark_below(s.m, LAYER_PLAN, "the last cm_map_plan_update");
    for (int l = 0; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), SINCE_PLAN_UPDATE[l] ? SINCE_PLAN_UPDATE[l] : "");
    // a merge: the three frame-tied layers
    s.all_fresh();
    ++s.frame_serial;
    for (int l = 0; l < LAYER_COUNT; ++l) CHECK_TEXT(s.ask(l, true), SINCE_MERGE[l] ? SINCE_MERGE[l] : "");
    // ... and the stale text comes before "since the last merge"
    layers_mark_below(s.m, LAYER_COST, "the last cm_map_cost_update");
    for (int l = LAYER_MATCH; l <= LAYER_MCL; ++l) CHECK_TEXT(s.ask(l, true), SINCE_COST_UPDATE[l]);
    for (int l = LAYER_MATCH; l <= LAYER_MCL; ++l) {
        layer_mark_failed(s.m, l);
        CHECK_TEXT(s.ask(l, true), FAILED[l]);
        layer_mark_fresh(s.m, l, s.frame_serial);
        CHECK_TEXT(s.ask(l, true), "");
    }
    // the localisation layer's own three causes
    s.all_fresh();
    for (const auto& c : MCL_SINCE) {
        layer_mark_stale(s.m, LAYER_MCL, c[0]);
        CHECK_TEXT(s.ask(LAYER_MCL, true), c[1]);
        for (int l = 0; l < LAYER_COUNT; ++l)
            if (l != LAYER_MCL) CHECK_TEXT(s.ask(l, true), "");
        layer_mark_fresh(s.m, LAYER_MCL, s.frame_serial);
    }
    // the last producer call failed; a cause that comes later replaces the failure; a producer that succeeds ends both
    for (int l = LAYER_PLAN; l < LAYER_COUNT; ++l) {
        s.all_fresh();
        layer_mark_failed(s.m, l);
        for (int k = 0; k < LAYER_COUNT; ++k) CHECK_TEXT(s.ask(k, true), k == l ? FAILED[l] : "");
        CHECK_TEXT(s.ask(l, false), "");
        layers_mark_below(s.m, LAYER_MAP, "the last cm_map_integrate");
        CHECK_TEXT(s.ask(l, true), SINCE_LAST_INTEGRATE[l]);
        layer_mark_failed(s.m, l);
        CHECK_TEXT(s.ask(l, true), FAILED[l]);
        layer_mark_fresh(s.m, l, s.frame_serial);
        CHECK_TEXT(s.ask(l, true), "");
    }
}

void cost_wordings() {
    Model s;
    s.all_on();
    // its own reads: the configure call while the map holds no frame, the last integration afterwards, whatever made it stale
    CHECK_TEXT(s.ask(LAYER_COST, true), "the cost tables are stale: no cm_map_cost_update since cm_map_cost_configure");
    s.has_frames = true;
    CHECK_TEXT(s.ask(LAYER_COST, true), "the cost tables are stale: no cm_map_cost_update since the last cm_map_integrate");
    // the producers behind it: always the last integration
    CHECK_TEXT(cost_stale_text(), "the cost tables are stale: no cm_map_cost_update since the last cm_map_integrate");
    CHECK_TEXT(cost_stale_text(true), "the cost tables are stale: no cm_map_cost_update since cm_map_cost_configure");
}

void marking_touches_the_descendants_only() {
    const char* const cause = "a cause";
    for (int node = 0; node < LAYER_COUNT; ++node) {
        Model s;
        s.all_on();
        s.all_fresh();
        layers_mark_below(s.m, node, cause);
        for (int l = 0; l < LAYER_COUNT; ++l) {
            CHECK(layer_below(l, node) == below(l, node));
            CHECK(s.m[l].on);
            if (l == LAYER_MAP) continue;    // (nothing marks the map: it has no result that goes stale)
            CHECK(s.m[l].fresh() == !below(l, node));
            CHECK(s.m[l].since == (below(l, node) ? cause : nullptr));
        }
    }
    // a configure call: everything below goes, nothing beside or above does
    Model s;
    s.all_on();
    s.all_fresh();
    s.configure(LAYER_PLAN);
    for (int l = 0; l < LAYER_COUNT; ++l) {
        CHECK(s.m[l].on == !below(l, LAYER_PLAN));
        if (l != LAYER_MAP) CHECK(s.m[l].fresh() == (l != LAYER_PLAN && !below(l, LAYER_PLAN)));
    }
    CHECK_TEXT(s.ask(LAYER_PLAN, true), SINCE_CONFIGURE[LAYER_PLAN]);
    CHECK_TEXT(s.ask(LAYER_TRAJ, false), ABSENT[LAYER_TRAJ]);
    CHECK_TEXT(s.ask(LAYER_CAST, true), "");
}

void the_table() {
    for (int l = 0; l < LAYER_COUNT; ++l) {
        CHECK(LAYER_TABLE[l].parent == PARENT[l] && LAYER_TABLE[l].parent < l);
        CHECK(LAYER_TABLE[l].frame_tied == (SINCE_MERGE[l] != nullptr));
        CHECK_TEXT(LAYER_TABLE[l].absent, ABSENT[l]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    return run_tests(argc, argv, [](const char*) {
        the_table();
        absent_and_order();
        causes();
        cost_wordings();
        marking_touches_the_descendants_only();
    }, [] {});
}
