// cm_map_layers.hpp — the tree of layers behind the occupancy map, written once: which layer hangs off which, what a call
// on a layer refuses and in which order, and when a layer's result is stale. No HIP in here: cm_ctx embeds one MapLayers,
// cm_api.cpp asks layer_refusal before every call, cm_byproducts.cpp makes the transitions, and host/layers_tests.cpp drives
// the whole state machine on the CPU. A new layer is a row of LAYER_TABLE.
#pragma once
#include <cstdint>
#include <string>

enum cm_layer : int { LAYER_MAP = 0, LAYER_COST, LAYER_PLAN, LAYER_TRAJ, LAYER_FRONT, LAYER_MATCH, LAYER_SEARCH, LAYER_MCL, LAYER_CAST, LAYER_COUNT };

struct LayerRow {
    int parent;                          // the layer it reads and goes with (a lower number); -1: the map itself
    const char* absent;                  // what a call says while the layer is not configured
    const char* subject;                 // the head of the stale text
    const char* producer;                // the call that makes the result
    const char* configure;               // the call that makes the layer
    const char* failed;                  // the cause after a producer call that failed (the cost layer keeps no such state)
    bool frame_tied;                     // the result is that of the merged frame: a merge since the producer makes it stale
};

inline constexpr LayerRow LAYER_TABLE[LAYER_COUNT] = {
    {-1, "no occupancy map (cm_map_configure first)", nullptr, nullptr, "cm_map_configure", nullptr, false},
    {LAYER_MAP, "no cost layer (cm_map_cost_configure first)", "the cost tables are stale", "cm_map_cost_update", "cm_map_cost_configure", nullptr, false},
    {LAYER_COST, "no plan layer (cm_map_plan_configure first)", "the potential is stale", "cm_map_plan_update", "cm_map_plan_configure",
     "the last cm_map_plan_update failed", false},
    {LAYER_PLAN, "no rollout layer (cm_map_traj_configure first)", "the scores are stale", "cm_map_traj_evaluate", "cm_map_traj_configure",
     "the last cm_map_traj_evaluate failed", false},
    {LAYER_PLAN, "no frontier layer (cm_map_frontier_configure first)", "the frontiers are stale", "cm_map_frontier_update", "cm_map_frontier_configure",
     "the last cm_map_frontier_update failed", false},
    {LAYER_COST, "no matching layer (cm_map_match_configure first)", "the match is stale", "cm_map_match_evaluate", "cm_map_match_configure",
     "the last cm_map_match_evaluate failed", true},
    {LAYER_COST, "no search layer (cm_map_match_search_configure first)", "the search is stale", "cm_map_match_search", "cm_map_match_search_configure",
     "the last cm_map_match_search failed", true},
    {LAYER_COST, "no localisation layer (cm_map_mcl_configure first)", "the weights are stale", "cm_map_mcl_update", "cm_map_mcl_configure",
     "the last cm_map_mcl_update failed", true},
    {LAYER_COST, "no cast layer (cm_map_cast_configure first)", "the rays are stale", "cm_map_cast_evaluate", "cm_map_cast_configure",
     "the last evaluate of the cast layer failed", false},
};

inline constexpr const char* LAYER_IN_FLIGHT = "a frame is in flight (cm_wait first)";
inline constexpr const char* SINCE_INTEGRATE = "the last cm_map_integrate";

struct LayerState {
    bool on = false;                     // the layer is configured
    bool failed = false;                 // the last producer call failed
    const char* since = nullptr;         // what came after the last producer call ("the last cm_map_integrate", the layer's own
                                         // configure call, ...); nullptr and not failed: the result is fresh
    uint64_t serial = 0;                 // frame-tied layers: the frame of the last producer call
    bool fresh() const { return !failed && !since; }
};

struct MapLayers {
    LayerState s[LAYER_COUNT];
    LayerState& operator[](int l) { return s[l]; }
    const LayerState& operator[](int l) const { return s[l]; }
};

// l hangs below node, at any depth.
inline bool layer_below(int l, int node) {
    for (int p = LAYER_TABLE[l].parent; p >= 0; p = LAYER_TABLE[p].parent)
        if (p == node) return true;
    return false;
}

// "<subject>: no <producer> since <since>".
inline std::string layer_stale_text(int l, const char* since) {
    return std::string(LAYER_TABLE[l].subject) + ": no " + LAYER_TABLE[l].producer + " since " + since;
}

// The cost layer's stale text. Its own reads name the configure call while the map holds no frame; the producers of the
// layers behind it always name the last integration.
inline std::string cost_stale_text(bool own_read_of_an_empty_map = false) {
    return layer_stale_text(LAYER_COST, own_read_of_an_empty_map ? LAYER_TABLE[LAYER_COST].configure : SINCE_INTEGRATE);
}

// The first missing layer on the way from the map down to l, or nullptr.
inline const char* layer_absent(const MapLayers& m, int l) {
    if (l < 0) return nullptr;
    if (const char* up = layer_absent(m, LAYER_TABLE[l].parent)) return up;
    return m[l].on ? nullptr : LAYER_TABLE[l].absent;
}

// Why a read of l's result is refused although the layer is there, or the empty string: the producer failed, something
// came after it, or (frame-tied layers) a merge did.
inline std::string layer_stale(const MapLayers& m, uint64_t frame_serial, int l, bool map_has_frames) {
    const LayerState& st = m[l];
    if (l == LAYER_MAP) return std::string();          // (the map accumulates: nothing behind it makes it stale)
    if (l == LAYER_COST) return st.fresh() ? std::string() : cost_stale_text(!map_has_frames);
    if (st.failed) return std::string(LAYER_TABLE[l].subject) + ": " + LAYER_TABLE[l].failed;
    if (st.since) return layer_stale_text(l, st.since);
    if (LAYER_TABLE[l].frame_tied && st.serial != frame_serial) return layer_stale_text(l, "the last merge");
    return std::string();
}

// What a call on layer l refuses before it looks at its own arguments, or the empty string: a frame in flight, a missing
// ancestor (root first), the missing layer, and for a read a stale result.
inline std::string layer_refusal(const MapLayers& m, bool pending, uint64_t frame_serial, int l, bool read, bool map_has_frames) {
    if (pending) return LAYER_IN_FLIGHT;
    if (const char* why = layer_absent(m, l)) return why;
    return read ? layer_stale(m, frame_serial, l, map_has_frames) : std::string();
}

// What l's configure call refuses first: a frame in flight and, unless it only gives the layer back, a missing ancestor.
inline std::string layer_configure_refusal(const MapLayers& m, bool pending, int l, bool gives_back) {
    if (pending) return LAYER_IN_FLIGHT;
    const char* why = gives_back ? nullptr : layer_absent(m, LAYER_TABLE[l].parent);
    return why ? why : std::string();
}

// The transitions. Stale since a cause (which replaces a failure), the producer failed, fresh as of a frame, and a layer
// that is not (or not yet again) configured: off, and stale since its own configure call. (layer_reset also zeroes the
// serial, which the configure calls used to leave alone: nobody can see it, since the stale text stands in front of the
// serial's until the next producer call sets both.)
inline void layer_mark_stale(MapLayers& m, int l, const char* since) {
    m[l].failed = false;
    m[l].since = since;
}
inline void layers_mark_below(MapLayers& m, int node, const char* since) {
    for (int l = 0; l < LAYER_COUNT; ++l)
        if (layer_below(l, node)) layer_mark_stale(m, l, since);
}
inline void layer_mark_failed(MapLayers& m, int l) { m[l].failed = true; }
inline void layer_mark_fresh(MapLayers& m, int l, uint64_t frame_serial) {
    m[l].failed = false;
    m[l].since = nullptr;
    m[l].serial = frame_serial;
}
inline void layer_reset(MapLayers& m, int l) {
    m[l] = LayerState{};
    m[l].since = LAYER_TABLE[l].configure;
}
