"""The refusal texts of the occupancy map's layers, byte for byte, through the library (csrc/cm_map_layers.hpp behind
cm_api.cpp and cm_byproducts.cpp): one context, one sensor, an 8 x 8 window, frames of five points, every layer at its smallest
configuration (one rollout sample and one step; n_a = wx = wy = 0; depth 0; 4 particles and 4 beams; 1 pose and 4 bearings).

The walk takes every layer through the causes tests/test_host_layers.py takes the state machine through on the CPU — an absent
ancestor at each depth, the layer's own configure call, an integration, a cost update, a plan update, the localisation layer's
init_pose / predict / init_uniform, a merge, a frame in flight, a load, a layer given back through an ancestor — and compares
the whole cm_last_error text of every read and every device call with a literal, then checks that the reads answer again once
the producer has run. ("The last producer call failed" needs a failing device; that cause is the CPU program's alone.)

The literals are the strings cm_api.cpp and cm_byproducts.cpp carried one by one before the layer table existed: this file,
copied into the tree of the commit before the table, passes there unchanged."""
import numpy as np
import pytest

from cloud_merger_amd import capi
from cloud_merger_amd.types import MergeParams, xyzi_cloud

F32 = np.float32
CELL, N = 0.5, 8
POINTS = np.array([[1.1, 0.2, 0.1], [1.2, -0.6, 0.1], [-0.8, 1.1, 0.1], [0.3, -1.2, 0.2], [1.1, 1.1, 0.3]], F32)
POSE = np.eye(3, 4, dtype=F32)
HERE = (0.1, 0.1)                                    # a world position inside the window: goal, start, pose
PARAMS = MergeParams(leaf=(0.05,) * 3, min_points_per_voxel=1)

IN_FLIGHT = b"a frame is in flight (cm_wait first)"
NO_PARTICLES = b"the particles are not initialised (cm_map_mcl_init_pose or cm_map_mcl_init_uniform first)"
NO_FRAME_IN_MAP = b"the map holds no frame (cm_map_integrate first)"
COST_SINCE_CONFIGURE = b"the cost tables are stale: no cm_map_cost_update since cm_map_cost_configure"
COST_SINCE_INTEGRATE = b"the cost tables are stale: no cm_map_cost_update since the last cm_map_integrate"
LAYERS = ("map", "cost", "plan", "traj", "front", "match", "search", "mcl", "cast")
PARENT = dict(cost="map", plan="cost", traj="plan", front="plan", match="cost", search="cost", mcl="cost", cast="cost")
ABSENT = dict(
    map=b"no occupancy map (cm_map_configure first)",
    cost=b"no cost layer (cm_map_cost_configure first)",
    plan=b"no plan layer (cm_map_plan_configure first)",
    traj=b"no rollout layer (cm_map_traj_configure first)",
    front=b"no frontier layer (cm_map_frontier_configure first)",
    match=b"no matching layer (cm_map_match_configure first)",
    search=b"no search layer (cm_map_match_search_configure first)",
    mcl=b"no localisation layer (cm_map_mcl_configure first)",
    cast=b"no cast layer (cm_map_cast_configure first)")
SINCE_CONFIGURE = dict(
    cost=COST_SINCE_CONFIGURE,
    plan=b"the potential is stale: no cm_map_plan_update since cm_map_plan_configure",
    traj=b"the scores are stale: no cm_map_traj_evaluate since cm_map_traj_configure",
    front=b"the frontiers are stale: no cm_map_frontier_update since cm_map_frontier_configure",
    match=b"the match is stale: no cm_map_match_evaluate since cm_map_match_configure",
    search=b"the search is stale: no cm_map_match_search since cm_map_match_search_configure",
    mcl=b"the weights are stale: no cm_map_mcl_update since cm_map_mcl_configure",
    cast=b"the rays are stale: no cm_map_cast_evaluate since cm_map_cast_configure")
SINCE_INTEGRATE = dict(
    cost=COST_SINCE_INTEGRATE,
    plan=b"the potential is stale: no cm_map_plan_update since the last cm_map_integrate",
    traj=b"the scores are stale: no cm_map_traj_evaluate since the last cm_map_integrate",
    front=b"the frontiers are stale: no cm_map_frontier_update since the last cm_map_integrate",
    match=b"the match is stale: no cm_map_match_evaluate since the last cm_map_integrate",
    search=b"the search is stale: no cm_map_match_search since the last cm_map_integrate",
    mcl=b"the weights are stale: no cm_map_mcl_update since the last cm_map_integrate",
    cast=b"the rays are stale: no cm_map_cast_evaluate since the last cm_map_integrate")
SINCE_LOAD = dict(
    cost=COST_SINCE_INTEGRATE,                       # (the cost layer's own text names the integration after a load as well)
    plan=b"the potential is stale: no cm_map_plan_update since the last cm_map_load",
    traj=b"the scores are stale: no cm_map_traj_evaluate since the last cm_map_load",
    front=b"the frontiers are stale: no cm_map_frontier_update since the last cm_map_load",
    match=b"the match is stale: no cm_map_match_evaluate since the last cm_map_load",
    search=b"the search is stale: no cm_map_match_search since the last cm_map_load",
    mcl=b"the weights are stale: no cm_map_mcl_update since the last cm_map_load",
    cast=b"the rays are stale: no cm_map_cast_evaluate since the last cm_map_load")
SINCE_COST_UPDATE = dict(
    plan=b"the potential is stale: no cm_map_plan_update since the last cm_map_cost_update",
    traj=b"the scores are stale: no cm_map_traj_evaluate since the last cm_map_cost_update",
    front=b"the frontiers are stale: no cm_map_frontier_update since the last cm_map_cost_update",
    match=b"the match is stale: no cm_map_match_evaluate since the last cm_map_cost_update",
    search=b"the search is stale: no cm_map_match_search since the last cm_map_cost_update",
    mcl=b"the weights are stale: no cm_map_mcl_update since the last cm_map_cost_update",
    cast=b"the rays are stale: no cm_map_cast_evaluate since the last cm_map_cost_update")
SINCE_PLAN_UPDATE = dict(
    traj=b"the scores are stale: no cm_map_traj_evaluate since the last cm_map_plan_update",
    front=b"the frontiers are stale: no cm_map_frontier_update since the last cm_map_plan_update")
SINCE_MERGE = dict(
    match=b"the match is stale: no cm_map_match_evaluate since the last merge",
    search=b"the search is stale: no cm_map_match_search since the last merge",
    mcl=b"the weights are stale: no cm_map_mcl_update since the last merge")
MCL_SINCE = dict(
    init_pose=b"the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_init_pose",
    init_uniform=b"the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_init_uniform",
    predict=b"the weights are stale: no cm_map_mcl_update since the last cm_map_mcl_predict")


def below(layer, node):
    while layer in PARENT:
        layer = PARENT[layer]
        if layer == node:
            return True
    return False


class Walk:
    def __init__(self, cm):
        self.cm = cm
        cm.set_transform(0, (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
        # the reads of a layer's result, and the device calls that are no reads (producers first)
        self.reads = dict(
            map=[cm.map, cm.map_device, cm.map_occupancy],
            cost=[cm.map_cost, cm.map_cost_device],
            plan=[cm.map_plan, cm.map_plan_device, lambda: cm.map_path(*HERE)],
            traj=[cm.map_traj, cm.map_traj_device],
            front=[cm.map_frontiers, cm.map_frontier_labels, cm.map_frontier_device],
            match=[cm.map_match_scores, cm.map_match_device],
            search=[cm.map_match_search_result, lambda: cm.map_match_search_level(0)],
            mcl=[cm.map_mcl_weights, cm.map_mcl_device],
            cast=[cm.map_cast_rays, cm.map_cast_device])
        self.calls = dict(
            map=[lambda: cm.map_load(np.zeros((N, N), capi.MAP_DTYPE), (-4, -4))],
            cost=[cm.map_cost_update, cm.map_cost_table],
            plan=[lambda: cm.map_plan_update(*HERE)],
            traj=[lambda: cm.map_traj_evaluate(HERE[0], HERE[1], 0.0)],
            front=[cm.map_frontier_update],
            match=[lambda: cm.map_match(POSE), cm.map_match_table],
            search=[lambda: cm.map_match_search(POSE)],
            mcl=[cm.map_mcl_update, lambda: cm.map_mcl_init_pose(HERE[0], HERE[1], 0.0), cm.map_mcl_init_uniform,
                 lambda: cm.map_mcl_predict(0.0, 0.0, 0.0), cm.map_mcl_particles],
            cast=[lambda: cm.map_cast([(HERE[0], HERE[1], 0.0)]), cm.map_cast_particles])
        self.configure = dict(
            map=lambda: cm.map_configure(CELL, N, N, l_free=-1),
            cost=lambda: cm.map_cost_configure(0.0, 0.5, 1.0),
            plan=lambda: cm.map_plan_configure(),
            traj=lambda: cm.map_traj_configure(nv=1, nw=1, n_steps=1),
            front=lambda: cm.map_frontier_configure(max_frontiers=4),
            match=lambda: cm.map_match_configure(sigma=0.5, max_dist=0.5),
            search=lambda: cm.map_match_search_configure(sigma=0.5, max_dist=0.5, depth=0, max_nodes=16, max_cells=64),
            mcl=lambda: cm.map_mcl_configure(n_particles=4, max_beams=4, range_cells=4, sigma=0.5, max_dist=0.5),
            cast=lambda: cm.map_cast_configure(max_poses=1, n_bearings=4, range_cells=4))

    def frame(self):
        self.cm.submit(0, xyzi_cloud(POINTS, np.ones(len(POINTS), F32)))
        assert self.cm.merge_voxelize(PARAMS).status == capi.OK

    def text(self, call):
        """None where the call answers; the whole error text of a CM_BAD_ARG refusal otherwise."""
        try:
            call()
        except capi.CloudMergeError as e:
            assert e.status == capi.BAD_ARG, e
            return self.cm._lib.cm_last_error(self.cm._ctx)
        return None

    def expect(self, calls, want):
        for k, call in enumerate(calls):
            assert self.text(call) == want, (k, want)

    def reads_say(self, wants):
        """wants: layer -> text; every layer that is not named answers."""
        for layer in LAYERS:
            self.expect(self.reads[layer], wants.get(layer))


@pytest.mark.gpu
def test_every_layer_through_every_cause():
    with capi.CloudMerger(max_points_total=4096, max_sensors=1) as cm:
        w = Walk(cm)
        everything = {layer: w.reads[layer] + w.calls[layer] for layer in LAYERS}
        w.frame()

        # an absent ancestor at each depth, root first: every call of a layer names the first missing layer on its way down
        # from the map, and so does the configure call of a layer whose parent is missing
        configured = []
        for step in LAYERS:
            for layer in LAYERS:
                chain = [layer]
                while chain[-1] in PARENT:
                    chain.append(PARENT[chain[-1]])
                missing = [a for a in reversed(chain) if a not in configured]
                if missing:
                    w.expect(everything[layer], ABSENT[missing[0]])
                    if missing[0] != layer:
                        w.expect([w.configure[layer]], ABSENT[missing[0]])
            if step == "map":
                w.expect([cm.map_integrate], ABSENT["map"])
            w.configure[step]()
            configured.append(step)

        # since its own configure call: the reads refuse, the calls that are no reads do not ask
        # (the localisation layer's reads want particles before they look at the weights)
        w.reads_say({**SINCE_CONFIGURE, "mcl": NO_PARTICLES})
        w.expect([cm.map_cost_table, cm.map_match_table], None)
        w.expect(w.calls["plan"], COST_SINCE_CONFIGURE)
        w.expect(w.calls["traj"] + w.calls["front"], SINCE_CONFIGURE["plan"])
        w.expect(w.calls["match"][:1] + w.calls["search"] + w.calls["mcl"][:1], NO_FRAME_IN_MAP)
        w.expect(w.calls["cast"], COST_SINCE_INTEGRATE)
        w.expect([cm.map_mcl_init_uniform], b"the map holds no frame (cm_map_integrate or cm_map_load first)")
        w.expect([w.calls["mcl"][3], cm.map_mcl_particles], NO_PARTICLES)

        # an integration: everything behind the map, and the producers behind the cost layer name its tables
        w.expect([cm.map_integrate], None)
        w.expect([cm.map_integrate], b"the last frame was already integrated")
        w.reads_say({**SINCE_INTEGRATE, "mcl": NO_PARTICLES})
        w.expect(w.calls["plan"], COST_SINCE_INTEGRATE)
        w.expect(w.calls["match"][:1] + w.calls["search"] + w.calls["mcl"][:1] + w.calls["cast"], COST_SINCE_INTEGRATE)

        # a cost update: the cost layer answers, everything behind it is stale since then
        w.expect([cm.map_cost_update], None)
        w.reads_say({**SINCE_COST_UPDATE, "mcl": NO_PARTICLES})
        w.expect(w.calls["traj"] + w.calls["front"], SINCE_COST_UPDATE["plan"])

        # a plan update: the plan layer answers, the two layers behind it are stale since then; their producers end that
        w.expect(w.calls["plan"], None)
        w.reads_say({**SINCE_COST_UPDATE, "plan": None, **SINCE_PLAN_UPDATE, "mcl": NO_PARTICLES})
        w.expect(w.calls["traj"] + w.calls["front"], None)
        w.reads_say({**{k: SINCE_COST_UPDATE[k] for k in ("match", "search", "cast")}, "mcl": NO_PARTICLES})

        # the three frame-tied layers and the cast layer: each producer ends its own staleness and nobody else's
        w.expect(w.calls["match"][:1], None)
        w.reads_say({**{k: SINCE_COST_UPDATE[k] for k in ("search", "cast")}, "mcl": NO_PARTICLES})
        w.expect(w.calls["search"], None)
        w.reads_say(dict(cast=SINCE_COST_UPDATE["cast"], mcl=NO_PARTICLES))
        w.expect(w.calls["cast"][:1], None)
        w.expect(w.calls["cast"][1:], NO_PARTICLES)
        w.reads_say(dict(mcl=NO_PARTICLES))           # (the particles come before the stale weights)
        w.expect(w.calls["mcl"][:1], NO_PARTICLES)

        # the localisation layer's own causes
        for cause, call in (("init_pose", w.calls["mcl"][1]), ("predict", w.calls["mcl"][3]), ("init_uniform", w.calls["mcl"][2])):
            w.expect([call], None)
            w.reads_say(dict(mcl=MCL_SINCE[cause]))
            w.expect([cm.map_mcl_particles], None)
            w.expect(w.calls["mcl"][:1], None)
            w.reads_say({})
        w.expect(w.calls["cast"][1:], b"n_particles is above max_poses")         # (4 particles, room for 1 pose)
        w.reads_say({})                               # fresh: every read of every layer answers

        # a merge: the three frame-tied layers, and nothing else
        w.frame()
        w.reads_say(SINCE_MERGE)
        # ... and the stale text comes before "since the last merge"
        w.expect([cm.map_integrate], None)
        w.reads_say(SINCE_INTEGRATE)

        # a frame in flight: before any ancestor, for every call and every configure call
        cm.submit(0, xyzi_cloud(POINTS, np.ones(len(POINTS), F32)))
        assert cm.merge_voxelize_async(capi.make_params(PARAMS)) == capi.OK
        for layer in LAYERS:
            w.expect(everything[layer] + [w.configure[layer]], IN_FLIGHT)
        w.expect([cm.map_integrate, lambda: cm.map_configure(None), lambda: cm.map_cost_configure(None)], IN_FLIGHT)
        assert cm.wait().status == capi.OK

        # a load: as an integration, in its own words
        w.expect(w.calls["map"], None)
        w.reads_say(SINCE_LOAD)
        w.expect(w.calls["cast"][:1], COST_SINCE_INTEGRATE)

        # a layer given back through an ancestor: what was below is absent, what is beside stays
        w.expect([lambda: cm.map_plan_configure(None)], None)
        for layer in LAYERS:
            if layer == "plan" or below(layer, "plan"):
                w.expect(everything[layer], ABSENT["plan"])
        w.expect([cm.map_cost_update], None)
        w.expect(w.reads["cost"], None)
        w.expect(w.reads["match"], SINCE_COST_UPDATE["match"])
        w.expect([lambda: cm.map_cost_configure(None)], None)
        for layer in LAYERS[2:]:
            w.expect(everything[layer], ABSENT["cost"])
        w.expect(w.reads["map"], None)
        w.expect([lambda: cm.map_configure(None)], None)
        for layer in LAYERS:
            w.expect(everything[layer], ABSENT["map"])
