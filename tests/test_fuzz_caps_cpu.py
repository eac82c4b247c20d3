"""What the capacity fuzz of the physics sub-step (tests/fuzz_caps.py, tests/test_gpu_fuzz_caps.py) reaches, asserted with the oracle alone: the GPU
comparison cannot pass for want of inputs, and it has no scene to leave out.

The oracle counts in the kernel's units (OracleShipIce.caps_stats, oracle/bp_oracle.c): arbiter lanes needed = arbiters in the cached set right after the
collision phase of a sub-step; velocity slots = the ship, the bodies that move when an env step begins and the bodies of every arbiter cached then or made
during the step; colours = stats()["ncol_max"].  The hub's neighbour count is recomputed in numpy from the oracle's poses after every env step (AABBs grown
by shape radius + skin).  EVERY scene of every family must reach exactly the value it names -- below, at and above the capacity -- and every scene that
make_scenes() serves must be legal in all four counts, also with damping != 0, so the at-capacity GPU tests skip nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_caps as F  # noqa: E402
from benchpush_amd.config import default_cfg, merge_user_cfg, ship_ice_physics_params  # noqa: E402
from oracle import oracle as orc  # noqa: E402

COUNT = {"colours": "ncol_max", "neighbours": "hub_nbr", "lanes": "lanes_max", "slots": "slots_max", "pair_lanes": "lanes_max", "pair_slots": "slots_max"}
DAMPING = 0.5


def measure(scene, radius, actions, damping=0.0):
    """Peaks of one scene over the settle sub-step and STEPS env steps, by a fresh oracle."""
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1, "sim": {"damping": damping}})
    params = F.fuzz_params(ship_ice_physics_params(cfg), radius, F.SUBSTEPS)
    assert (params["damping_pow"] != 0.0) == (damping != 0.0)
    o = orc.OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
    o.reset(scene, observe=False)
    nbr, touched = [], set()
    for t in range(F.STEPS):
        before = o.bodies().copy()
        o.step(float(actions[t]), observe=False)
        touched |= set(np.nonzero((o.bodies() != before).any(axis=1))[0].tolist())
        if "hub" in scene:
            wp, cnt = o.world_polys()
            ab = np.array([[wp[k, : cnt[k]].min(0), wp[k, : cnt[k]].max(0)] for k in range(len(cnt))])
            nbr.append(F.fat_neighbours(ab, scene["hub"], radius))
    out = dict(o.stats())
    out.update(o.caps_stats())
    out.update(hub_nbr=nbr, nb=len(o.bodies()), moved=touched)
    return out


def legal(m):
    return m["ncol_max"] <= 16 and m["lanes_max"] <= 64 and m["slots_max"] <= 96 and (not m["hub_nbr"] or max(m["hub_nbr"]) <= 24)


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("family", list(F.LEGAL))
def test_every_scene_reaches_the_value_it_names(family, radius):
    for maker, targets in ((F.make_scenes, F.LEGAL[family]), (F.make_over_scenes, F.OVER.get(family, ()))):
        if not targets:
            continue
        scenes = maker(family, radius)
        acts = F.actions_for(len(scenes))
        hit = dict.fromkeys(targets, 0)
        for e, sc in enumerate(scenes):
            m = measure(sc, radius, acts[:, e])
            if sc["family"] == "ordinary":
                assert legal(m), (family, e)
                continue
            got = m[COUNT[family]]
            assert (got == [sc["target"]] * F.STEPS) if family == "neighbours" else (got == sc["target"]), (family, radius, e, sc["target"], got)
            hit[sc["target"]] += 1
            if maker is F.make_scenes:
                assert sc["target"] <= F.CAPACITY[family] or family.startswith("pair_")
                assert legal(m), (family, radius, e, m)
                assert legal(measure(sc, radius, acts[:, e], DAMPING)), (family, radius, e, "damping")
                if family.startswith("pair_"):
                    assert max(F.LEGAL[family]) > F.CAPACITY[family] > min(F.LEGAL[family])     # the targets straddle the half-wave limit
            else:
                # over exactly one capacity: the flag a scene raises is the one its family names
                assert sc["target"] > F.CAPACITY[family]
                others = dict(colours=m["ncol_max"] <= 16, neighbours=max(m["hub_nbr"] or [0]) <= 24, lanes=m["lanes_max"] <= 64, slots=m["slots_max"] <= 96)
                assert all(v for k, v in others.items() if k != family), (family, radius, e, m)
        assert min(hit.values()) >= 4, hit


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_damped_counts_of_the_at_capacity_scenes(radius):
    """With damping != 0 bodies keep the velocity a contact gave them, so slots and lanes could be reached sooner: the counts the families name are the same."""
    for family in ("colours", "lanes", "slots"):
        scenes = F.make_scenes(family, radius)
        acts = F.actions_for(len(scenes))
        for e, sc in enumerate(scenes):
            assert measure(sc, radius, acts[:, e], DAMPING)[COUNT[family]] == sc["target"], (family, e)


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_edge_fields_collide_across_the_lane_boundaries(radius):
    """Fields of 63 .. 449 bodies: the bodies the ship moves are exactly the chain at the named indices (which straddle 63|64 and 127|128 where the field is
    large enough), the cold pair at the end of the larger fields holds an arbiter, every batch mixes the largest field with an empty scene."""
    batches = F.make_edge_batches(radius)
    seen = set()
    for cap, scenes in batches.items():
        nbs = [1 + len(s["obstacles"]) for s in scenes]
        assert min(nbs) == 1 and (max(nbs) + 7) // 8 * 8 == cap
        acts = F.actions_for(len(scenes), seed=cap)
        for e, sc in enumerate(scenes):
            m = measure(sc, radius, acts[:, e])
            assert m["nb"] == sc["target"] and legal(m)
            idx = sc["contact_idx"]
            if not idx:
                continue
            seen.add(sc["target"])
            assert m["moved"] - {0} == set(idx), (cap, e, sorted(m["moved"]), idx)          # the whole chain is pushed, nothing else moves
            assert m["lanes_max"] == len(idx) + (1 if sc["tail_idx"] else 0)                # ship x A, the links of the chain, the cold pair
            if sc["target"] >= 65:
                assert 63 in idx and 64 in idx
            if sc["target"] >= 129:
                assert 127 in idx and 128 in idx
            if sc["tail_idx"]:
                assert sc["tail_idx"] == [sc["target"] - 2, sc["target"] - 1]
    assert seen == set(F.EDGE_NB)


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_purge_scenes_fill_the_hub_list_then_stale_it_then_arrive(radius):
    """The conditions under which the list rebuild of the arriving floe must purge the hub's full list (fuzz_caps.purge_scene), from the oracle's poses: the
    hub has exactly 24 fat-AABB neighbours after the settle sub-step, the two bars among them and the arriving floe not; the hub never moves (its list is never
    rebuilt); after the first env step both bars have left their own fat AABBs (their lists were rebuilt) on the side away from the hub by more than the 2 cm
    they reached into the hub's, while the floe is still inside its own; after the third the floe has left its fat AABB through the side that faces the hub,
    by which its new fat AABB meets the hub's."""
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1})
    params = F.fuzz_params(ship_ice_physics_params(cfg), radius, F.SUBSTEPS)
    scenes = F.make_purge_scenes(radius)
    acts = F.actions_for(len(scenes))
    grow = radius + F.SKIN
    for e, sc in enumerate(scenes):
        o = orc.OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
        o.reset(sc, observe=False)

        def aabbs():
            wp, cnt = o.world_polys()
            return np.array([[wp[k, : cnt[k]].min(0), wp[k, : cnt[k]].max(0)] for k in range(len(cnt))])

        def meets(a, b):
            return bool((a[0] <= b[1]).all() and (b[0] <= a[1]).all())

        hub, bars, z = sc["hub"], sc["stale"], sc["arrives"]
        a0 = aabbs()
        fat0 = np.stack([a0[:, 0] - grow, a0[:, 1] + grow], 1)
        assert F.fat_neighbours(a0, hub, radius) == 24 and all(meets(fat0[hub], fat0[x]) for x in bars) and not meets(fat0[hub], fat0[z]), e
        hub0 = o.bodies()[hub].copy()
        for t in range(F.STEPS):
            o.step(float(acts[t, e]), observe=False)
            assert np.array_equal(o.bodies()[hub], hub0), (e, t)
            a = aabbs()
            bb = np.stack([a[:, 0] - radius, a[:, 1] + radius], 1)
            inside = lambda k: bool((bb[k, 0] >= fat0[k, 0]).all() and (bb[k, 1] <= fat0[k, 1]).all())   # noqa: E731
            if t == 0:
                for x in bars:
                    assert not inside(x) and not meets(fat0[hub], np.stack([bb[x, 0] - F.SKIN, bb[x, 1] + F.SKIN])), (e, x)
                assert inside(z), e
        assert bb[z, 0, 0] < fat0[z, 0, 0] and bb[z, 0, 1] >= fat0[z, 0, 1] and bb[z, 1, 1] <= fat0[z, 1, 1], e       # out through the side that faces the hub
        assert meets(fat0[hub], np.stack([bb[z, 0] - F.SKIN, bb[z, 1] + F.SKIN])), e
        m = measure(sc, radius, acts[:, e])
        assert legal(m) and legal(measure(sc, radius, acts[:, e], DAMPING))


def maze_setup(version=1):
    import benchpush_amd.envs.maze_namo as mz
    from benchpush_amd.config import maze_walls
    cfg = mz._maze_cfg({"num_obstacles": F.MAZE_BOXES, "maze_version": version})
    p = dict(mz.maze_physics_params(cfg))
    p.update(settle_steps=1, steps=F.SUBSTEPS, dt=float(p["dt"]) / int(p["steps"]) * F.SUBSTEPS)
    return cfg, p, maze_walls(cfg)


def test_maze_piles_reach_the_lane_capacity():
    """maze-NAMO-v0: every pile layout needs exactly the arbiter lanes it names (62, 63, 64 | 65, 69), all of them from the settle sub-step, and stays inside
    the colour capacity; the pile comes apart while the steps run (fewer active arbiters at the end than lanes at the peak); the ordinary layouts are legal."""
    from oracle.oracle import OracleMaze
    cfg, params, walls = maze_setup()
    assert cfg.obstacle_size == F.MAZE_HALF
    for layouts, targets in ((F.make_maze_layouts(walls), F.MAZE_LEGAL), (F.make_maze_over_layouts(walls), F.MAZE_OVER)):
        acts = F.actions_for(len(layouts), seed=13)
        hit = dict.fromkeys(targets, 0)
        for e, lay in enumerate(layouts):
            o = OracleMaze(params, cfg.robot.vertices, cfg.robot.wheel_vertices, cfg.obstacle_size)
            o.reset(lay, observe=False)
            for t in range(F.STEPS):
                o.step(float(acts[t, e]), observe=False)
            lanes, ncol = o.caps_stats()["lanes_max"], o.stats()["ncol_max"]
            assert ncol <= 16 and np.isfinite(o.shape_states()).all()
            if lay["family"] == "ordinary":
                assert lanes <= 64, (e, lanes)
                continue
            assert lanes == lay["target"], (e, lay["target"], lanes)
            hit[lay["target"]] += 1
        assert min(hit.values()) >= (4 if targets is F.MAZE_LEGAL else 2), hit


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("kind", ["lanes", "slots"])
def test_midstep_scenes_reach_their_count_in_the_first_step(kind, radius):
    """fuzz_caps.midstep_scene: one under the target after the settle sub-step (so the reset's template carries no flag even for the over-capacity scenes), the
    target from the first env step on; for lanes one of them is held by an arbiter that is no longer active (more lanes than active arbiters)."""
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1})
    params = F.fuzz_params(ship_ice_physics_params(cfg), radius, F.SUBSTEPS)
    key = kind + "_max"
    for scenes in (F.make_midstep_scenes(kind, radius), F.make_midstep_over_scenes(kind, radius)):
        acts = F.actions_for(len(scenes))
        for e, sc in enumerate(scenes):
            o = orc.OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
            o.reset(sc, observe=False)
            if sc["family"] == "ordinary":
                continue
            assert o.caps_stats()[key] == sc["target"] - 1, (kind, e, o.caps_stats())
            o.step(float(acts[0, e]), observe=False)
            assert o.caps_stats()[key] == sc["target"], (kind, e, o.caps_stats())
            for t in range(1, F.STEPS):
                o.step(float(acts[t, e]), observe=False)
            c, st = o.caps_stats(), o.stats()
            assert c[key] == sc["target"] and st["ncol_max"] <= 16, (kind, e, c)
            if kind == "lanes":
                assert st["arb_max"] < c["lanes_max"] and c["slots_max"] <= 96
            else:
                assert c["lanes_max"] <= 64


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_pair_leave_scenes_sit_on_the_leave_limits(radius):
    """fuzz_caps.make_pair_leave_scenes: after the settle sub-step exactly 26 lanes (slots <= 34) or exactly 34 slots (lanes <= 26) -- admitted to a pair --;
    with leave=True one more in the first env step, with leave=False never; the ordinary scenes stay far below both."""
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1})
    params = F.fuzz_params(ship_ice_physics_params(cfg), radius, F.SUBSTEPS)
    for leave in (True, False):
        scenes = F.make_pair_leave_scenes(radius, leave)
        acts = F.actions_for(len(scenes))
        for e, sc in enumerate(scenes):
            o = orc.OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
            o.reset(sc, observe=False)
            c0 = o.caps_stats()
            for t in range(F.STEPS):
                o.step(float(acts[t, e]), observe=False)
            c = o.caps_stats()
            if sc["family"] == "ordinary":
                assert c["lanes_max"] <= 20 and c["slots_max"] <= 20, (e, c)
                continue
            key, other, lim, olim = ("lanes_max", "slots_max", F.PAIR_KEYS, F.PAIR_SLOTS) if sc["family"].endswith("lanes") else ("slots_max", "lanes_max", F.PAIR_SLOTS, F.PAIR_KEYS)
            assert c0[key] == lim and c[key] == lim + (1 if leave else 0) and c[other] <= olim, (leave, e, c0, c)
