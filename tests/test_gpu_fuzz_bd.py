"""Differential fuzz of the fourth copy of the sub-step -- the BP_ENV_BOX instantiation of substep<KIND, DAMP> (csrc/bp_physics.hpp) that csrc/bp_boxdelivery.hpp
drives for box-delivery-v0 and area-clearing-v0 -- against the oracle (oracle/bp_oracle.c driven by oracle/bp_oracle_bd.c), on the scenes of
tests/fuzz_scenes_bd.py: boxes dropped anywhere (on columns, the divider, the corners, each other, the robot, in the receptacle, outside the clearance
boundary), constructed parallel-face / vertex-to-vertex / corner contacts, and the two tasks' own edges.

One env per scene, 3 env steps, STEP_LIMIT lowered to 300 sim steps on both sides (an env step is then about 300 sim steps after the 1000 settle steps
of the reset, and most steps leave through the STEP_LIMIT path).  Bar: `==` after every env step on the info block, reward, terminated, truncated, the
binary64 state of every live shape and the alive mask; the four observation channels byte for byte at reset and after the last step.  The oracle side of
a case is computed once and shared by the kernel variants (default, single pass, second pass, no recurrence shortcut; damping 0.8 has its own).

An env whose in-kernel capacity flags (BP_ERR_*: the neighbour, velocity-slot and arbiter capacities of DESIGN.md "In-kernel capacities" and box-delivery's BP_EVCAP -- unconstrained piles can reach them by design) are set is printed
and left out from that step on; at most 2 % of a case's scenes may go that way.  Nothing else is left out.

A case takes 0.2 - 3 s on the GPU machine (all 28 together 36 s), 1 - 2 s of a default variant the oracle (DESIGN.md "Differential fuzz of the box-delivery / area-clearing step" has the
findings and the one-off sweep of 1000 scenes).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_scenes_bd import CASES, STEPS, STEP_LIMIT, case_setup, oracle_case, oracle_scene, teeth  # noqa: E402,F401


pytestmark = pytest.mark.gpu

# kernel variant -> (environment variables, cfg.sim.damping)
VARIANTS = {
    "default": ({}, 0.0),
    "single pass (BP_BD_BUDGET=0)": ({"BP_BD_BUDGET": "0"}, 0.0),
    "second pass (BP_BD_BUDGET=120)": ({"BP_BD_BUDGET": "120"}, 0.0),
    "no recurrence shortcut (BP_BD_CYCLE=0)": ({"BP_BD_CYCLE": "0"}, 0.0),
    "damping 0.8 (substep<BP_ENV_BOX, DAMP>)": ({}, 0.8),
}
PARAMS = [(c, v) for c in CASES for i, v in enumerate(VARIANTS) if i < 2 or CASES[c][2] == "heading"]   # the cases of one task side by side: one oracle run serves them


_ref_cache = {}


def _reference(case, damping):
    if (case, damping) not in _ref_cache:
        _ref_cache.clear()       # one case at a time: the observations of a case are tens of MB
        cfg, over, scenes, actions, make_oracle = case_setup(case, damping)
        _ref_cache[(case, damping)] = (over, scenes, actions, oracle_case(make_oracle, scenes, actions))
    return _ref_cache[(case, damping)]


def _gpu_run(monkeypatch, task, over, envvars, scenes, actions):
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    for k in ("BP_BD_BUDGET", "BP_BD_CYCLE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    E = len(scenes)
    env = (BatchedBoxDeliveryEnv if task == "bd" else BatchedAreaClearingEnv)(E, cfg=over, trials=scenes, bd_overrides={"step_limit": STEP_LIMIT})
    assert env.bd_params["step_limit"] == STEP_LIMIT
    n = 6 + env.nbox
    obs, _ = env.reset()
    torch.cuda.synchronize()
    out = dict(obs0=obs.cpu().numpy().copy(), flags=[env.error_flags().copy()], steps=[])
    for t in range(STEPS):
        obs, rew, term, trunc, info = env.step(torch.from_numpy(np.ascontiguousarray(actions[t])))
        torch.cuda.synchronize()
        alive, _, _ = env.box_state()
        out["steps"].append((info.cpu().numpy().copy(), rew.cpu().numpy().copy(), term.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool),
                             env.body_state().cpu().numpy()[:, :n].copy(), alive[:, : env.nbox].astype(bool)))
        out["flags"].append(env.error_flags().copy())
    out["obs"] = obs.cpu().numpy().copy()
    out["resumed"], out["limited"] = env.stragglers()
    env.close()
    return out


def compare(case, variant, scenes, ref, got, only=None):
    """The bar.  Raises on the first scene that differs, naming case, kernel variant, scene, family, step and the shapes; returns the scenes left out."""
    E = len(scenes)
    left_out = {}
    for e in (range(E) if only is None else only):
        who = "%s, %s: scene %d (family %d)" % (case, variant, e, scenes[e]["fuzz"]["family"])
        r = ref[e]
        if got["flags"][0][e]:
            left_out[e] = (-1, int(got["flags"][0][e]))
        elif not np.array_equal(got["obs0"][e], r["obs0"]):
            raise AssertionError("%s, reset: the observation differs from the oracle in channels %s" % (who, np.nonzero((got["obs0"][e] != r["obs0"]).any(axis=(0, 1)))[0].tolist()))
        for t in range(STEPS):
            if e in left_out:
                break
            if got["flags"][t + 1][e]:
                left_out[e] = (t, int(got["flags"][t + 1][e]))
                break
            ginfo, grew, gterm, gtrunc, gst, galive = (x[e] for x in got["steps"][t])
            oinfo, orew, oterm, otrunc, ost, oalive = r["steps"][t]
            if not np.array_equal(galive, oalive):
                raise AssertionError("%s, step %d: the alive mask differs from the oracle for boxes %s" % (who, t, np.nonzero(galive != oalive)[0].tolist()))
            live = np.ones(len(ost), bool)
            live[6:] = oalive
            if not np.array_equal(gst[live], ost[live]):
                bad = np.nonzero(live & (gst != ost).any(axis=1))[0]
                raise AssertionError("%s, step %d: shape state differs from the oracle for shapes %s" % (who, t, bad.tolist()))
            if not np.array_equal(ginfo, oinfo):
                raise AssertionError("%s, step %d: the info block differs from the oracle in entries %s" % (who, t, np.nonzero(ginfo != oinfo)[0].tolist()))
            if not (grew == orew and bool(gterm) == oterm and bool(gtrunc) == otrunc):
                raise AssertionError("%s, step %d: reward / terminated / truncated differ from the oracle: %r vs %r" % (who, t, (grew, gterm, gtrunc), (orew, oterm, otrunc)))
        if e not in left_out and not np.array_equal(got["obs"][e], r["obs"]):
            raise AssertionError("%s, step %d: the observation differs from the oracle in channels %s" % (who, STEPS - 1, np.nonzero((got["obs"][e] != r["obs"]).any(axis=(0, 1)))[0].tolist()))
    return left_out


@pytest.mark.parametrize("case,variant", PARAMS, ids=["%s-%s" % (c, v.split(" (")[0].replace(" ", "_")) for c, v in PARAMS])
def test_differential_fuzz_box_step_vs_oracle(monkeypatch, case, variant):
    task, floors = CASES[case][0], CASES[case][5]
    envvars, damping = VARIANTS[variant]
    over, scenes, actions, ref = _reference(case, damping)
    E = len(scenes)
    assert sorted({s["fuzz"]["family"] for s in scenes}) == [0, 1, 2, 3]
    if variant == "default":
        seen = teeth(task, ref)
        print("%s: oracle records %s; peak active arbiters %d, peak colours %d" % (case, seen, max(r["stats"]["arb_max"] for r in ref), max(r["stats"]["ncol_max"] for r in ref)))
        scale = E / CASES[case][3]
        for k, floor in floors.items():
            assert seen[k] >= floor * scale, (case, "the scenes no longer collide as they did", k, seen, floors)
    got = _gpu_run(monkeypatch, task, over, envvars, scenes, actions)
    left_out = compare(case, variant, scenes, ref, got)
    for e, (t, bits) in sorted(left_out.items()):
        print("%s, %s: scene %d (family %d) left out from %s on: capacity flags 0x%x; oracle peaks: %d active arbiters, %d colours"
              % (case, variant, e, scenes[e]["fuzz"]["family"], "the reset" if t < 0 else "step %d" % t, bits, ref[e]["stats"]["arb_max"], ref[e]["stats"]["ncol_max"]))
    assert len(left_out) <= 0.02 * E, (case, variant, "more than 2 % of the scenes ran into an in-kernel capacity", sorted(left_out))
    if "BP_BD_BUDGET" in envvars:
        # a heading step drives 1.5 - 1.75 m at 0.2 - 0.3 m/s: thousands of 2 ms sim steps, cut by STEP_LIMIT at 300 -- every env step whose robot has a
        # path at all passes a budget of 120 unfinished
        assert got["resumed"] == 0 if envvars["BP_BD_BUDGET"] == "0" else got["resumed"] >= E * STEPS // 2, (variant, got["resumed"])


# Scenes that the fuzz found, kept by name: (case, seed, scenes in the batch, scene index).
REGRESSIONS = [
    # The robot starts on the middle column.  The (1,3) pre_solve of the 1000 settle sub-steps moves it off and leaves robot_hit_obstacle set: the reference
    # clears the flag before the settle (area_clearing.py:305,407) and again only at the end of a step (:776), so execute_robot_path of the FIRST step gives
    # up as soon as the robot has moved 0.05 m (231 sim steps in the oracle).  The handle cleared the flag in reset() and drove on (401).  Fixed: the settle
    # kernel hands the flag to reset().
    pytest.param("ac-walled_env_with_columns-position", 22000, 96, 4, id="robot_starts_on_a_column"),
    # Boxes 0, 8 and 9 start as a pile between a wall segment and the outer wall.  In the last sub-step of an env step the (2,3) pre_solve pushes box 9,
    # which has no velocity of any kind, 6.5e-6 m off the wall segment.  Inside a launch substep() re-lists such a box for the next sub-step; the next
    # LAUNCH rebuilt its moving list from the velocities alone, box 9 kept the world vertices of its pose before the push-out, and its contact with box 0
    # came out 3.7e-6 m deeper than the oracle's (bias velocities off in the 4th digit, positions 3e-9 m after three steps).  Fixed in load_state_b.
    pytest.param("ac-walled_env-heading", 24000, 96, 54, id="pile_against_the_outer_wall"),
    # Family 0, a draw that the reference's own generate_boxes accepts (it does not look at corners): box 9 starts at (4.751, -2.217), on the corner
    # triangles, and prevent_boundary_intersection throws it through the wall to x = 5.276 during the settle, in the oracle as on the device.
    pytest.param("bd-small_columns-heading", 11000, 1000, 128, id="box_thrown_through_the_corner"),
    # Two scenes of a one-off sweep (bd-large_divider-heading, 500 scenes): a box is delivered at the end of env step 0 after a (2,3) push-out off the wall
    # behind the receptacle in that step's last sub-step.  The stale-vertex test of load_state_b (the fix of the scene above) then listed the REMOVED box
    # at the next launch, the integrate phase gave it an AABB again, and it pushed its neighbours (first difference in sim step 1 of env step 1, the
    # removed shape among the ones that moved).  Fixed: a parked box (empty AABB) is never listed.
    pytest.param("bd-large_divider-heading", 12100, 500, 115, id="delivered_box_after_a_push_out_115"),
    pytest.param("bd-large_divider-heading", 12100, 500, 332, id="delivered_box_after_a_push_out_332"),
]


@pytest.mark.parametrize("case,seed,n,index", REGRESSIONS)
def test_regression_scene_vs_oracle(monkeypatch, case, seed, n, index):
    task = CASES[case][0]
    cfg, over, scenes, actions, make_oracle = case_setup(case, nscenes=n, seed=seed)
    scenes, actions = scenes[index: index + 1], np.ascontiguousarray(actions[:, index: index + 1])
    ref = oracle_case(make_oracle, scenes, actions)
    got = _gpu_run(monkeypatch, task, over, {}, scenes, actions)
    assert not compare(case, "default, seed %d scene %d alone" % (seed, index), scenes, ref, got)
