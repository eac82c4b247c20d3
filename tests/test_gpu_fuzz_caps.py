"""The physics sub-step at its fixed in-kernel capacities and at the lane / stride edges of its per-body loops (-m gpu): the constructed scenes of
tests/fuzz_caps.py against oracle/bp_oracle.c.  tests/test_fuzz_caps_cpu.py shows with the oracle alone that every scene reaches the value it names and that
every at-capacity scene is legal, so nothing is left out here.  DESIGN.md "In-kernel capacities" is the audit these tests stand on.

At or below a capacity the bar is that of tests/test_gpu_fuzz.py: `==` on the binary64 state of every shape, reward, termination and the info block after
each of 3 env steps, no capacity flag, for its four KERNELS (whose pairing mode is asserted, so a variant cannot fall back silently) and for the
damping != 0 instantiation against a damped oracle.  One documented exception: BP_PAIR=1 pairs envs for the whole step (the parity-test kernel, no way out of
the pair), so an env that needs more than the half-wave's 32 arbiter lanes or 40 velocity slots raises BP_ERR_ARB_OVERFLOW there, as DESIGN.md section 4p
says (and at most BP_ERR_LEVEL_OVERFLOW beside it, which follows when bodies share the last slot).  That kernel is therefore not run on the `lanes`, `slots`
and mid-step families, whose every scene is beyond the half-wave: "zero scenes left out" holds for the other four kernels.  On the pair_* families it must
equal the oracle without a flag up to exactly 32 lanes / 40 slots (asserted to happen) and carry the bit beyond, and every other env, its mate included, must
equal the oracle.  Inside the scheduler (BP_PAIR=2) the pair_* scenes hold their counts from the settle sub-step, above the leave limits of 26 lanes / 34
slots: they are declined at load and run alone -- equal, no flag.  The leave in the middle of a step has a test of its own, with scenes that sit on those
limits and pass them in the first env step.

The -DBP_PROF twin then shows that the device itself counted to the capacity: peaks of occupied arbiter lanes, velocity slots, neighbours found by a list
rebuild and colours asked for equal the scene's target (so: the capacity on the "exactly at" scenes, less below).

Above a capacity: BpError from check_errors(), exactly the documented bit in exactly the over-capacity envs, every ordinary env of the batch still == the
oracle in state, reward, info and observation bytes, the over-capacity env finite with its body count unchanged, and the flag after reset(mask) as documented
(sticky; a reset adds what the new trial's template raised while it settled).  Those scenes are over the capacity from the settle sub-step on, so the bit is
in the template before a step kernel runs: they show isolation and finiteness, not which kernel raised the bit.  The mid-step scenes (lanes, slots) are legal
after the settle sub-step and pass the capacity in the first env step: there the step kernel named by the variant raises it (arbiters_take, slot_get).  No
scene passes the colour or the neighbour capacity only in the middle of a step.

maze-NAMO-v0 runs the lane capacity once through substep<BP_ENV_MAZE>: piles of overlapping boxes at 62, 63, 64 | 65, 69 arbiters."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_caps as F  # noqa: E402
from test_gpu_bias_lanes import prof_twin  # noqa: E402,F401  (the -DBP_PROF twin for the duration of a test)
from test_gpu_fuzz import KERNELS  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, SUBSTEPS = F.STEPS, F.SUBSTEPS
DAMPING = 0.5
ADJ, ARB, LEVEL = 1, 2, 4                                  # BP_ERR_ADJ_OVERFLOW, BP_ERR_ARB_OVERFLOW, BP_ERR_LEVEL_OVERFLOW (include/benchpush_amd.h)
BIT = {"colours": LEVEL, "neighbours": ADJ, "lanes": ARB, "slots": ARB}
SWITCHES = ("BP_PAIR", "BP_SCHED", "BP_SCHED_PERSIST", "BP_SCHED_IMAGE", "BP_SCHED_YMASK", "BP_BIAS_LANES", "BP_PAIR_SOLO", "BP_PP_ACT", "BP_PP_WORK", "BP_PP_RATE",
            "BP_PP_KEYS", "BP_PP_SLOTS", "BP_PP_MV")
DAMPED = ("damping != 0 (substep<KIND, DAMP = true>)", {"BP_PAIR": "0"})
P_LANES, P_ACTIVE, P_SLOTS, P_MOVING, P_CAPS = 11, 12, 14, 15, 22      # counters of the -DBP_PROF twin (bp_physics.hpp)
PP_LANES, PP_SLOTS, PP_NBCAP = 32, 40, 448                 # the half-wave's capacities (bp_physics_pair.hpp)

_REF = {}


def _plain(scenes):
    return [{k: s[k] for k in ("ship_state", "goal", "obstacles")} for s in scenes]


def _oracle(key, params, cfg, scenes, actions, observe=False):
    """Per scene: [(bodies, reward, terminated, info, obs) per step] and the oracle's counts.  Computed once per batch and shared by the kernels."""
    if key not in _REF:
        from oracle.oracle import OracleShipIce
        out = []
        for e, sc in enumerate(_plain(scenes)):
            o = OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
            o.reset(sc, observe=False)
            rec = []
            for t in range(STEPS):
                ob, r, term, info = o.step(float(actions[t, e]), observe=observe)
                rec.append((o.bodies().copy(), r, term, np.array(list(info.values())), ob))
            out.append((rec, o.caps_stats()))
        _REF[key] = out
    return _REF[key]


def _gpu(monkeypatch, envvars, radius, scenes, actions, damping=0.0, want_pair=None, prof=False, observe=False, reset_after=False):
    import benchpush_amd.envs.ship_ice as si
    from benchpush_amd._lib import BpError
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    real = si.ship_ice_physics_params
    monkeypatch.setattr(si, "ship_ice_physics_params", lambda cfg: F.fuzz_params(real(cfg), radius, SUBSTEPS))
    E = len(scenes)
    cfg = {"concentration": 0.1, "sim": {"damping": damping}} if damping else {"concentration": 0.1}
    env = si.BatchedShipIceEnv(E, cfg=cfg, trials=_plain(scenes), device="cuda:0")    # env e plays scene e in episode 0, scene (e + 1) % E in episode 1
    monkeypatch.setattr(si, "ship_ice_physics_params", real)
    assert env.params["settle_steps"] == 1 and env.params["steps"] == SUBSTEPS and (env.params["damping_pow"] != 0.0) == (damping != 0.0)
    if want_pair is None:
        want_pair = int(envvars.get("BP_PAIR", "0"))
    assert int(env.L.bp_pair_mode(env.h)) == want_pair, "the fuzz must run the kernel it names"
    out = {"steps": [], "peaks": np.zeros((E, 64), np.int64), "caps": {k: np.zeros(E, np.int64) for k in ("neighbours", "reset_neighbours", "colours", "lanes", "purges")}}
    pbuf = None
    if prof:
        pbuf = torch.zeros((E, 64), dtype=torch.int64, device="cuda:0")
        env.L.bp_debug_prof(env.h, pbuf.data_ptr())
        env.set_resettle(True)           # the settle sub-step runs in reset(), where the counters can see it, instead of at load

    def launch_peaks():                  # a launch adds its counters to the buffer: cleared before every launch, each is the launch's own
        if pbuf is not None:
            torch.cuda.synchronize()
            p = pbuf.cpu().numpy()
            out["peaks"] = np.maximum(out["peaks"], p)
            w = p[:, P_CAPS]             # five fields in one word: the peaks field by field, the purges summed
            for k, v in (("neighbours", w & 255), ("colours", (w >> 8) & 255), ("lanes", (w >> 16) & 255), ("reset_neighbours", (w >> 32) & 255)):
                out["caps"][k] = np.maximum(out["caps"][k], v)
            out["caps"]["purges"] = out["caps"]["purges"] + ((w >> 24) & 255)
            pbuf.zero_()

    env.reset()
    launch_peaks()
    out["flags_at_reset"] = env.error_flags().copy()
    for t in range(STEPS):
        obs, rew, term, _, info = env.step(torch.from_numpy(actions[t]))
        launch_peaks()
        out["steps"].append((env.body_state().cpu().numpy().copy(), env.num_bodies().copy(), rew.cpu().numpy().copy(), term.cpu().numpy().copy(),
                             info.cpu().numpy().copy(), obs.cpu().numpy().copy() if observe else None))
    out["flags"] = env.error_flags().copy()
    pst = np.zeros(16, np.int32)
    env.L.bp_get_pair_stats(env.h, pst.ctypes.data)
    out["pairstat"] = pst       # [0..7] the pairing parameters, [8..] cumulative: paired first tasks, paired tasks from the queues, halves finished in a pair,
    try:                        # halves that carried on alone, halves queued as heavy, halves queued as light
        env.check_errors()
        out["raised"] = False
    except BpError:
        out["raised"] = True
    if reset_after:
        env.reset(torch.ones(E, dtype=torch.bool, device="cuda:0"))
        out["flags_after_reset"] = env.error_flags().copy()
    out["params"], out["cfg"] = dict(env.params), env.cfg
    env.close()
    return out


def _assert_env_equals_oracle(what, got, ref, e, observe=False):
    for t in range(STEPS):
        bs, nb, rew, term, info, obs = got["steps"][t]
        ob, orr, ot, oi, oobs = ref[e][0][t]
        assert nb[e] == len(ob), (what, "bodies", e)
        if not np.array_equal(bs[e, : nb[e]], ob):
            bad = np.nonzero((bs[e, : nb[e]] != ob).any(axis=1))[0]
            raise AssertionError("%s: scene %d, step %d: body state differs from the oracle for shapes %s" % (what, e, t, bad.tolist()))
        assert rew[e] == orr and bool(term[e]) == ot, (what, "reward / termination", e, t)
        assert np.array_equal(info[e], oi), (what, "info", e, t)
        if observe:
            assert np.array_equal(obs[e], oobs), (what, "observation", e, t)


def _kernels():
    return [(n, v, 0.0) for n, v in KERNELS] + [(DAMPED[0], DAMPED[1], DAMPING)]


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("family", list(F.LEGAL))
def test_at_and_below_capacity_equals_oracle(monkeypatch, family, radius):
    scenes = F.make_scenes(family, radius)
    acts = F.actions_for(len(scenes))
    nstrict_at_limit = 0
    for name, envvars, damping in _kernels():
        fixed = envvars.get("BP_PAIR") == "1"
        if fixed and family in ("lanes", "slots"):
            continue      # every scene of these two families is beyond the half-wave: the fixed pairs could only flag them all (module docstring)
        got = _gpu(monkeypatch, envvars, radius, scenes, acts, damping=damping)
        ref = _oracle((family, radius, damping), got["params"], got["cfg"], scenes, acts)
        what = "%s, %s, radius %g" % (name, family, radius)
        for e, sc in enumerate(scenes):
            caps = ref[e][1]
            if fixed and (caps["lanes_max"] > PP_LANES or caps["slots_max"] > PP_SLOTS):
                # fixed pairs cannot leave: beyond the half-wave the env is flagged, never wrong without a flag (bodies that share the half's last slot
                # share its colour mask too, so the colouring may run out of colours as a consequence)
                assert got["flags"][e] & ARB and not got["flags"][e] & ~(ARB | LEVEL), (what, e, got["flags"][e])
                continue
            assert got["flags"][e] == 0, (what, "flag", e, sc["target"], int(got["flags"][e]))
            _assert_env_equals_oracle(what, got, ref, e)
            if fixed and family.startswith("pair_") and sc["target"] == F.CAPACITY[family]:
                nstrict_at_limit += 1     # exactly 32 lanes / 40 slots in half a wavefront, held to == like any other env
    if family.startswith("pair_"):
        assert nstrict_at_limit >= 4


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_lane_and_stride_edges_equal_oracle(monkeypatch, radius):
    """Fields of 63 .. 449 bodies whose colliding bodies straddle 63|64 and 127|128, an empty scene in every batch; body capacity 192 | 200 (the moving list
    grows with the field) and 448 (paired kernels on) | 456 (pairing refused, and the result still equals the oracle)."""
    for cap, scenes in F.make_edge_batches(radius).items():
        acts = F.actions_for(len(scenes), seed=cap)
        for name, envvars, damping in _kernels():
            want = int(envvars.get("BP_PAIR", "0")) if cap <= PP_NBCAP else 0
            got = _gpu(monkeypatch, envvars, radius, scenes, acts, damping=damping, want_pair=want)
            ref = _oracle(("edges", cap, radius, damping), got["params"], got["cfg"], scenes, acts)
            what = "%s, fields of up to %d bodies, radius %g" % (name, cap, radius)
            assert got["steps"][0][0].shape[1] == cap
            assert not got["flags"].any(), (what, got["flags"])
            for e in range(len(scenes)):
                _assert_env_equals_oracle(what, got, ref, e)


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("family", ["colours", "neighbours", "lanes", "slots"])
def test_device_counts_reach_the_capacity(monkeypatch, prof_twin, family, radius):
    """One launch per step (BP_SCHED=0) in the -DBP_PROF twin, counters cleared before every launch: the peak the device saw equals the scene's target --
    16 colours, 24 neighbours, 64 arbiter lanes, 96 velocity slots on the "exactly at" scenes -- and the other counts stay inside their capacities."""
    scenes = F.make_scenes(family, radius)
    acts = F.actions_for(len(scenes))
    got = _gpu(monkeypatch, {"BP_PAIR": "0", "BP_SCHED": "0"}, radius, scenes, acts, prof=True)
    ref = _oracle((family, radius, 0.0), got["params"], got["cfg"], scenes, acts)
    assert not got["flags"].any()
    p = got["peaks"]
    seen = dict(got["caps"], slots=p[:, P_SLOTS])
    assert not seen.pop("purges").any()
    targets = np.array([sc["target"] for sc in scenes])
    print(family, radius, "targets", targets.tolist(), "device", {k: v.tolist() for k, v in seen.items()}, "lanes after the filter", p[:, P_LANES].tolist())
    if family == "neighbours":
        # the list build of the reset and refresh_body keep separate peaks: every hub has its count at reset, and in the scenes whose hub the ship pushes out of
        # its fat AABB within the three steps refresh_body finds the same count again (the boxes on its edges have fewer neighbours than the hub)
        assert np.array_equal(seen["reset_neighbours"], targets), (seen["reset_neighbours"].tolist(), targets.tolist())
        assert (seen["neighbours"] <= targets).all()
        for t in F.LEGAL[family]:
            assert ((seen["neighbours"] == targets) & (targets == t)).sum() >= 2, (t, seen["neighbours"].tolist())
    else:
        assert np.array_equal(seen[family], targets), (family, seen[family].tolist(), targets.tolist())
        assert F.CAPACITY[family] in seen[family]
    seen["neighbours"] = np.maximum(seen["neighbours"], seen.pop("reset_neighbours"))
    assert (seen["neighbours"] <= 24).all() and (seen["colours"] <= 16).all() and (seen["lanes"] <= 64).all() and (seen["slots"] <= 96).all()
    assert np.array_equal(seen["lanes"], [ref[e][1]["lanes_max"] for e in range(len(scenes))])       # the oracle counts in the device's units
    assert np.array_equal(seen["slots"], [ref[e][1]["slots_max"] for e in range(len(scenes))])
    assert np.array_equal(p[:, P_LANES], [ref[e][1]["cached_max"] for e in range(len(scenes))])
    for e in range(len(scenes)):
        _assert_env_equals_oracle("prof twin, %s" % family, got, ref, e)


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_reciprocal_insertion_purges_a_full_neighbour_list(monkeypatch, prof_twin, radius):
    """fuzz_caps.purge_scene: the hub's list holds 24 entries, two of them stale, when the floe the ship drives towards it is re-listed.  The twin counts at
    least one purge per scene and sees a rebuild find 24 neighbours; no flag; every kernel equals the oracle."""
    scenes = F.make_purge_scenes(radius)
    acts = F.actions_for(len(scenes))
    got = _gpu(monkeypatch, {"BP_PAIR": "0", "BP_SCHED": "0"}, radius, scenes, acts, prof=True)
    ref = _oracle(("purge", radius, 0.0), got["params"], got["cfg"], scenes, acts)
    caps = got["caps"]
    print("purge", radius, "purges", caps["purges"].tolist(), "neighbours at reset", caps["reset_neighbours"].tolist(), "in refresh_body", caps["neighbours"].tolist())
    assert not got["flags"].any(), got["flags"]
    assert (caps["purges"] >= 1).all() and (caps["reset_neighbours"] == 24).all() and (caps["neighbours"] < 24).all()   # the hub's list is never rebuilt
    for e in range(len(scenes)):
        _assert_env_equals_oracle("prof twin, purge", got, ref, e)
    monkeypatch.setenv("BP_PROF", "0")       # the product library for the kernels
    from benchpush_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    for name, envvars, damping in _kernels():
        got = _gpu(monkeypatch, envvars, radius, scenes, acts, damping=damping)
        ref = _oracle(("purge", radius, damping), got["params"], got["cfg"], scenes, acts)
        assert not got["flags"].any(), (name, got["flags"])
        for e in range(len(scenes)):
            _assert_env_equals_oracle("%s, purge, radius %g" % (name, radius), got, ref, e)


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("family", list(F.OVER))
def test_over_capacity_is_flagged_and_stays_in_its_env(monkeypatch, family, radius):
    scenes = F.make_over_scenes(family, radius)
    acts = F.actions_for(len(scenes))
    over = np.array([sc["family"] != "ordinary" for sc in scenes])
    assert over[1::2].all() and not over[0::2].any() and len(scenes) % 2 == 1
    E = len(scenes)
    for name, envvars in KERNELS:
        got = _gpu(monkeypatch, envvars, radius, scenes, acts, observe=True, reset_after=True)
        ref = _oracle((family, radius, "over"), got["params"], got["cfg"], scenes, acts, observe=True)
        what = "%s, over %s, radius %g" % (name, family, radius)
        assert got["raised"], what
        assert np.array_equal(got["flags"], np.where(over, BIT[family], 0)), (what, got["flags"].tolist())
        for e in range(E):
            if not over[e]:
                _assert_env_equals_oracle(what, got, ref, e, observe=True)     # the overflow wrote nothing outside its own env
            else:
                for t in range(STEPS):
                    bs, nb = got["steps"][t][0], got["steps"][t][1]
                    assert nb[e] == 1 + len(scenes[e]["obstacles"]) and np.isfinite(bs[e, : nb[e]]).all(), (what, e, t)
        # flags are sticky, and reset(mask) ORs in what the next trial's template raised while it settled: env e now plays scene (e + 1) % E
        want = np.where(over | np.roll(over, -1), BIT[family], 0)
        assert np.array_equal(got["flags_after_reset"], want), (what, got["flags_after_reset"].tolist())


@pytest.mark.parametrize("radius", [0.02, 0.0])
@pytest.mark.parametrize("kind", ["lanes", "slots"])
def test_capacity_reached_in_the_middle_of_a_step(monkeypatch, prof_twin, kind, radius):
    """fuzz_caps.midstep_scene: the last arbiter lane / velocity slot is taken while the first env step runs (arbiters_take / slot_get of the step kernels, not
    the reset's), for lanes with a stale arbiter holding one of the 64.  At 63, 64 lanes and 95, 96 slots: the twin counts the target (and fewer active arbiters
    than lanes), every kernel equals the oracle.  At 65 lanes / 97 slots: no flag after reset() -- the template is legal --, BP_ERR_ARB_OVERFLOW after the steps in
    exactly those envs, raised by the kernel the variant names; the ordinary envs equal the oracle."""
    scenes = F.make_midstep_scenes(kind, radius)
    acts = F.actions_for(len(scenes))
    got = _gpu(monkeypatch, {"BP_PAIR": "0", "BP_SCHED": "0"}, radius, scenes, acts, prof=True)
    ref = _oracle(("mid", kind, radius), got["params"], got["cfg"], scenes, acts)
    targets = np.array([sc["target"] for sc in scenes])
    seen = got["caps"]["lanes"] if kind == "lanes" else got["peaks"][:, P_SLOTS]
    print("mid-step", kind, radius, "targets", targets.tolist(), "device", seen.tolist(), "active", got["peaks"][:, P_ACTIVE].tolist())
    assert not got["flags"].any() and np.array_equal(seen, targets) and F.CAPACITY[kind] in seen
    if kind == "lanes":
        assert (got["peaks"][:, P_ACTIVE] < seen).all()
    for e in range(len(scenes)):
        _assert_env_equals_oracle("prof twin, mid-step %s" % kind, got, ref, e)
    monkeypatch.setenv("BP_PROF", "0")       # the product library for the kernels
    from benchpush_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    over_scenes = F.make_midstep_over_scenes(kind, radius)
    over_acts = F.actions_for(len(over_scenes))
    over = np.array([sc["family"] != "ordinary" for sc in over_scenes])
    for name, envvars, damping in _kernels():
        if envvars.get("BP_PAIR") == "1":
            continue      # beyond the half-wave from the start: see test_at_and_below_capacity_equals_oracle
        got = _gpu(monkeypatch, envvars, radius, scenes, acts, damping=damping)
        ref = _oracle(("mid", kind, radius, damping), got["params"], got["cfg"], scenes, acts)
        assert not got["flags"].any(), (name, got["flags"])
        for e in range(len(scenes)):
            _assert_env_equals_oracle("%s, mid-step %s, radius %g" % (name, kind, radius), got, ref, e)
        got = _gpu(monkeypatch, envvars, radius, over_scenes, over_acts, damping=damping, observe=True)
        ref = _oracle(("mid over", kind, radius, damping), got["params"], got["cfg"], over_scenes, over_acts, observe=True)
        assert not got["flags_at_reset"].any(), (name, got["flags_at_reset"].tolist())
        assert got["raised"] and np.array_equal(got["flags"], np.where(over, ARB, 0)), (name, got["flags"].tolist())
        for e in range(len(over_scenes)):
            if not over[e]:
                _assert_env_equals_oracle("%s, over mid-step %s" % (name, kind), got, ref, e, observe=True)
            else:
                assert all(np.isfinite(st[0][e, : st[1][e]]).all() for st in got["steps"]), (name, e)


@pytest.mark.parametrize("radius", [0.02, 0.0])
def test_env_leaves_its_pair_in_the_middle_of_a_step(monkeypatch, radius):
    """Pairs inside the scheduler (BP_PAIR=2), every first task a pair and the heaviness limits out of the way, so that only the capacity limits decide:
    envs with exactly 26 arbiter lanes or exactly 34 velocity slots are admitted (the control batch keeps those counts: no half is ever parked out of a pair),
    and the batch whose envs take one more in the first env step parks halves out of their pairs -- the mid-step leave.  Both batches equal the oracle, no flag."""
    envvars = {"BP_PAIR": "2", "BP_PAIR_SOLO": "0", "BP_PP_ACT": "64", "BP_PP_WORK": "1000000", "BP_PP_RATE": "1000000"}
    left = {}
    for leave in (False, True):
        scenes = F.make_pair_leave_scenes(radius, leave)
        acts = F.actions_for(len(scenes))
        got = _gpu(monkeypatch, envvars, radius, scenes, acts)
        ref = _oracle(("pair leave", radius, leave), got["params"], got["cfg"], scenes, acts)
        pst = got["pairstat"]
        print("pair leave", radius, leave, pst.tolist())
        assert pst[2] == F.PAIR_KEYS and pst[3] == F.PAIR_SLOTS
        assert not got["flags"].any(), got["flags"]
        for e in range(len(scenes)):
            _assert_env_equals_oracle("pairs inside the scheduler, leave=%s" % leave, got, ref, e)
        assert pst[8] >= len(scenes) // 2      # every first task of every step was a pair
        left[leave] = int(pst[11] + pst[12])      # parked out of a pair as heavy: over a limit (the mate it takes along counts as light)
    assert left[False] == 0 and left[True] >= len(scenes) // 2, left


def _maze_run(monkeypatch, envvars, layouts, actions, prof=False):
    import benchpush_amd.envs.maze_namo as mz
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    real = mz.maze_physics_params

    def params_of(cfg):
        p = dict(real(cfg))
        p.update(settle_steps=1, steps=SUBSTEPS, dt=float(p["dt"]) / int(p["steps"]) * SUBSTEPS)
        return p

    monkeypatch.setattr(mz, "maze_physics_params", params_of)
    N = len(layouts)
    env = mz.BatchedMazeEnv(N, cfg={"num_obstacles": F.MAZE_BOXES, "maze_version": 1}, layouts=[{k: l[k] for k in ("centres", "walls", "start")} for l in layouts],
                            device="cuda:0")
    monkeypatch.setattr(mz, "maze_physics_params", real)
    assert env.params["settle_steps"] == 1 and env.params["steps"] == SUBSTEPS
    out = {"steps": [], "lanes": np.zeros(N, np.int64)}
    pbuf = None
    if prof:
        pbuf = torch.zeros((N, 64), dtype=torch.int64, device="cuda:0")
        env.L.bp_debug_prof(env.h, pbuf.data_ptr())
        env.set_resettle(True)

    def launch_peaks():
        if pbuf is not None:
            torch.cuda.synchronize()
            out["lanes"] = np.maximum(out["lanes"], (pbuf.cpu().numpy()[:, P_CAPS] >> 16) & 255)
            pbuf.zero_()

    env.reset()
    launch_peaks()
    for t in range(STEPS):
        _, rew, term, _, info = env.step(torch.from_numpy(actions[t]))
        launch_peaks()
        out["steps"].append((env.body_state().cpu().numpy().copy(), rew.cpu().numpy().copy(), term.cpu().numpy().copy(), info.cpu().numpy().copy()))
    out["flags"] = env.error_flags().copy()
    out["params"], out["cfg"] = dict(env.params), env.cfg
    env.close()
    return out


def _maze_oracle(key, params, cfg, layouts, actions):
    if key not in _REF:
        from oracle.oracle import OracleMaze
        out = []
        for e, lay in enumerate(layouts):
            o = OracleMaze(params, cfg.robot.vertices, cfg.robot.wheel_vertices, cfg.obstacle_size)
            o.reset(lay, observe=False)
            rec = []
            for t in range(STEPS):
                _, r, term, info = o.step(float(actions[t, e]), observe=False)
                rec.append((o.shape_states().copy(), r, term, np.array(list(info.values()))))
            out.append(rec)
        _REF[key] = out
    return _REF[key]


def _assert_maze_env_equals_oracle(what, got, ref, e):
    for t in range(STEPS):
        bs, rew, term, info = got["steps"][t]
        ss, orr, ot, oi = ref[e][t]
        if not np.array_equal(bs[e, : len(ss)], ss):
            bad = np.nonzero((bs[e, : len(ss)] != ss).any(axis=1))[0]
            raise AssertionError("%s: layout %d, step %d: shape state differs from the oracle for shapes %s" % (what, e, t, bad.tolist()))
        assert rew[e] == orr and bool(term[e]) == ot, (what, "reward / termination", e, t)
        assert np.array_equal(info[e], oi), (what, "info", e, t)


MAZE_KERNELS = (("scheduled, resident (default)", {}), ("one wavefront per env, no scheduler", {"BP_SCHED": "0"}))


def test_maze_piles_at_the_lane_capacity_equal_oracle(monkeypatch, prof_twin):
    """substep<BP_ENV_MAZE> at 62, 63 and 64 arbiter lanes (fuzz_caps.maze_lanes_layout: a pile of overlapping boxes that the bias impulses drive apart, so
    lanes are freed while the steps run): the twin counts the layout's target in lanes, no flag; both maze kernels equal OracleMaze."""
    from benchpush_amd.config import maze_walls
    import benchpush_amd.envs.maze_namo as mz
    layouts = F.make_maze_layouts(maze_walls(mz._maze_cfg({"num_obstacles": F.MAZE_BOXES, "maze_version": 1})))
    acts = F.actions_for(len(layouts), seed=13)
    got = _maze_run(monkeypatch, {"BP_SCHED": "0"}, layouts, acts, prof=True)
    ref = _maze_oracle("maze", got["params"], got["cfg"], layouts, acts)
    print("maze lanes", got["lanes"].tolist())
    assert not got["flags"].any(), got["flags"]
    assert np.array_equal(got["lanes"], [l["target"] for l in layouts]) and 64 in got["lanes"]
    for e in range(len(layouts)):
        _assert_maze_env_equals_oracle("prof twin, maze", got, ref, e)
    monkeypatch.setenv("BP_PROF", "0")       # the product library for the kernels
    from benchpush_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    for name, envvars in MAZE_KERNELS:
        got = _maze_run(monkeypatch, envvars, layouts, acts)
        assert not got["flags"].any(), (name, got["flags"])
        for e in range(len(layouts)):
            _assert_maze_env_equals_oracle(name, got, ref, e)


def test_maze_pile_over_the_lane_capacity_is_flagged_and_stays_in_its_env(monkeypatch):
    """[ordinary, over, ordinary, ...] with piles of 65 and 69 arbiters: BP_ERR_ARB_OVERFLOW in exactly those envs, their state finite, the ordinary envs ==
    OracleMaze.  (The piles are over the capacity from the settle sub-step, like the ship-ice scenes: see the module docstring.)"""
    from benchpush_amd.config import maze_walls
    import benchpush_amd.envs.maze_namo as mz
    layouts = F.make_maze_over_layouts(maze_walls(mz._maze_cfg({"num_obstacles": F.MAZE_BOXES, "maze_version": 1})))
    acts = F.actions_for(len(layouts), seed=13)
    over = np.array([l["family"] != "ordinary" for l in layouts])
    assert over[1::2].all() and not over[0::2].any()
    for name, envvars in MAZE_KERNELS:
        got = _maze_run(monkeypatch, envvars, layouts, acts)
        ref = _maze_oracle("maze over", got["params"], got["cfg"], layouts, acts)
        assert np.array_equal(got["flags"], np.where(over, ARB, 0)), (name, got["flags"].tolist())
        for e in range(len(layouts)):
            if not over[e]:
                _assert_maze_env_equals_oracle(name + ", over", got, ref, e)
            else:
                assert all(np.isfinite(st[0][e]).all() for st in got["steps"]), (name, e)
