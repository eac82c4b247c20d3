"""Lane groups of the plane-bound rounds (substep 4a': three sides per round, 21 lanes each) against the CPU oracle (-m gpu).

Bar: bit-exact.  The mapping only changes which lane evaluates which plane of which surviving pair; every separation is computed by the same
operations, and the per-side maxima are resolved by atomics on keys, so body state, rewards, info and observations must equal the oracle's with ==.
The cases are the ones in which the grouping can go wrong: candidate rounds with four and more surviving pairs (more than one trip, a last trip that
is only partly filled), the diagnostic bit that takes one side per round (every pair a trip of its own), hulls that fill a 21-lane group to its last
plane (20 vertices: f = 19, the idle f = 20 and lane 63) next to small ones, the 8-vertex instantiation of the maze, and the scheduler's resumed
waves against the one-wave-per-env kernel.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run_ship(E, trials, steps, seed, cfg, actions=None):
    """E ship-ice envs against E oracles, every output compared after every step.  Returns the ship's contact-point count at the end."""
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from oracle.oracle import OracleShipIce
    env = BatchedShipIceEnv(E, cfg=cfg, trials=trials, device="cuda:0")
    T = len(trials)
    obs, _ = env.reset()
    c = env.cfg
    orcs = [OracleShipIce(env.params, c.ship.vertices, c.ship.head, c.ship.tail) for _ in range(E)]
    for e, o in enumerate(orcs):
        oo, _ = o.reset(trials[e % T])
        assert np.array_equal(obs[e].cpu().numpy(), oo), ("reset obs", e)
    rng = np.random.default_rng(seed)
    ncontact = 0
    for t in range(steps):
        a = rng.uniform(-1, 1, E) if actions is None else np.asarray(actions[t], np.float64)
        a = a.astype(np.float32).astype(np.float64)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a))
        bs, nb = env.body_state().cpu().numpy(), env.num_bodies()
        go, gi, gr, gt = obs.cpu().numpy(), info.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
        assert not trunc.any() and not gt.any()           # short runs: nobody reaches the goal line
        for e, o in enumerate(orcs):
            oo, orr, ot, oi = o.step(float(a[e]))
            ob = o.bodies()
            assert nb[e] == len(ob)
            assert np.array_equal(bs[e, : nb[e]], ob), ("bodies", t, e)
            assert np.array_equal(go[e], oo), ("obs", t, e)
            assert np.array_equal(gi[e], np.array(list(oi.values()))), ("info", t, e)
            assert gr[e] == orr and bool(gt[e]) == ot, ("reward/term", t, e)
            ncontact = max(ncontact, int(oi["n_contact_pts"]))
    env.check_errors()
    env.close()
    return ncontact


def test_crowded_candidate_rounds_match_oracle():
    """50 % concentration: the ship ploughs through packed floes, candidate rounds carry four and more surviving pairs, i.e. two and more trips of three
    pairs with every filling of the last one."""
    from benchpush_amd.envs.ship_ice import default_trials
    assert _run_ship(8, default_trials(0.5, 3, base_seed=31), steps=6, seed=31, cfg={"concentration": 0.5}) > 100


def test_one_side_per_round_matches_oracle(monkeypatch):
    """BP_DEBUG_PATHS bit 16 (diagnostic twin): one side per bound round, so every surviving pair takes a trip of its own and the trip loop runs as
    often as there are survivors.  Alone and together with bit 2, which sends the rounds through the flushing loop that reads the same side table."""
    from benchpush_amd import _lib
    from benchpush_amd.build import DBG_LIB_PATH, build_debug_paths
    from benchpush_amd.envs.ship_ice import default_trials
    build_debug_paths()                                   # up to date after the build step: a no-op
    monkeypatch.setattr(_lib, "_lib", None)               # load the twin for this test only; monkeypatch restores the product library afterwards
    monkeypatch.setenv("BP_PROF", "1")
    monkeypatch.setenv("BP_PROF_LIB", DBG_LIB_PATH)
    trials = default_trials(0.5, 3, base_seed=31)
    for mask in (16, 18):
        monkeypatch.setenv("BP_DEBUG_PATHS", str(mask))
        assert _run_ship(8, trials, steps=6, seed=31, cfg={"concentration": 0.5}) > 100


def _hull(n, cx, cy, rx, ry, phase):
    """n vertices on an ellipse at uneven, increasing angles: strictly convex, counter-clockwise."""
    k = np.arange(n)
    ang = phase + 2 * np.pi * (k + 0.3 * np.sin(1.7 * k + n)) / n
    return np.stack([cx + rx * np.cos(ang), cy + ry * np.sin(ang)], axis=1)


def _hull_size_trial(start_x, shift):
    """Rows of touching floes right ahead of the ship that alternate between 20 vertices (a full lane group: planes f = 0..19) and 10."""
    obstacles = []
    for row in range(4):
        for col in range(5):
            n = 20 if (row + col + shift) % 2 == 0 else 10
            cx, cy = start_x - 2.0 + 1.0 * col + 0.5 * (row % 2), 2.6 + 0.9 * row
            v = _hull(n, cx, cy, 0.51, 0.50, 0.37 * (row * 5 + col))
            obstacles.append({"vertices": v, "centre": (float(cx), float(cy)), "radius": 0.51})
    return {"goal": (0, 9.0), "ship_state": (float(start_x), 1.0, float(np.pi / 2)), "obstacles": obstacles}


def test_hulls_of_20_and_10_vertices_beside_the_ship():
    """Group edges: a 20-vertex hull uses every plane lane of its group (f = 19 is the last, f = 20 and lane 63 stay idle), its 10-vertex neighbour
    half of them, the ship's hull fewer still.  The floes touch from the start, so ship x 20, ship x 10 and 20 x 10 pairs survive into the bound rounds together."""
    trials = [_hull_size_trial(5.6, 0), _hull_size_trial(6.3, 1)]
    counts = sorted({len(o["vertices"]) for t in trials for o in t["obstacles"]})
    assert counts == [10, 20]
    rng = np.random.default_rng(2)
    acts = rng.uniform(-0.4, 0.4, (8, 4))
    assert _run_ship(4, trials, steps=8, seed=0, cfg={"concentration": 0.3}, actions=acts) > 20


def test_maze_instantiation_matches_oracle():
    """The maze kernels instantiate the sub-step with 8-vertex loops (VL = 8): 8 envs x 6 steps among 20 boxes, straight into them."""
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    from oracle.oracle import OracleMaze
    E, T, steps = 8, 3, 6
    env = BatchedMazeEnv(E, cfg={"num_obstacles": 20}, num_layouts=T, base_seed=12, device="cuda:0")
    obs, _ = env.reset()
    c = env.cfg
    orcs = [OracleMaze(env.params, c.robot.vertices, c.robot.wheel_vertices, c.obstacle_size) for _ in range(E)]
    for e, o in enumerate(orcs):
        assert np.array_equal(obs[e].cpu().numpy(), o.reset(env.layouts[e % T])), ("reset obs", e)
    rng = np.random.default_rng(12)
    for t in range(steps):
        a = rng.uniform(-1, 1, E)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a))
        bs = env.body_state().cpu().numpy()
        go, gi, gr, gt = obs.cpu().numpy(), info.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy()
        for e, o in enumerate(orcs):
            oo, orr, ot, oi = o.step(float(a[e]))
            ss = o.shape_states()
            assert np.array_equal(bs[e, : len(ss)], ss), ("state", t, e)
            assert np.array_equal(go[e], oo), ("obs", t, e)
            assert np.array_equal(gi[e], np.array(list(oi.values()))), ("info", t, e)
            assert gr[e] == orr and bool(gt[e]) == ot, ("reward/term", t, e)
        if gt.any():
            break                                         # (a robot on a wall ends its episode: the steps so far have been compared)
    env.check_errors()
    env.close()


def test_scheduled_step_equals_one_wave_per_env(monkeypatch):
    """512 envs x 8 steps of the flagship configuration (30 %): the default scheduler path, whose waves park and resume between chunks of sub-steps,
    leaves exactly what the one-wave-per-env kernel (BP_SCHED=0) leaves."""
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    E, steps = 512, 8
    trials = default_trials(0.3, 16, base_seed=40)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(40)
    acts = (torch.rand((steps, E), generator=g, device="cuda:0", dtype=torch.float64) * 2 - 1).float().double()

    def run(env_vars):
        for k in ("BP_SCHED", "BP_SCHED_PERSIST", "BP_PAIR"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env_vars.items():
            monkeypatch.setenv(k, v)
        env = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, trials=trials, device="cuda:0")
        assert (env.sched_chunk() == 0) == (env_vars.get("BP_SCHED") == "0")
        env.reset()
        rsum = torch.zeros(E, dtype=torch.float64, device="cuda:0")
        for t in range(steps):
            _, rew, term, _, _ = env.step(acts[t])
            rsum += rew
            env.reset(term)
        env.check_errors()
        out = (env.body_state().clone(), rsum, env.obs.clone(), env.info.clone())
        env.close()
        return out

    ref = run({"BP_SCHED": "0"})
    got = run({})
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
