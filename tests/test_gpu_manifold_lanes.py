"""Manifold phase with one lane per side of a pair (substep 4b / 4c, manifold_lanes) against the CPU oracle (-m gpu).

Bar: bit-exact.  The mapping only changes which lane evaluates which shape's half of a pair's manifold and sends the few shared values across with DPP; every
floating-point value comes from the operands and the operation order of the one-lane text, so body state, rewards, info and observations must equal the
oracle's with ==.  The cases are the ones in which the mapping can go wrong: crowded candidate rounds (lane pairs next to each other in a quad and a row, more
survivors than mailbox entries per batch), the diagnostic bits that restore the one-lane text and that give every pair a trip of its own, hulls of 20 vertices
(vertex indices up to 19 in the feature hashes), the maze's 8-vertex instantiation with its flag-only robot x wall pairs, the scheduler's resumed waves, and a
run of the counter twin that shows that every branch of the new text was taken.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# -DBP_PROF counters of the manifold phase (bp_debug_prof slots 50..55; where two counts share a slot the second is in the high word)
P_TRIPS, P_N_PLANE, P_N_VERTEX, P_QUERY, P_ONE, P_TWO = 50, 51, 52, 53, 54, 55


def _run_ship(E, trials, steps, seed, cfg, actions=None, prof=False):
    """E ship-ice envs against E oracles, every output compared after every step.  Returns the ship's contact-point count at the end (and the twin's counters)."""
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from oracle.oracle import OracleShipIce
    env = BatchedShipIceEnv(E, cfg=cfg, trials=trials, device="cuda:0")
    T = len(trials)
    counters = None
    if prof:
        counters = torch.zeros((E, 64), dtype=torch.int64, device="cuda:0")
        env.L.bp_debug_prof(env.h, counters.data_ptr())
    obs, _ = env.reset()
    c = env.cfg
    orcs = [OracleShipIce(env.params, c.ship.vertices, c.ship.head, c.ship.tail) for _ in range(E)]
    for e, o in enumerate(orcs):
        oo, _ = o.reset(trials[e % T])
        assert np.array_equal(obs[e].cpu().numpy(), oo), ("reset obs", e)
    if prof:
        counters.zero_()
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
    if prof:
        torch.cuda.synchronize()
        counters = counters.sum(dim=0).cpu().numpy()
    env.close()
    return (ncontact, counters) if prof else ncontact


def _crowded():
    from benchpush_amd.envs.ship_ice import default_trials
    return default_trials(0.5, 3, base_seed=31)


def test_crowded_fields_match_oracle():
    """50 % concentration: the ship ploughs through packed floes; candidate rounds carry several surviving pairs, so neighbouring lane pairs are live together."""
    assert _run_ship(8, _crowded(), steps=6, seed=31, cfg={"concentration": 0.5}) > 100


@pytest.fixture
def paths_twin(monkeypatch):
    """The -DBP_DEBUG_PATHS twin of the library for the duration of a test; the product library is loaded afresh afterwards."""
    from benchpush_amd import _lib
    from benchpush_amd.build import DBG_LIB_PATH, build_debug_paths
    build_debug_paths()                                   # up to date after the build step: a no-op
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setenv("BP_PROF", "1")
    monkeypatch.setenv("BP_PROF_LIB", DBG_LIB_PATH)
    yield
    monkeypatch.setattr(_lib, "_lib", None)


@pytest.mark.parametrize("mask", [32, 34, 64, 66], ids=["one_lane_text", "one_lane_text+flushing_loop", "one_pair_per_trip", "one_pair_per_trip+flushing_loop"])
def test_diagnostic_mappings_match_oracle(monkeypatch, paths_twin, mask):
    """BP_DEBUG_PATHS bit 32 sends every instantiation through the one-lane text (the mapping box-delivery keeps), bit 64 limits a trip to one pair, so the trip
    loop runs once per survivor and the tables are read at every rank offset.  Alone and with bit 2 (bound rounds through the flushing loop, which fills the
    same tables)."""
    monkeypatch.setenv("BP_DEBUG_PATHS", str(mask))
    assert _run_ship(8, _crowded(), steps=6, seed=31, cfg={"concentration": 0.5}) > 100


def _hull(n, cx, cy, rx, ry, phase):
    """n vertices on an ellipse at uneven, increasing angles: strictly convex, counter-clockwise."""
    k = np.arange(n)
    ang = phase + 2 * np.pi * (k + 0.3 * np.sin(1.7 * k + n)) / n
    return np.stack([cx + rx * np.cos(ang), cy + ry * np.sin(ang)], axis=1)


def _hull_size_trial(start_x, shift):
    """Rows of touching floes right ahead of the ship that alternate between 20 vertices and 10."""
    obstacles = []
    for row in range(4):
        for col in range(5):
            n = 20 if (row + col + shift) % 2 == 0 else 10
            cx, cy = start_x - 2.0 + 1.0 * col + 0.5 * (row % 2), 2.6 + 0.9 * row
            v = _hull(n, cx, cy, 0.51, 0.50, 0.37 * (row * 5 + col))
            obstacles.append({"vertices": v, "centre": (float(cx), float(cy)), "radius": 0.51})
    return {"goal": (0, 9.0), "ship_state": (float(start_x), 1.0, float(np.pi / 2)), "obstacles": obstacles}


def test_hulls_of_20_and_10_vertices_beside_the_ship():
    """Vertex indices up to 19 in the feature hashes that the two lanes of a pair put together from one index each, and the cyclic neighbours of a support
    vertex at both ends of a 20-vertex hull."""
    trials = [_hull_size_trial(5.6, 0), _hull_size_trial(6.3, 1)]
    assert sorted({len(o["vertices"]) for t in trials for o in t["obstacles"]}) == [10, 20]
    rng = np.random.default_rng(2)
    acts = rng.uniform(-0.4, 0.4, (8, 4))
    assert _run_ship(4, trials, steps=8, seed=0, cfg={"concentration": 0.3}, actions=acts) > 20


def test_maze_instantiation_matches_oracle():
    """The maze kernels: 8-vertex support queries (VL = 8) and the robot x wall pairs that are evaluated for the wall flag only and never delivered."""
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
    """512 envs x 8 steps of the flagship configuration (30 %): the default scheduler path, whose waves park and resume between chunks of sub-steps (the
    candidate cache that the even lanes now write for the candidate lanes travels in the park image), against the one-wave-per-env kernel (BP_SCHED=0)."""
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


def test_every_branch_of_the_side_lanes_is_taken(monkeypatch):
    """The counter twin (-DBP_PROF) on the crowded case: normals from a plane of A, from a plane of B and from a vertex pair, a support query posted by each
    side, and manifolds of one point from the first candidate, one point from the second, and two points -- all counted, with the oracle still matched."""
    from benchpush_amd import _lib
    from benchpush_amd.build import PROF_LIB_PATH, build_prof
    build_prof()
    monkeypatch.setattr(_lib, "_lib", None)               # load the twin for this test only; monkeypatch restores the product library afterwards
    monkeypatch.setenv("BP_PROF", "1")
    monkeypatch.setenv("BP_PROF_LIB", PROF_LIB_PATH)
    for k in ("BP_SCHED", "BP_PAIR"):                      # one wave per env: the counters of an env stay in one LDS block
        monkeypatch.setenv(k, "0")
    ncontact, p = _run_ship(8, _crowded(), steps=6, seed=31, cfg={"concentration": 0.5}, prof=True)
    lo, hi = (lambda s: int(p[s]) & 0xFFFFFFFF), (lambda s: int(p[s]) >> 32)
    got = {"trips": int(p[P_TRIPS]), "normal_plane_A": lo(P_N_PLANE), "normal_plane_B": hi(P_N_PLANE), "normal_vertex_pair": int(p[P_N_VERTEX]),
           "query_A": lo(P_QUERY), "query_B": hi(P_QUERY), "one_point_first": lo(P_ONE), "one_point_second": hi(P_ONE), "two_points": int(p[P_TWO])}
    print("manifold-phase counters:", got)
    assert ncontact > 100
    for name, v in got.items():
        assert v > 0, name
