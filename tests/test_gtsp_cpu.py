"""The GTSP push planner without a GPU: the restatement (tests/gtsp_ref.py) against the goldens recorded from the reference's own transition tables,
instance rows, evaluate_tour and PlanningBasedPolicy.act; the set DP against brute force; boundary_goals; GTSPConfig; the ABI pieces."""
import math
import os

import numpy as np
import pytest

import gtsp_ref as R
from test_track_cpu import YAW_TOL      # the tolerance of the same comparison there: the oracle's trig against the reference's libm

# The reference's tables against the restatement's: entry by entry within what the reference's arccos can differ from the atan2 angle at that
# entry's own two angles (gtsp_ref.arccos_error, derived there; a few 1e-15 / sin(angle), 4.2e-8 only where directions are parallel), the lengths
# within LENGTH_ERR, the cost within lin_vel and ang_vel times those plus the rounding of a cost below 32.
COST_ROUND = 4 * 2.0 ** -53 * 32


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def plans(golden):
    """The restatement (with the oracle's trig) on every golden scene, computed once."""
    G, Z = golden
    out = {}
    for s in G["scenes"]:
        boxes = np.zeros((s["n"], 20, 2))
        boxes[:, :4] = Z["boxes_%d" % s["seed"]]
        out[s["seed"]] = R.plan(s["pose"], boxes, np.full(s["n"], 4), G["goals"], G["boundary"])
    return out


def test_golden_was_generated_within_its_limits(golden):
    G, _ = golden
    S = G["scenes"]
    assert len(S) >= 12 and {s["n"] for s in S} == set(range(1, 11)) and sum(s["straddle"] > 0 for s in S) >= 2
    print("generator: min distance of 100 * cost to a half-integer %.3g, max table / act difference %.3g / %.3g"
          % (G["min_half_distance"], G["max_table_diff"], G["max_act_diff"]))
    assert G["min_half_distance"] > G["near_half"] >= 1e-5 and G["max_act_diff"] <= YAW_TOL
    assert sum(s["act"] is not None for s in S) >= 3 and any(s["status"] & R.FLAG_DEGENERATE for s in S)


def test_restatement_equals_the_reference_tables_rows_and_tour(golden, plans):
    G, Z = golden
    worst, widest, lin, ang = [0.0, 0.0, 0.0], 0.0, R.DEFAULTS["lin_vel"], R.DEFAULTS["ang_vel"]
    for s in G["scenes"]:
        r = plans[s["seed"]]
        n, N = s["n"], 4 * s["n"] + 1
        assert r["status"] == s["status"] and r["n_push"] == n and r["clusters"] == list(range(n))
        W, T, B = R.weight_matrix(r["routes"], s["pose"], 4, R.DEFAULTS, tables=True, bounds=True)
        assert np.array_equal(W, Z["rows_%d" % s["seed"]]) and np.array_equal(r["W"], W)          # entry for entry, the diagonal and the clusters' zeros too
        Tref = Z["tables_%d" % s["seed"]]
        for k in range(3):
            worst[k] = max(worst[k], float(np.abs(T[k] - Tref[k]).max()))
        Bc = lin * R.LENGTH_ERR + ang * B + COST_ROUND
        widest = max(widest, float((np.abs(T[2] - Tref[2])[B > 0] / B[B > 0]).max()))
        assert (np.abs(T[2] - Tref[2]) <= B).all() and (np.abs(T[1] - Tref[1]) <= R.LENGTH_ERR).all() and (np.abs(T[0] - Tref[0]) <= Bc).all()
        # the optimum of the reference's own integer objective, and its evaluate_tour on that tour
        assert r["tour"] == s["tour"] == s["final_nodes"] and r["cost"] == s["cost"]
        seq = [N - 1] + r["tour"] + [N - 1]
        assert r["cost"] == sum(int(W[a, b]) for a, b in zip(seq[:-1], seq[1:]))
        inner = sum(T[0][a, b] for a, b in zip(r["tour"][:-1], r["tour"][1:]))
        assert abs(inner - s["transition_cost"]) <= sum(Bc[a, b] for a, b in zip(r["tour"][:-1], r["tour"][1:])) + COST_ROUND * n
        path = Z["path_%d" % s["seed"]]
        assert r["path"].shape == path.shape == (2 * n + 1, 3) and np.array_equal(r["path"][:, :2], path[:, :2])
        assert np.abs(r["path"][:, 2] - path[:, 2]).max() <= YAW_TOL
    print("restatement against the reference's tables: worst cost / length / angle difference %.3g / %.3g / %.3g; the angle difference nearest its "
          "entry's bound: %.3g of it" % (tuple(worst) + (widest,)))
    assert max(worst) == G["max_table_diff"]        # the figure the generator recorded, found again


def test_restatement_equals_the_reference_act_call_by_call(golden, plans):
    G, _ = golden
    worst, switches, ends = 0.0, 0, 0
    for s in G["scenes"]:
        if s["act"] is None:
            continue
        r = plans[s["seed"]]
        state = r["track"]
        assert state[0] == 1
        for pose, (v, om, pid) in zip(s["act"]["poses"], s["act"]["out"]):
            before = state[0]
            (sv, so), diag, state = R.track(r["path"], r["length"], pose, state, 1.0, 1.0)
            assert diag == pid == state[0]
            worst = max(worst, abs(sv - v), abs(so - om))
            switches += diag != before
            ends += diag >= r["length"] and (sv, so) == (0.0, 0.0)
    print("tracker against the reference's act: worst difference %.3g over %d switches" % (worst, switches))
    assert worst <= YAW_TOL and switches >= 10 and ends >= 3


def test_dp_equals_brute_force(golden, plans):
    G, _ = golden
    small = [s for s in G["scenes"] if s["n"] <= 5]
    assert len(small) >= 5
    for s in small:
        r = plans[s["seed"]]
        assert R.brute_force(r["W"], s["n"], 4) == (r["cost"], r["tour"])
    rng = np.random.default_rng(7)
    ties = 0
    for _ in range(200):
        n, g = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        W = rng.integers(0, int(rng.integers(2, 5)), (n * g + 1, n * g + 1))          # weights in 0..1, 0..2 or 0..3
        cost, tour = R.solve(W, n, g)
        bc, bt, optimal = R.brute_force(W, n, g, ties=True)
        assert (cost, tour) == (bc, bt)
        assert sorted(u // g for u in tour) == list(range(n))
        ties += optimal >= 2                       # a second tour costs as little: the lexicographic rule decided
    print("instances whose optimum is tied: %d of 200" % ties)
    # a quarter of the instances at the least (one with a single node per cluster and a single cluster has one tour and cannot tie)
    assert ties >= 50 and R.solve(np.zeros((1, 1)), 0, 3) == (0, []) == R.brute_force(np.zeros((1, 1)), 0, 3)


def test_restatement_edge_rules():
    bd = [(-5.0, -5.0), (-5.0, 5.0), (5.0, 5.0), (5.0, -5.0)]
    sq = lambda cx, cy, h=0.5: [(cx + h, cy + h), (cx - h, cy + h), (cx - h, cy - h), (cx + h, cy - h)]   # noqa: E731
    assert R.intersects(bd, sq(5.5, 0.0)) and not R.intersects(bd, sq(5.5 + 1e-9, 0.0))      # touching counts: the test's `< 0` is strict
    assert R.intersects(bd, sq(0.0, 0.0)[::-1])                                               # either winding
    p = R.shrink(sq(1.0, 2.0), 0.4)
    assert np.allclose(sorted(p), sorted((1.0 + a, 2.0 + b) for a in (0.1, -0.1) for b in (0.1, -0.1)), rtol=0, atol=1e-15)
    assert R.shrink(sq(0.0, 0.0, 0.3), 0.4) is None and R.shrink([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)], 0.1) is None
    tri = R.shrink([(0.0, 0.0), (4.0, 0.0), (4.0, 0.2), (0.0, 3.0)], 0.15)                    # the short edge's half-plane cuts nothing off: 3 vertices
    assert tri is not None and len(tri) == 3
    # the tie rule: an axis-aligned box facing a parallel segment has two equally near vertices, the lower index wins
    box = sq(0.0, 0.0)
    poly = R.shrink(box, 0.4)
    bp, gp, deg = R.nearest_pair(box, poly, (5.0, 5.0), (5.0, -5.0))
    d2 = [R._proj(v, (5.0, 5.0), (5.0, -5.0))[1] for v in poly]
    first = d2.index(min(d2))
    assert sum(d == min(d2) for d in d2) == 2                                                  # the tie is there
    assert not deg and bp == poly[first] and gp[0] == 5.0 and abs(gp[1] - bp[1]) <= 1e-15      # a vertex pair, not an endpoint's projection
    route, deg = R.push_route(box, poly, (5.0, 5.0), (5.0, -5.0), 2.0, 1e7)
    assert not deg and route[2][0] == 5.0 and np.allclose(route, [(bp[0] - 2.0, bp[1]), bp, (5.0, bp[1])], rtol=0, atol=1e-7)
    assert all(v == float(np.rint(v * 1e7)) / 1e7 for q in route for v in q)
    # a segment's end projected onto a box edge, worked by hand: the diamond's edge (3, 0) - (2, 1) lies on x + y = 3, the end (3.5, 1.5) of the piece
    # is sqrt(2) from it, at the edge's midpoint (2.5, 0.5); the two vertices of that edge are sqrt(2.5) from the piece, so the end wins strictly
    dia = [(3.0, 0.0), (2.0, 1.0), (1.0, 0.0), (2.0, -1.0)]
    for g0, g1 in (((3.5, 5.0), (3.5, 1.5)), ((3.5, 1.5), (3.5, 5.0))):
        assert R.nearest_pair(dia, dia, g0, g1) == ((2.5, 0.5), (3.5, 1.5), False)
        assert R.nearest_pair(dia[::-1], dia[::-1], g0, g1) == ((2.5, 0.5), (3.5, 1.5), False)
        route, deg = R.push_route(dia, dia, g0, g1, 2.0, 1e7)                                     # 2 behind (2.5, 0.5) along (-1, -1) / sqrt(2)
        assert not deg and route == [(1.0857864, -0.9142136), (2.5, 0.5), (3.5, 1.5)]
    # and not strictly: the end (2, 0.5) is 1 from the unit square's edge x = 1, the vertex (1, 1) is 1 from the piece: the vertex pair stays
    unit = [(1.0, 1.0), (0.0, 1.0), (0.0, 0.0), (1.0, 0.0)]
    assert R.nearest_pair(unit, unit, (2.0, 0.5), (2.0, 5.0)) == ((1.0, 1.0), (2.0, 1.0), False)
    # the degenerate rule: the shrunk box lies on the segment
    box = sq(5.0, 1.0)
    route, deg = R.push_route(box, R.shrink(box, 0.4), (5.0, 5.0), (5.0, -5.0), 2.0, 1e7)
    assert deg and route == [(5.0, 1.0)] * 3
    # the plan's status rules
    boxes = np.zeros((3, 20, 2))
    boxes[0, :4], boxes[2, :4] = sq(6.0, 0.0), sq(0.0, 0.0, 0.3)
    goals = [[bd[i], bd[(i + 1) % 4]] for i in range(4)]
    r = R.plan((0.0, 0.0, 0.0), boxes, [4, 0, 4], goals, bd)
    assert r["status"] == R.NOTHING_TO_PUSH | R.FLAG_VANISHED and r["length"] == 1 and r["W"].tolist() == [[R.SELF_WEIGHT]]
    assert R.plan((math.nan, 0.0, 0.0), boxes, [4, 0, 4], goals, bd)["status"] == R.INVALID
    assert R.plan((0.0, 0.0, 0.0), boxes, [4, 2, 4], goals, bd)["status"] == R.INVALID
    boxes[2, :4] = sq(0.0, 0.0)
    assert R.plan((0.0, 0.0, 0.0), boxes, [4, 0, 4], goals, bd, n_max=0)["status"] == R.CAP
    # the tracker: NaN and an untouched state for a short path or a bad pose; (0, 0) past the end
    path = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    a, d, st = R.track(path, 1, (0.0, 0.0, 0.0), (1, 9.0, 9.0), 1.0, 1.0)
    assert math.isnan(a[0]) and d == -1 and st == (1, 9.0, 9.0)
    assert R.track(path, 3, (0.0, math.inf, 0.0), (1, 9.0, 9.0), 1.0, 1.0)[1] == -1
    assert R.track(path, 3, (0.0, 0.0, 0.0), (3, 9.0, 9.0), 1.0, 1.0) == ((0.0, 0.0), 3, (3, 9.0, 9.0))
    a, d, st = R.track(path, 3, (0.7, 0.0, 0.0), (1, 1.0, 0.0), 0.2, 0.1)
    assert d == 2 and st == (2, 2.0, 0.0) and a[0] == 1.0 and a[1] == 0.0
    assert R.track(path, 3, (1.7, 0.0, 0.0), st, 0.2, 0.1) == ((0.0, 0.0), 3, (3, 2.0, 0.0))


def test_boundary_goals():
    from benchpush_amd.config import default_cfg, merge_user_cfg
    from benchpush_amd.planning import boundary_goals
    for name in ("clear_env_small", "clear_env", "walled_env", "walled_env_with_columns"):
        c = merge_user_cfg(default_cfg("area_clearing"), {"env": name})
        lay = c.envs[c.env]
        bd = np.asarray(lay.boundary, np.float64)
        g = boundary_goals(lay.boundary, lay.walls if "walls" in lay else [])
        assert g.shape == (len(bd), 2, 2) == (4, 2, 2)
        assert np.array_equal(g[:, 0], bd) and np.array_equal(g[:, 1], np.roll(bd, -1, 0))            # the four whole edges
    # a wall crossing the first edge at y = -4.85: the cut is +-0.1 around it, the piece below is 0.05 long and dropped
    bd = [[-5.0, -5.0], [-5.0, 5.0], [5.0, 5.0], [5.0, -5.0]]
    g = boundary_goals(bd, [[[-6.0, -4.85], [-4.0, -4.85]]])
    assert g.shape == (4, 2, 2) and np.array_equal(g[1:, 0], np.asarray(bd)[1:])
    assert np.allclose(g[0], [[-5.0, -4.75], [-5.0, 5.0]], atol=1e-12)
    g = boundary_goals(bd, [[[-6.0, 1.0], [-4.0, 1.0]]])                                                # in the middle: two pieces
    assert g.shape == (5, 2, 2) and np.allclose(g[:2], [[[-5.0, -5.0], [-5.0, 0.9]], [[-5.0, 1.1], [-5.0, 5.0]]], atol=1e-12)
    # a wall that ends 0.06 short of the edge: the round cap takes sqrt(0.1^2 - 0.06^2) = 0.08 to either side
    g = boundary_goals(bd, [[[-4.94, 0.0], [-3.0, 0.0]]])
    assert g.shape == (5, 2, 2) and np.allclose([g[0, 1, 1], g[1, 0, 1]], [-0.08, 0.08], atol=1e-12)
    assert boundary_goals(bd, [[[-4.8, 0.0], [-3.0, 0.0]]]).shape == (4, 2, 2)                           # 0.2 away: nothing cut


def test_config_validation_and_abi():
    from benchpush_amd import _lib
    from benchpush_amd.planning import GTSPConfig, GTSPPlan, GTSPTrackerState    # noqa: F401
    c = GTSPConfig()
    assert c.as_dict() == dict(R.DEFAULTS, num_goals=None)
    for bad in (dict(shrink=-0.1), dict(extend=math.nan), dict(dt=0.0), dict(round_decimals=16), dict(max_boxes=0), dict(num_goals=0),
                dict(v_scale=0.0), dict(w_scale=math.inf), dict(lin_vel=-1.0)):
        with pytest.raises(ValueError):
            GTSPConfig(**bad)
    s = GTSPConfig(v_scale=0.2, w_scale=0.1).as_struct(num_goals=4)
    assert (s.max_boxes, s.num_goals, s.round_decimals, s.shrink, s.extend, s.ang_vel) == (10, 4, 7, 0.4, 2.0, math.pi / 4)
    for name in ("bp_sizeof_gtsp_config", "bp_gtsp_workspace_bytes", "bp_gtsp_plan", "bp_gtsp_track"):
        assert name in _lib.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "benchpush_amd.h")).read()
    assert "#define BP_ABI_VERSION 11" in header and "bp_gtsp_plan(" in header and "bp_gtsp_track(" in header and "bp_gtsp_workspace_bytes(" in header
    assert (_lib.GTSP_OK, _lib.GTSP_NOTHING_TO_PUSH, _lib.GTSP_SKIPPED, _lib.GTSP_CAP, _lib.GTSP_INVALID) == (R.OK, R.NOTHING_TO_PUSH, R.SKIPPED, R.CAP, R.INVALID)
    assert (_lib.GTSP_FLAG_VANISHED, _lib.GTSP_FLAG_DEGENERATE) == (R.FLAG_VANISHED, R.FLAG_DEGENERATE)
    if os.path.exists(_lib.LIB_PATH):
        import ctypes as C
        L = _lib.load()
        assert L.bp_abi_version() == 11 and L.bp_sizeof_gtsp_config() == C.sizeof(_lib.BpGtspConfig) == 96
        assert L.bp_gtsp_workspace_bytes(C.byref(s), 3) == 3 * 1024 * 40 * 4
        for k, v in (("max_boxes", 13), ("num_goals", 9), ("max_boxes", 0), ("round_decimals", -1)):
            t = GTSPConfig(v_scale=0.2, w_scale=0.1).as_struct(num_goals=4)
            setattr(t, k, v)
            assert L.bp_gtsp_workspace_bytes(C.byref(t), 3) < 0
        assert L.bp_gtsp_workspace_bytes(C.byref(s), 0) < 0


def test_policy_module_imports_without_a_gpu():
    from benchpush_amd.baselines.area_clearing.planning_based.policy import PlanningBasedPolicy
    p = PlanningBasedPolicy(glns_executable_path="/nowhere/GLNS", cfg=None)
    assert p.path is None and p.glns_executable_path == "/nowhere/GLNS"
    bd = [[-5.0, -5.0], [-5.0, 5.0], [5.0, 5.0], [5.0, -5.0]]
    p.update_boundary_and_obstacles(bd, [], [])
    assert np.asarray(p.boundary_goals).shape == (4, 2, 2)
    p.path = np.zeros((3, 3))
    p.reset()
    assert p.path is None
