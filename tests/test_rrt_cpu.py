"""The batched RRT and its controller without a GPU: the restatement (tests/rrt_ref.py) against the goldens recorded from the reference's own
``_run_rrt``, ``prune_by_distance`` and ``DP.ideal_control``; its predicates on hand-built cases; the edge rules; the ABI pieces and the policy's
refusal."""
import ctypes as C
import hashlib
import math
import os
import random

import numpy as np
import pytest

import rrt_ref as R

ROOM = [[0, 0, 4, 0], [4, 0, 4, 3], [4, 3, 0, 3], [0, 3, 0, 0]]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(), np.load(os.path.join(R.GOLDEN, "rrt_golden.npz"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_golden_covers_what_it_should(golden):
    G, A = golden
    runs = {r["name"]: r for r in G["runs"]}
    assert all(r["restatement_agrees"] and r["argmin_diff"] == 0 for r in G["runs"])      # hypot-argmin and d2-argmin never named different nodes
    m1, m2, m3 = runs["maze1_layout0"], runs["maze2_layout0"], runs["maze1_layout1"]
    assert all(r["cfg"]["step"] == 0.05 and r["cfg"]["max_nodes"] == 26000 and r["seed"] == 42 for r in (m1, m2, m3))
    assert m1["status"] == R.FOUND and m1["passes"][0]["iterations"] > 3000 and m1["raw_points"] == 526
    assert m2["status"] == R.FOUND and m2["passes"][0]["iterations"] > 12000 and m2["raw_points"] == 1021
    assert m3["status"] == R.FOUND_IGNORING_BOXES and m3["passes"][0]["iterations"] == 26000        # pass 0 uses up its nodes, pass 1 finds
    small = [r for r in G["runs"] if r["cfg"]["step"] == 0.25 and r["cfg"]["max_nodes"] == 2000]
    assert len(small) >= 5 and {r["status"] for r in small} == {R.FOUND, R.FOUND_IGNORING_BOXES, R.FALLBACK}
    for f in ("rrt_golden.json", "rrt_golden.npz"):
        assert os.path.getsize(os.path.join(R.GOLDEN, f)) <= os.path.getsize(os.path.join(R.GOLDEN, "track_golden.json"))


def test_restatement_reproduces_the_reference_runs(golden):
    """The recorded draws (random.Random(seed), in order) through the sampler hook, the reference's arithmetic (hypot): node lists, parents, raw and
    pruned paths with ==.  Trees above 4000 nodes are recorded as sha256 of their bytes."""
    G, A = golden
    for r in G["runs"]:
        rng, used = random.Random(r["seed"]), []

        def sampler(p, k, j):
            used.append(rng.random())
            return used[-1]

        sc = r["scene"]
        got = R.rrt_plan(sc["start"], sc["goal"], sc["walls"], sc["boxes"], 0, dict(r["cfg"], inflate_radius=sc["inflate_radius"], max_waypoints=1 << 20),
                         sampler=sampler, hypot=math.hypot)
        assert len(used) == r["n_draws"] and used[:4] == r["first_draws"] and used[-4:] == r["last_draws"], r["name"]
        assert got["status"] == r["status"], r["name"]
        for p, rec in enumerate(r["passes"]):
            assert got["iterations"][p] == rec["iterations"] and got["n_nodes"][p] == rec["n_nodes"], (r["name"], p)
        nodes, parents = np.asarray(got["nodes"], np.float64), np.asarray(got["parents"], np.int32)
        assert _sha(nodes) == r["nodes_sha256"] and _sha(parents) == r["parents_sha256"], r["name"]
        if r["full_tree"]:
            assert np.array_equal(nodes, A[r["name"] + "/nodes"]) and np.array_equal(parents, A[r["name"] + "/parents"])
        if r["status"] != R.FALLBACK:
            assert np.array_equal(np.asarray(got["raw"]), A[r["name"] + "/raw"]), r["name"]
        assert np.array_equal(np.asarray(got["path"]), A[r["name"] + "/pruned"]), r["name"]


def test_device_arithmetic_stays_next_to_the_reference(golden):
    """The kernel's form (sqrt of the summed squares where the reference calls hypot) on the same draws: the same tree shape on the small scenes, the
    nodes within a few ulp."""
    G, A = golden
    for r in G["runs"]:
        if not r["full_tree"] or r["cfg"]["step"] != 0.25:
            continue
        rng = random.Random(r["seed"])
        sc = r["scene"]
        got = R.rrt_plan(sc["start"], sc["goal"], sc["walls"], sc["boxes"], 0, dict(r["cfg"], inflate_radius=sc["inflate_radius"]),
                         sampler=lambda p, k, j: rng.random())
        assert got["status"] == r["status"] and got["parents"] == A[r["name"] + "/parents"].tolist(), r["name"]
        assert np.abs(np.asarray(got["nodes"]) - A[r["name"] + "/nodes"]).max() <= 1e-12


def test_predicates_on_hand_built_cases():
    wall = ((0.0, 0.0), (4.0, 0.0))
    Rr = 0.5
    # a segment touching the capsule exactly at R: parallel above the wall, and end-on beyond its end (binary fractions, so the expected values are exact)
    assert R.seg_seg_d2((1.0, 0.5), (3.0, 0.5), *wall) == Rr * Rr
    assert R.seg_seg_d2((4.375, 0.5), (5.0, 2.0), *wall) == 0.390625 and R.seg_seg_d2((4.5, 0.0), (6.0, 0.0), *wall) == Rr * Rr
    sc = R.Scene([[0, 0, 4, 0]], [], Rr)
    assert sc.static_hit((1.0, 0.5), (3.0, 0.5)) and sc.static_hit((4.5, 0.0), (6.0, 0.0))          # closed: touching counts
    assert not sc.static_hit((1.0, 0.5000001), (3.0, 0.5000001)) and not sc.static_hit((4.5000001, 0.0), (6.0, 0.0))
    assert sc.blocked((2.0, -0.5)) and not sc.blocked((2.0, -0.5000001))
    # crossing a wall: distance 0, also where all four end points are far from the other segment
    assert R.seg_meet((2.0, -3.0), (2.0, 3.0), *wall) and R.seg_seg_d2((2.0, -3.0), (2.0, 3.0), *wall) == 0.0
    assert R.Scene([[0, 0, 4, 0]], [], 0.0).static_hit((2.0, -3.0), (2.0, 3.0))
    assert not R.seg_meet((5.0, -3.0), (5.0, 3.0), *wall)
    # collinear: overlapping, touching end to end, apart
    assert R.seg_meet((1.0, 0.0), (6.0, 0.0), *wall) and R.seg_meet((4.0, 0.0), (6.0, 0.0), *wall) and not R.seg_meet((4.5, 0.0), (6.0, 0.0), *wall)
    assert R.seg_seg_d2((1.0, 0.0), (6.0, 0.0), *wall) == 0.0 and R.seg_seg_d2((5.0, 0.0), (6.0, 0.0), *wall) == 1.0
    # T junction: an end point on the other segment
    assert R.seg_meet((2.0, 0.0), (2.0, 1.0), *wall) and R.seg_meet((2.0, 1.0), (2.0, 0.0), *wall)
    # boxes: either winding; an end point on an edge and on a vertex is a hit, just outside is not
    sq = [(1.0, 1.0), (2.0, 1.0), (2.0, 2.0), (1.0, 2.0)]
    for poly in (sq, sq[::-1]):
        b = R.Scene([], [poly], 0.0)
        assert b.movable_hit((0.0, 1.5), (1.0, 1.5)) and b.movable_hit((0.0, 0.0), (1.0, 1.0)) and b.movable_hit((1.5, 1.5), (1.6, 1.6))
        assert not b.movable_hit((0.0, 1.5), (0.999999, 1.5)) and b.movable_hit((0.0, 1.5), (3.0, 1.5)) and b.movable_hit((0.0, 2.0), (3.0, 2.0))
        assert R.point_in_poly((1.0, 1.5), poly) and R.point_in_poly((2.0, 2.0), poly) and not R.point_in_poly((2.0000001, 2.0), poly)
        assert b.seg_hit((0.0, 1.5), (3.0, 1.5), True) == "movable" and b.seg_hit((0.0, 1.5), (3.0, 1.5), False) == "none"
    # a degenerate segment is a point
    assert R.seg_meet((2.0, 0.0), (2.0, 0.0), *wall) and not R.seg_meet((2.0, 0.1), (2.0, 0.1), *wall)
    assert R.seg_seg_d2((2.0, 0.3), (2.0, 0.3), *wall) == 0.3 * 0.3 and R.seg_seg_d2((2.0, 0.3), (2.0, 0.3), (1.0, 0.3), (1.0, 0.3)) == 1.0
    assert R.Scene([], [sq], 0.0).movable_hit((1.5, 1.5), (1.5, 1.5)) and not R.Scene([], [sq], 0.0).movable_hit((0.5, 1.5), (0.5, 1.5))
    assert R.Scene([], [], 0.1).bounds == (-3.0, 3.0, -3.0, 3.0) and R.Scene([[0, 1, 4, -2]], [sq, []], 0.1).bounds == (0.0, 4.0, -2.0, 2.0)


def test_edge_rules_and_statuses():
    cfg = dict(step=0.25, max_nodes=300, inflate_radius=0.2, max_waypoints=64)
    ok = R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [], 7, cfg)
    assert ok["status"] == R.FOUND and ok["path"][0] == (0.5, 0.5) and ok["path"][-1] == (3.5, 2.5) and ok["n_nodes"][1] == ok["iterations"][1] == 0
    assert ok["nodes"][-1] == (3.5, 2.5) and ok["parents"][-1] == len(ok["nodes"]) - 2 and ok["n_nodes"][0] == len(ok["nodes"])
    assert R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [], 7, cfg) == ok and R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [], 8, cfg)["nodes"] != ok["nodes"]
    # prune: consecutive waypoints at least min_dist apart, and none but the last within min_dist of the goal
    pr = ok["path"]
    assert all(math.dist(a, b) >= 0.3 for a, b in zip(pr[:-2], pr[1:-1])) and all(math.dist(a, pr[-1]) >= 0.3 for a in pr[1:-1])
    # _densify: a = dense[-1]; n = max(1, int(L / ds)) points per edge
    assert R.densify([(0.0, 0.0), (0.25, 0.0), (0.25, 0.1)], 0.08) == [(0.0, 0.0), (0.25 / 3, 0.0), (2 / 3 * 0.25, 0.0), (0.25, 0.0), (0.25, 0.1)]
    # BLOCKED: start or goal within the inflated walls -- no search, the reference's [start, goal]
    for s, g in (((0.2, 1.0), (3.5, 2.5)), ((0.5, 0.5), (3.9, 2.5))):
        b = R.rrt_plan(s, g, ROOM, [], 7, cfg)
        assert b["status"] == R.BLOCKED and b["path"] == [s, g] and b["n_nodes"] == [0, 0] and b["iterations"] == [0, 0]
    # FALLBACK: a wall between them; both passes use up max_nodes; two points
    f = R.rrt_plan((0.7, 1.5), (3.3, 1.5), ROOM + [[2, 0, 2, 3]], [], 7, cfg)
    assert f["status"] == R.FALLBACK and f["path"] == [(0.7, 1.5), (3.3, 1.5)] and f["iterations"] == [300, 300]
    assert R.rrt_plan((0.7, 1.5), (3.3, 1.5), ROOM + [[2, 0, 2, 3]], [], 7, dict(cfg, passes=1))["iterations"] == [300, 0]
    # CAP: more waypoints than rows
    c = R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [], 7, dict(cfg, max_waypoints=len(pr) - 1))
    assert c["status"] == R.CAP and c["path"] == [] and c["cap_prefix"] == pr[:-1]
    assert R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [], 7, dict(cfg, max_waypoints=len(pr)))["status"] == R.FOUND
    # BAD_INPUT
    assert R.rrt_plan((math.nan, 0.5), (3.5, 2.5), ROOM, [], 7, cfg)["status"] == R.BAD_INPUT
    assert R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [[(1, 1), (math.inf, 1), (2, 2)]], 7, cfg)["status"] == R.BAD_INPUT
    assert R.rrt_plan((0.5, 0.5), (3.5, 2.5), ROOM, [[(1, 1), (2, 2)]], 7, cfg)["status"] == R.BAD_INPUT
    # the batch: inactive envs are SKIPPED with nothing written; a plan does not depend on the env's place
    starts, goals = np.array([[0.5, 0.5]] * 3), np.array([[3.5, 2.5]] * 3)
    st, nn, it, paths, lengths, _ = R.rrt_plan_batch(starts, goals, ROOM, np.zeros((3, 1, 4, 2)), np.zeros((3, 1), np.int32), [9, 7, 7], cfg, [1, 0, 1])
    assert st.tolist() == [R.FOUND, R.SKIPPED, R.FOUND] and lengths[1] == 0 and not paths[1].any() and nn[1].tolist() == [0, 0]
    assert paths[2, :lengths[2]].tolist() == [list(q) for q in pr]


def test_controller_restatement_equals_the_reference(golden):
    G, A = golden
    scale, worst, n = G["action_scale"], 0.0, 0
    assert G["max_action_diff"] <= R.THETA_TOL / (G["track_cfg"]["dt"] * scale)
    for t in G["track"]:
        path = A[t["path"] + "/pruned"]
        for pose, act, idx in zip(t["poses"], t["actions"], t["indices"]):
            a, near_target = R.track_waypoints_ref(path, pose, scale)
            assert list(near_target) == idx, (t["path"], pose)
            worst, n = max(worst, abs(a - act)), n + 1
    print("controller restatement against the reference: largest action difference %.3g over %d calls (the generator saw %.3g with libm)"
          % (worst, n, G["max_action_diff"]))
    assert n >= 160 and worst <= R.THETA_TOL / (G["track_cfg"]["dt"] * scale)
    # edge rules
    line = np.stack([np.arange(10) * 0.1, np.zeros(10)], 1)
    assert R.track_waypoints_ref(line, (0.0, 0.0, 0.0), scale, length=0)[1] == (-1, -1) and math.isnan(R.track_waypoints_ref(line, (math.nan, 0, 0), scale)[0])
    assert R.track_waypoints_ref(line, (0.0, 0.0, 0.0), scale)[1] == (0, 5)            # the first waypoint that is not within Lfc
    assert R.track_waypoints_ref(line, (0.45, 0.0, 0.0), scale)[1] == (4, 9)           # (4 and 5 tie: the first) ... the last waypoint at most
    assert R.track_waypoints_ref(line, (0.8, 0.0, 0.0), scale, cfg=dict(Lfc=0.0))[1] == (8, 8)
    assert R.track_waypoints_ref(line[:1], (1.0, 1.0, 0.0), scale)[1] == (0, 0)


def test_uniform_config_sizes_and_exports():
    from benchpush_amd import _lib
    from benchpush_amd.build import build_hip
    from benchpush_amd.planning import RRTConfig
    build_hip()
    L = _lib.load()
    for seed, stream, p, k, j in [(42, 0, 0, 0, 0), (42, 1, 0, 0, 0), (42, 7 << 32, 1, 25999, 2), (2 ** 64 - 1, -5, 0, 12345, 1), (0, 2 ** 40 + 17, 1, 1, 0)]:
        u = L.bp_rrt_uniform(seed, stream, p, k, j)
        assert u == R.rrt_uniform(seed, stream, p, k, j) and 0.0 <= u < 1.0
    us = [R.rrt_uniform(42, 3, 0, k, j) for k in range(2000) for j in range(3)]
    assert len(set(us)) == len(us) and 0.45 < sum(us) / len(us) < 0.55
    assert R.rrt_uniform(42, 3, 0, 5, 1) != R.rrt_uniform(42, 3, 1, 5, 1) != R.rrt_uniform(42, 4, 1, 5, 1) != R.rrt_uniform(43, 4, 1, 5, 1)
    assert L.bp_sizeof_rrt_config() == C.sizeof(_lib.BpRrtConfig) == 72 and L.bp_sizeof_track_wp_config() == C.sizeof(_lib.BpTrackWpConfig) == 32
    s = RRTConfig(inflate_radius=0.0).as_struct()
    ref = dict(R.DEFAULTS)
    assert {k: getattr(s, k) for k in ref} == ref                                     # the reference's values are the defaults
    assert L.bp_rrt_workspace_bytes(C.byref(s), 3) == 3 * ((26002 * 20 + 15) // 16 * 16)   # 520 KB per env
    for bad in (dict(step=0.0), dict(max_nodes=0), dict(max_waypoints=1), dict(step=200.0, densify_ds=0.001), dict(max_nodes=5000000)):     # the last two: > 2^22 dense points
        assert L.bp_rrt_workspace_bytes(C.byref(RRTConfig(inflate_radius=0.0, **bad).as_struct()), 3) < 0
    names = ["bp_sizeof_rrt_config", "bp_rrt_workspace_bytes", "bp_rrt_uniform", "bp_rrt_plan", "bp_sizeof_track_wp_config", "bp_track_waypoints"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "benchpush_amd.h")).read()
    assert "#define BP_ABI_VERSION 11" in header and L.bp_abi_version() == 11
    for n in names:
        assert n in _lib.EXPORTS and n + "(" in header and hasattr(L, n)
    assert (_lib.RRT_FOUND, _lib.RRT_FOUND_IGNORING_BOXES, _lib.RRT_FALLBACK, _lib.RRT_BLOCKED, _lib.RRT_CAP, _lib.RRT_BAD_INPUT, _lib.RRT_SKIPPED) == (
        R.FOUND, R.FOUND_IGNORING_BOXES, R.FALLBACK, R.BLOCKED, R.CAP, R.BAD_INPUT, R.SKIPPED)


def test_policy_imports_and_refuses_unknown_planners():
    from benchpush_amd.baselines.base_class import BasePolicy
    from benchpush_amd.baselines.maze_NAMO.planning_based.policy import PlanningBasedPolicy
    with pytest.raises(Exception, match="Invalid planner type"):
        PlanningBasedPolicy("lattice")
    p = PlanningBasedPolicy("RRT", planner_config=dict(step=0.25), num_envs=3)
    assert isinstance(p, BasePolicy) and p.path is None and p.env is None and p._config().step == 0.25     # no device is touched before the first call
    p.reset()
