"""Path tracking without a GPU: the restatement (tests/track_ref.py) against the goldens recorded from the reference's own PlanningBasedPolicy.act,
straight_paths against the reference's straight_planner, the ABI pieces and the policy's refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import track_ref as T

YAW_TOL = 1e-10   # only trig differences of a few ulp of pi enter; through kd / dt / action_scale = 2 * 200 / 0.224 they give about 5e-12


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


def test_golden_was_generated_within_its_limits(golden):
    G = golden
    assert len(G["cases"]) >= 40 and G["calls"] == sum(len(c["poses"]) for c in G["cases"])
    assert G["dropped"] <= 0.02 * G["calls"] and G["dropped"] == sum(not k for c in G["cases"] for k in c["keep"])
    assert min(G["kept_by_branch"].values()) >= 30
    lengths = [len(c["path"]) for c in G["cases"]]
    assert min(lengths) == 2 and max(lengths) >= 390 and {c["spacing"] for c in G["cases"]} == {0.02, 0.5, 2.0}
    # the largest differences between the restatement (libm) and the reference that the generator saw
    print("generator: max yaw / surge / state difference", G["max_yaw_diff"], G["max_surge_diff"], G["max_state_diff"])
    assert G["max_yaw_diff"] <= YAW_TOL and G["max_surge_diff"] == 0.0


def test_restatement_equals_the_reference_call_by_call(golden):
    G = golden
    seen = {T.GENTLE: 0, T.PID: 0, T.NEAR: 0}
    worst_yaw = worst_state = 0.0
    first_pid = dead = 0
    for c in G["cases"]:
        path = np.asarray(c["path"])
        before = [0.0, 0.0, 0.0, 0.0]
        for pose, out, after, keep, (ri, rb) in zip(c["poses"], c["out"], c["state_after"], c["keep"], c["near_branch"]):
            if keep:
                (yaw, surge), ct, diag, st = T.track_ref(path, pose, before, G["action_scale"])
                assert diag[0] == ri and diag[1] == rb, (pose, diag, ri, rb)
                assert surge == out[1] and st[2] == after[2] and st[3] == after[3]
                worst_yaw = max(worst_yaw, abs(yaw - out[0]))
                worst_state = max(worst_state, abs(st[0] - after[0]), abs(st[1] - after[1]))
                seen[rb] += 1
                if rb == T.PID:
                    first_pid += before[3] == 0.0
                    dead += abs(st[1]) <= 0.02
            before = after
    print("restatement against the reference: worst yaw action difference %.3g, worst integrator difference %.3g; calls per branch %s; "
          "first PID calls %d, dead-zone calls %d" % (worst_yaw, worst_state, seen, first_pid, dead))
    assert worst_yaw <= YAW_TOL
    assert worst_state <= 1e-12      # yaw_err itself, and its integral: a few ulp of pi
    assert min(seen.values()) >= 30 and first_pid > 0 and dead > 0


def test_restatement_edge_rules():
    path = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 3.0, 0.0]])
    st = (0.25, -0.5, 0.125, 1.0)
    assert T.track_ref(path, (0.0, 0.0, 1.0), st, 0.2, length=0) is None
    a, ct, diag, st2 = T.track_ref(path, (math.nan, 0.0, 1.0), st, 0.2)
    assert all(math.isnan(v) for v in a) and math.isnan(ct) and diag == (-1, T.NONE, -1, -1) and st2 == st
    a, ct, diag, st2 = T.track_ref(np.array([[0.0, 0.0, 0.0], [math.inf, 1.0, 0.0]]), (0.0, 0.0, 1.0), st, 0.2)
    assert math.isnan(a[0]) and st2 == st
    assert T.track_ref(np.array([[0.0, 0.0, 0.0], [math.inf, 1.0, 0.0]]), (0.0, 0.0, 1.0), st, 0.2, length=1)[2][1] == T.NEAR
    # the duplicated nearest sample: the smaller index wins
    assert T.track_ref(path, (0.3, 1.0, 1.0), st, 0.2)[2][0] == 1
    # one sample: both walks stay put, yaw_ref = atan2(0, 0) = 0
    a, ct, diag, _ = T.track_ref(path[:1], (3.0, 4.0, 0.0), (0.0, 0.0, 0.0, 0.0), 0.2)
    assert ct == 5.0 and diag == (0, T.NEAR, 0, 0) and a[0] == 0.0 and a[1] == 20.0 * 2.5
    # the walks stop at the first sample at or beyond the limit
    line = np.stack([np.zeros(50), np.arange(50.0), np.zeros(50)], 1)
    assert T.track_ref(line, (0.0, 20.2, 1.5), (0.0,) * 4, 0.2)[2] == (20, T.NEAR, 45, 5)
    assert T.track_ref(line, (12.0, 20.2, 1.5), (0.0,) * 4, 0.2)[2][2] == 49       # the carrot, 50 ahead, ends at the last sample


def test_straight_paths_equal_the_reference_planner(golden):
    from benchpush_amd.planning import straight_paths
    for dy in sorted({s["dy"] for s in golden["straight"]}):
        S = [s for s in golden["straight"] if s["dy"] == dy]
        paths, lengths = straight_paths(torch.tensor([s["pose"] for s in S], dtype=torch.float64),
                                        torch.tensor([s["goal_y"] for s in S], dtype=torch.float64), dy)
        assert lengths.dtype == torch.int32 and paths.shape == (len(S), max(1, max(len(s["path"]) for s in S)), 3)
        for i, s in enumerate(S):
            want = np.asarray(s["path"], np.float64).reshape(-1, 3)
            assert int(lengths[i]) == len(want)
            assert np.array_equal(paths[i, :len(want)].numpy(), want), (s["pose"], s["goal_y"])
            assert not paths[i, len(want):].any()
    on, off = golden["straight"][0], golden["straight"][1]
    assert on["path"][-1][1] == on["goal_y"] and all(q[1] != off["goal_y"] for q in off["path"])   # goal_y on and off the dy grid
    assert any(len(s["path"]) == 0 for s in golden["straight"])                                 # a start beyond the goal: no samples
    # max_len: nothing is read back, longer paths are cut
    p2, l2 = straight_paths(torch.tensor([[1.0, 2.0, 1.5]], dtype=torch.float64), 32.0, 10, max_len=3)
    assert p2.shape == (1, 3, 3) and l2.tolist() == [3] and p2[0, :, 1].tolist() == [2.0, 12.0, 22.0]
    with pytest.raises(ValueError):
        straight_paths(torch.zeros(3, dtype=torch.float64), 1.0)


def test_tracker_state_and_config():
    from benchpush_amd.planning import TrackerConfig, TrackerState
    assert TrackerConfig().as_dict() == T.DEFAULTS and TrackerConfig().action_scale is None
    assert TrackerConfig(kp=0.3, action_scale=2).kp == 0.3
    st = TrackerState(3, "cpu")
    assert st.state.shape == (3, 4) and st.state.dtype == torch.float64 and not st.state.any()
    st.state += 1.0
    cl = st.clone()
    st.reset(torch.tensor([True, False, True]))
    assert st.state[:, 0].tolist() == [0.0, 1.0, 0.0] and bool((cl.state == 1.0).all())
    assert not st.reset().state.any() and st.to("cpu").state.device.type == "cpu"


def test_track_config_layout_matches_the_library():
    from benchpush_amd import _lib
    from benchpush_amd.build import build_hip
    build_hip()
    L = _lib.load()
    assert L.bp_sizeof_track_config() == C.sizeof(_lib.BpTrackConfig) == 152
    assert [n for n, _ in _lib.BpTrackConfig._fields_][2:19] == list(T.DEFAULTS)
    assert "bp_sizeof_track_config" in _lib.EXPORTS and "bp_track_path" in _lib.EXPORTS and L.bp_abi_version() == 11
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "benchpush_amd.h")).read()
    assert "#define BP_ABI_VERSION 11" in header and "bp_track_path(" in header and "bp_sizeof_track_config(" in header


def test_policy_refuses_unknown_and_predictive_planners(golden):
    from benchpush_amd.baselines.base_class import BasePolicy
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    with pytest.raises(Exception):
        PlanningBasedPolicy("bogus")
    with pytest.raises(NotImplementedError):
        PlanningBasedPolicy("predictive")
    p = PlanningBasedPolicy("straight", num_envs=3)
    assert isinstance(p, BasePolicy) and p.path is None and p.env is None      # no device is touched before the first call
    for s in golden["straight"]:          # the single-env planner is straight_paths for a batch of one: the reference's recorded outputs
        got = p.straight_planner(tuple(s["pose"]), (0, s["goal_y"]), s["dy"])
        assert got.shape == (len(s["path"]), 3) and np.array_equal(got, np.asarray(s["path"], np.float64).reshape(-1, 3))
