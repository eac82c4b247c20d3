"""bp_track_path / BatchedShipIceEnv.track_paths and PlanningBasedPolicy on the GPU: bit-exact against the scalar restatement (tests/track_ref.py), the
goldens recorded from the reference, untouched rows, guards, refusals and the closed loops of the straight and the lattice baseline."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import track_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, P = 8, 97                                   # P crosses a 64-lane chunk and is no multiple of it
LENGTHS = [0, 1, 2, 64, 65, 97, 97, 97]
YAW_TOL = 1e-10                                # as in test_track_cpu.py


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@pytest.fixture(scope="module")
def env():
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    e = BatchedShipIceEnv(E, cfg={"concentration": 0.1}, trials=default_trials(0.1, 2, base_seed=31), device=DEV)
    e.reset()
    yield e
    e.check_errors()
    e.close()


def make_paths():
    """[E, P, 3]: gentle curves one unit apart; env 7 a straight line; env 5 with sample 41 a copy of sample 40."""
    i = np.arange(P, dtype=np.float64)
    paths = np.zeros((E, P, 3))
    for e in range(E):
        paths[e, :, 0] = 6.0 + (0.0 if e == 7 else 2.0 * np.sin(0.05 * i + e))
        paths[e, :, 1] = i
        paths[e, :, 2] = math.pi / 2
    paths[5, 41] = paths[5, 40]
    return paths


def sentinels():
    return (torch.full((E, 2), -7.25, dtype=torch.float64, device=DEV), torch.full((E,), -7.25, dtype=torch.float64, device=DEV),
            torch.full((E, 4), -9, dtype=torch.int32, device=DEV))


def run(env, paths, state, poses, lengths=None, active=None, config=None, out=None):
    """One device call next to the restatement's; returns (device, reference) as numpy (actions, ct_err, diag, state)."""
    st_d = dev(state)
    out = out or sentinels()
    want = tuple(o.cpu().numpy().copy() for o in out)
    got = env.track_paths(dev(paths), st_d, lengths=None if lengths is None else dev(np.asarray(lengths), torch.int32), poses=dev(poses),
                          active=None if active is None else dev(np.asarray(active, np.uint8)), config=config, out=out)
    torch.cuda.synchronize()
    st_r = np.array(state, np.float64)
    cfg = dict(config.as_dict()) if config is not None else None
    T.track_ref_batch(paths, poses, st_r, env.max_yaw_rate_step, lengths, active, cfg, out=want)
    return tuple(o.cpu().numpy() for o in got) + (st_d.cpu().numpy(),), want + (st_r,)


def same(got, want):
    return all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))


def test_six_consecutive_calls_equal_the_restatement(env):
    paths = make_paths()
    state = np.zeros((E, 4))
    state[0] = (0.5, 0.25, 0.125, 1.0)              # length 0: must stay
    state[6] = (9.9995, 0.1, 0.3, 1.0)              # one step below the integrator cap
    seen = dict(branches=set(), first_pid=False, dead=False, capped=False, near0=False, near_last=False, tie=False)
    for t in range(6):
        poses = np.zeros((E, 3))
        poses[0] = (6.0, 3.0 + t, 1.5)
        poses[1] = (6.0 + 12.0, 0.5 * t, 1.5 if t < 3 else 2.9)            # one sample, 12 away: the carrot is the sample itself
        poses[2] = (5.0 + 0.3 * t, 0.4 * t, 1.2)
        poses[3] = (paths[3, 63, 0] + 0.5, 63.0 + 1.0 + t, 1.6)             # beyond the last counted sample
        poses[4] = (paths[4, 0, 0] - 11.0, -2.0 - t, 1.0 + 0.2 * t)         # before the first sample, far
        poses[5] = (paths[5, 40, 0] + 0.3, 40.2 + 0.1 * t, 1.7)             # nearest: the duplicated sample
        poses[6] = (6.0 + 13.0, 30.0 + 0.6 * t, 1.5)
        poses[7] = (6.0 - 12.5, 20.0 + 0.6 * t, 0.2 if t < 2 else 1.3)      # straight slice: a big yaw error turns at the fixed rate
        if t in (3, 4):   # aim env 6 at its carrot: the PID's dead zone
            jt = T.track_ref(paths[6], poses[6], state[6], env.max_yaw_rate_step)[2][2]
            poses[6, 2] = math.atan2(paths[6, jt, 1] - poses[6, 1], paths[6, jt, 0] - poses[6, 0]) + 0.004 * (t - 3.5)
        before = state.copy()
        got, want = run(env, paths, state, poses, LENGTHS)
        for name, g, w in zip(("actions", "ct_err", "diag", "state"), got, want):
            assert np.array_equal(g, w), (t, name, g, w)
        assert (got[0][0] == -7.25).all() and got[1][0] == -7.25 and (got[2][0] == -9).all() and (got[3][0] == before[0]).all()
        diag, state = want[2], want[3]
        for e in range(1, E):
            br = int(diag[e, 1])
            seen["branches"].add(br)
            seen["first_pid"] |= br == T.PID and before[e, 3] == 0.0 and state[e, 3] == 1.0
            seen["dead"] |= br == T.PID and abs(state[e, 1]) <= 0.02
            seen["capped"] |= br == T.PID and abs(state[e, 0]) == 10.0
            seen["near0"] |= diag[e, 0] == 0 and LENGTHS[e] > 2
            seen["near_last"] |= diag[e, 0] == LENGTHS[e] - 1 and LENGTHS[e] > 2
        seen["tie"] |= diag[5, 0] == 40
    assert seen["branches"] == {T.GENTLE, T.PID, T.NEAR}, seen
    assert all(v for k, v in seen.items() if k != "branches"), seen


def test_shared_path_equals_the_per_env_copy(env):
    paths = make_paths()
    rng = np.random.RandomState(2)
    poses = np.stack([rng.uniform(-8, 20, E), rng.uniform(-5, 100, E), rng.uniform(0, 3, E)], 1)
    state = rng.uniform(0, 0.1, (E, 4))
    state[:, 3] = rng.randint(0, 2, E)
    copies = np.repeat(paths[3:4], E, 0)
    got_c, want_c = run(env, copies, state, poses)
    got_s, want_s = run(env, paths[3], state, poses)
    assert same(got_c, want_c) and same(got_s, got_c)
    assert set(got_c[2][:, 1]) >= {T.NEAR, T.PID}


def test_inactive_and_empty_rows_are_untouched(env):
    paths = make_paths()
    rng = np.random.RandomState(3)
    poses = np.stack([rng.uniform(0, 12, E), rng.uniform(0, 90, E), rng.uniform(0, 3, E)], 1)
    state = rng.uniform(0.01, 0.1, (E, 4))
    active = [1, 0, 1, 0, 1, 1, 0, 1]
    lengths = [5, 97, 0, 0, -3, 97, 20, 200]             # above P: all P count
    got, want = run(env, paths, state, poses, lengths, active)
    assert same(got, want)
    for e in (1, 2, 3, 4, 6):
        assert (got[0][e] == -7.25).all() and got[1][e] == -7.25 and (got[2][e] == -9).all() and np.array_equal(got[3][e], state[e])
    for e in (0, 5, 7):
        assert got[2][e, 1] != 0 and got[1][e] >= 0


def test_non_finite_input_gives_nan_and_keeps_the_state(env):
    paths = make_paths()
    poses = np.tile([7.0, 30.0, 1.5], (E, 1))
    poses[1, 2] = math.nan
    poses[2, 0] = math.inf
    paths[3, 96, 1] = math.nan                            # counted for env 3, not for env 4 (length 65)
    paths[4, 96, 1] = math.nan
    state = np.full((E, 4), 0.0625)
    lengths = [97, 97, 97, 97, 65, 97, 97, 97]
    got, want = run(env, paths, state, poses, lengths)
    assert same(got, want)
    for e in (1, 2, 3):
        assert np.isnan(got[0][e]).all() and np.isnan(got[1][e]) and got[2][e].tolist() == [-1, 0, -1, -1] and np.array_equal(got[3][e], state[e])
    assert np.isfinite(got[0][[0, 4, 5, 6, 7]]).all() and (got[2][[0, 4, 5, 6, 7], 1] == T.NEAR).all()


def test_device_equals_the_reference_goldens(env):
    G = T.load_golden()
    cases = G["cases"]
    Pm = max(len(c["path"]) for c in cases)
    assert abs(G["action_scale"] - env.max_yaw_rate_step) == 0.0
    worst = 0.0
    counted = 0
    for g0 in range(0, len(cases), E):
        group = cases[g0:g0 + E]
        paths, lengths = np.zeros((E, Pm, 3)), np.zeros(E, np.int32)
        for e, c in enumerate(group):
            paths[e, :len(c["path"])], lengths[e] = c["path"], len(c["path"])
        pd, ld = dev(paths), dev(lengths)
        for t in range(len(group[0]["poses"])):
            poses, state = np.zeros((E, 3)), np.zeros((E, 4))
            for e, c in enumerate(group):
                poses[e] = c["poses"][t]
                state[e] = c["state_after"][t - 1] if t else 0.0
            st = dev(state)
            actions, ct, diag = env.track_paths(pd, st, lengths=ld, poses=dev(poses))
            torch.cuda.synchronize()
            actions, diag, st = actions.cpu().numpy(), diag.cpu().numpy(), st.cpu().numpy()
            for e, c in enumerate(group):
                if not c["keep"][t]:
                    continue
                want = T.track_ref(paths[e], poses[e], state[e], G["action_scale"], lengths[e])
                assert tuple(actions[e]) == want[0] and tuple(diag[e]) == want[2] and tuple(st[e]) == want[3]       # the restatement, bit for bit
                assert [int(diag[e, 0]), int(diag[e, 1])] == c["near_branch"][t]
                assert actions[e, 1] == c["out"][t][1] and st[e, 2] == c["state_after"][t][2]
                worst = max(worst, abs(actions[e, 0] - c["out"][t][0]))
                counted += 1
    print("device against the reference: %d calls, worst yaw action difference %.3g" % (counted, worst))
    assert counted == G["calls"] - G["dropped"] and worst <= YAW_TOL


def test_refusals_write_nothing(env):
    from benchpush_amd import _lib
    from benchpush_amd._lib import BpError
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    from benchpush_amd.planning import TrackerConfig
    paths = dev(make_paths())
    poses = dev(np.tile([7.0, 30.0, 1.5], (E, 1)))
    state = torch.full((E, 4), 0.0625, dtype=torch.float64, device=DEV)
    out = sentinels()

    def unchanged():
        torch.cuda.synchronize()
        return bool((out[0] == -7.25).all() and (out[1] == -7.25).all() and (out[2] == -9).all() and (state == 0.0625).all())

    maze = BatchedMazeEnv(E, cfg={"num_obstacles": 20}, num_layouts=2, device=DEV)
    maze.reset()
    with pytest.raises(BpError):
        maze.track_paths(paths, state, poses=poses, out=out)
    maze.close()
    assert unchanged()
    with pytest.raises(BpError):
        env.track_paths(paths[:, :0].contiguous(), state, poses=poses, out=out)                     # P = 0
    with pytest.raises(BpError):
        env.track_paths(paths, state, poses=poses, config=TrackerConfig(dt=0.0), out=out)
    with pytest.raises(BpError):
        env.track_paths(paths, state, poses=poses, config=TrackerConfig(action_scale=-1.0), out=out)
    cfg = _lib.BpTrackConfig(P=P, pad_=0, action_scale=0.2, **TrackerConfig().as_dict())
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    with pytest.raises(BpError):             # a stride shorter than a path
        _lib.check(env.L, env.h, env.L.bp_track_path(env.h, C.byref(cfg), p(paths), 3 * P - 1, None, p(poses), None, p(state), p(out[0]), p(out[1]),
                                                     p(out[2]), env._stream()), "bp_track_path")
    with pytest.raises(BpError):             # a NULL required pointer
        _lib.check(env.L, env.h, env.L.bp_track_path(env.h, C.byref(cfg), p(paths), 3 * P, None, None, None, p(state), p(out[0]), p(out[1]),
                                                     p(out[2]), env._stream()), "bp_track_path")
    assert unchanged()
    for kw in (dict(paths=paths.float()), dict(paths=paths.cpu()), dict(paths=paths.transpose(0, 1)), dict(paths=paths[:, :, :2].contiguous()),
               dict(paths=paths[:3].contiguous()), dict(state=state.float()), dict(state=state[:, :3].contiguous()), dict(state=state.cpu()),
               dict(poses=poses.cpu()), dict(poses=poses[:, :2].contiguous()), dict(lengths=torch.zeros(E, dtype=torch.int64, device=DEV)),
               dict(lengths=torch.zeros(E + 1, dtype=torch.int32, device=DEV)), dict(active=torch.zeros(E, dtype=torch.int32, device=DEV)),
               dict(out=(out[0], out[1], out[2].long())), dict(out=(out[0][:, :1].contiguous(), out[1], out[2]))):
        args = dict(dict(paths=paths, state=state, poses=poses, out=out), **kw)
        with pytest.raises(ValueError):
            env.track_paths(args.pop("paths"), args.pop("state"), **args)
    assert unchanged()
    # and the call that is accepted writes
    env.track_paths(paths, state, poses=poses, out=out)
    assert not unchanged()


def closed_loop_straight(steps=6):
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    pol = PlanningBasedPolicy("straight", cfg={"concentration": 0.1}, num_envs=4, num_trials=2, device=DEV)
    env = pol._ensure_env()
    for _ in range(2):   # turn the ships off the channel's axis first: on it, the straight path's error is exactly zero
        env.step(torch.ones(4, dtype=torch.float64, device=DEV))
    log = []
    for t in range(steps):
        info = env.info[:, :3].cpu().numpy().copy()
        st = pol.tracker.state.cpu().numpy().copy() if pol.tracker is not None else np.zeros((4, 4))
        a = pol.act_batch(env)
        torch.cuda.synchronize()
        want, _, diag = T.track_ref_batch(pol.paths.cpu().numpy(), info, st, env.max_yaw_rate_step, pol.lengths.cpu().numpy())
        assert np.array_equal(a.cpu().numpy(), want[:, 0]), (t, a, want)
        assert np.array_equal(pol.tracker.state.cpu().numpy(), st) and (diag[:, 1] != 0).all()      # st: the restatement's integrators after the call
        obs, rew, term, trunc, _ = env.step(a)
        log.append((a.cpu().numpy().copy(), rew.cpu().numpy().copy(), obs.cpu().numpy().copy()))
        assert not bool((term | trunc).any())
    env.check_errors()
    pol.close()
    return log


def test_closed_loop_straight_baseline_equals_the_restatement_and_repeats():
    first, second = closed_loop_straight(), closed_loop_straight()
    assert any(a.any() for a, _, _ in first)
    for (a1, r1, o1), (a2, r2, o2) in zip(first, second):
        assert np.array_equal(a1, a2) and np.array_equal(r1, r2) and np.array_equal(o1, o2)


def test_closed_loop_lattice_baseline_equals_the_restatement():
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    with open(os.path.join(T.GOLDEN, "lattice_golden.json")) as f:
        s = json.load(f)["set_8"]
    pol = PlanningBasedPolicy("lattice", cfg={"concentration": 0.1}, planner_config={"edges": s["edges"], "turning_radius": s["turning_radius"]},
                              num_envs=2, num_trials=2, device=DEV)
    env = pol._ensure_env()
    for t in range(3):
        info = env.info[:, :3].cpu().numpy().copy()
        st = pol.tracker.state.cpu().numpy().copy() if pol.tracker is not None else np.zeros((2, 4))
        a = pol.act_batch(env)
        torch.cuda.synchronize()
        if t == 0:
            kept = pol.paths.cpu().numpy().copy()
            assert pol.planner.status.tolist() == [0, 0] and int(pol.planner.found) == 2 and (pol.lengths.cpu().numpy() > 64).all()
        assert np.array_equal(pol.paths.cpu().numpy(), kept)                # one plan
        want, _, diag = T.track_ref_batch(kept, info, st, env.max_yaw_rate_step, pol.lengths.cpu().numpy())
        assert np.array_equal(a.cpu().numpy(), want[:, 0]) and (diag[:, 1] != 0).all(), (t, a, want)
        assert np.array_equal(pol.tracker.state.cpu().numpy(), st)
        env.step(a)
    env.check_errors()
    pol.close()


def test_evaluate_returns_the_scores_of_finished_episodes():
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    pol = PlanningBasedPolicy("straight", cfg={"concentration": 0.1}, num_envs=4, num_trials=2, device=DEV)
    eff, effort, rewards, name = pol.evaluate(2)
    pol.close()
    assert name == "Straight Planning" and len(eff) >= 2 and len(eff) == len(effort) == len(rewards)
    assert all(math.isfinite(v) for v in eff + effort + rewards)


def test_single_env_act_keeps_the_reference_shape():
    """act(observation, ship_pos=, goal=, action_scale=) plans once, returns the pair (yaw, surge) and carries its integrators, like the reference's."""
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    G = T.load_golden()
    pol = PlanningBasedPolicy("straight", cfg={"concentration": 0.1}, num_envs=1, num_trials=2, device=DEV)
    scale, goal = (math.pi / 2) / 7, (0, 76.0)
    st = (0.0, 0.0, 0.0, 0.0)
    path = T.golden_straight(G, (2.25, 6.0, 1.4), 76.0)          # what the reference planned from the first pose
    assert len(path) == 8
    seen = set()
    for pose in [(2.25, 6.0, 1.4), (2.4, 6.5, 1.0), (3.1, 7.2, 1.9), (15.0, 12.0, 1.7)]:
        got = pol.act(None, ship_pos=pose, goal=goal, action_scale=scale, conc=0.1, obstacles=None)
        assert np.array_equal(pol.path, path)                     # planned at the first call, kept afterwards
        want, _, diag, st = T.track_ref(path, pose, st, scale)
        assert isinstance(got, tuple) and got == want, (pose, got, want, diag)
        seen.add(diag[1])
    assert seen == {T.NEAR, T.PID}
    pol.reset()
    assert pol.path is None
    one = T.golden_straight(G, (3.0, 71.0, 1.2), 76.0)            # a path of one sample
    assert len(one) == 1
    again = pol.act(None, ship_pos=(3.0, 71.0, 1.2), goal=goal, action_scale=scale, dt=0.01)
    assert np.array_equal(pol.path, one) and again == T.track_ref(one, (3.0, 71.0, 1.2), (0.0,) * 4, scale, cfg={"dt": 0.01})[0]
    pol.close()


def test_lattice_plan_path_refuses_a_pose_that_is_not_the_envs():
    from benchpush_amd.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy
    with open(os.path.join(T.GOLDEN, "lattice_golden.json")) as f:
        s = json.load(f)["set_8"]
    pol = PlanningBasedPolicy("lattice", cfg={"concentration": 0.1}, planner_config={"edges": s["edges"], "turning_radius": s["turning_radius"]},
                              num_envs=1, num_trials=2, device=DEV)
    env = pol._ensure_env()
    x, y, yaw = env.info[0, :3].cpu().tolist()
    with pytest.raises(ValueError):
        pol.act(None, ship_pos=(x + 1.0, y, yaw), goal=env.goal, action_scale=env.max_yaw_rate_step)
    assert pol.path is None
    rounded = (round(x, 2), round(y, 2), round(yaw, 2))           # info['state'] of the gym-shaped env
    got = pol.act(None, ship_pos=rounded, goal=env.goal, action_scale=env.max_yaw_rate_step)
    assert len(pol.path) > 64 and got == T.track_ref(pol.path, rounded, (0.0,) * 4, env.max_yaw_rate_step)[0]
    pol.close()


def test_named_edge_cases_on_the_device(env):
    """The cases of test_track_cpu.py::test_restatement_edge_rules through the kernel: a path of one sample, the indices at which the walks stop, the
    carrot that ends at the last sample, the duplicated nearest sample, a non-finite sample beyond the counted ones and among them."""
    Pn = 50
    line = np.stack([np.zeros(Pn), np.arange(float(Pn)), np.zeros(Pn)], 1)
    dup = np.zeros((Pn, 3))
    dup[:4] = [[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 3.0, 0.0]]
    bad = np.zeros((Pn, 3))
    bad[1] = [math.inf, 1.0, 0.0]
    paths = np.stack([line, line, line, dup, bad, bad, line, line])
    lengths = [1, Pn, Pn, 4, 1, 2, 0, 0]
    poses = np.array([[3.0, 4.0, 0.0], [0.0, 20.2, 1.5], [12.0, 20.2, 1.5], [0.3, 1.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    state = np.zeros((E, 4))
    got, want = run(env, paths, state, poses, lengths)
    assert same(got, want)
    actions, ct, diag, st = got
    assert ct[0] == 5.0 and diag[0].tolist() == [0, T.NEAR, 0, 0] and actions[0].tolist() == [0.0, 50.0]      # one sample: yaw_ref = atan2(0, 0) = 0
    assert diag[1].tolist() == [20, T.NEAR, 45, 5]                # 25 ahead and 15 back of sample 20, one unit per segment
    assert diag[2, 1] in (T.GENTLE, T.PID) and diag[2, 2] == 49   # the carrot, 50 ahead, ends at the last sample
    assert diag[3, 0] == 1                                        # the smaller index of the duplicated nearest sample
    assert diag[4, 1] == T.NEAR and np.isfinite(actions[4]).all() # the infinite sample is not counted
    assert np.isnan(actions[5]).all() and diag[5].tolist() == [-1, 0, -1, -1] and not st[5].any()
    assert (actions[6:] == -7.25).all() and (diag[6:] == -9).all()
