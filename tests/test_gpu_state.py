"""Save, restore and clone of environment state on the device (-m gpu): bp_save_state / bp_load_state / bp_clone_state through the Python surface.

Bar: bit-exact.  A restored or cloned env continues exactly as the saved one would have, so every comparison is torch.equal / np.array_equal -- no
tolerance anywhere.  Every test also asserts that its window is not idle (bodies move, episodes end), so that "equal" is not "nothing happened".
"""
import functools
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCHES = ("BP_SCHED", "BP_SCHED_IMAGE", "BP_SCHED_YMASK", "BP_SCHED_PERSIST", "BP_PAIR", "BP_PAIR_RESIDENT")


@functools.lru_cache(maxsize=None)
def _trials(conc=0.3, n=3, seed=5):
    from benchpush_amd.envs.ship_ice import default_trials
    return default_trials(conc, n, base_seed=seed)


def _ship(E=8, conc=0.3, trials=None, **cfg):
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    return BatchedShipIceEnv(E, cfg=dict({"concentration": conc}, **cfg), trials=_trials(conc) if trials is None else trials, device=DEV)


def _actions(steps, E, seed, dim=1):
    """seeded actions in [-1, 1], rounded through float32 as a learner's would be"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (steps, E) if dim == 1 else (steps, E, dim)).astype(np.float32).astype(np.float64)
    return torch.from_numpy(a).to(DEV)


def _snap(env, box=False):
    """Everything a caller can read from the env right now, as private copies."""
    out = {n: getattr(env, n).clone() for n in ("obs", "reward", "terminated", "truncated", "info")}
    out["bodies"] = env.body_state().clone()
    verts, cnt = env.world_polys()
    out["poly_verts"], out["poly_counts"] = verts.clone(), cnt.clone()
    out["num_bodies"] = torch.from_numpy(env.num_bodies().copy())
    if box:
        alive, wp, nwp = env.box_state()
        out["alive"], out["waypoints"], out["nwp"] = torch.from_numpy(alive.copy()), torch.from_numpy(wp.copy()), torch.from_numpy(nwp.copy())
    else:
        ring, sums, counts = env.episode_history()
        out["ep_ring"], out["ep_sums"], out["ep_counts"] = ring.clone(), sums.clone(), counts.clone()
    return out


def _equal(a, b, what, rows=None, other_rows=None):
    """every entry of two snapshots (or two lists of snapshots) is identical; rows / other_rows: compare a[k][rows] with b[k][other_rows]"""
    if isinstance(a, list):
        assert len(a) == len(b)
        for t, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, (what, t), rows, other_rows)
        return
    assert a.keys() == b.keys()
    for k in a:
        x = a[k] if rows is None else a[k][rows]
        y = b[k] if rows is None else b[k][rows if other_rows is None else other_rows]
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, k)


def _window(env, acts, reset_env=None, reset_after=1, box=False):
    """Step through acts, recording everything after every step; after step `reset_after` the env `reset_env` is reset by the caller (a truncation: it
    writes a metrics row and advances the trial) and everything is recorded again."""
    rec = []
    for t in range(acts.shape[0]):
        env.step(acts[t])
        rec.append(_snap(env, box))
        if reset_env is not None and t == reset_after:
            mask = torch.zeros(env.num_envs, dtype=torch.uint8, device=DEV)
            mask[reset_env] = 1
            env.reset(mask)
            rec.append(_snap(env, box))
    return rec


def _rewind(env, pre, win, seed, reset_env=2, box=False, dim=1):
    """reset, `pre` steps, save, a window of `win` steps with a forced reset, restore, the same window again: identical, and not idle."""
    acts = _actions(pre + win, env.num_envs, seed, dim)
    env.reset()
    at_reset = _snap(env, box)
    for t in range(pre):
        env.step(acts[t])
    at_save = _snap(env, box)
    s = env.save_state()
    first = _window(env, acts[pre:], reset_env, box=box)
    assert not torch.equal(first[-1]["bodies"], at_save["bodies"]), "nothing moved inside the window"
    if reset_env is not None and not box:
        assert not torch.equal(first[-1]["ep_counts"], at_save["ep_counts"]), "no episode ended inside the window"
        assert int(first[-1]["ep_counts"][reset_env]) == int(at_save["ep_counts"][reset_env]) + 1
    env.restore_state(s)
    _equal(_snap(env, box), at_save, "right after the restore")      # output rows included: no step is needed to see the restored state
    second = _window(env, acts[pre:], reset_env, box=box)
    _equal(first, second, "replayed window")
    env.check_errors()
    return s, at_save, first, at_reset


def _fresh(monkeypatch, env_vars):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    gc.collect()


# ---- 1, 2: rewind ------------------------------------------------------------------------------------------------------------------------------
def test_rewind_ship_ice(monkeypatch):
    _fresh(monkeypatch, {})
    env = _ship()
    s = _rewind(env, 3, 4, seed=11)[0]
    assert s.records.shape == (8, env.state_bytes()) and s.records.dtype == torch.uint8 and s.layout_id == env.state_layout_id()
    assert s.obs.shape == env.obs.shape and s.info.shape == env.info.shape
    env.close()


VARIANTS = [({"BP_SCHED": "0"}, {}, lambda e: e.sched_chunk() == 0),
            ({"BP_PAIR": "2"}, {}, lambda e: int(e.L.bp_pair_mode(e.h)) == 2),
            ({}, {"sim": {"damping": 0.9}}, lambda e: e.sched_chunk() == 0),            # the generic kernel has no scheduler
            ({}, {"random_start": True}, lambda e: True)]


@pytest.mark.parametrize("env_vars,cfg,served", VARIANTS, ids=["sched0", "pair2", "damping", "random_start"])
def test_rewind_under_each_step_kernel_variant(monkeypatch, env_vars, cfg, served):
    _fresh(monkeypatch, env_vars)
    env = _ship(**cfg)
    assert served(env), "the handle does not run the variant this case is about"
    _, at_save, first, at_reset = _rewind(env, 3, 4, seed=12)
    if cfg.get("random_start"):
        # env 2 was reset inside the window (snapshot 2 of it): episode 0 came from the first reset, so the forced reset starts episode 1, in the first
        # pass and in the replay -- the start x is the draw of (env 2's own id, the restored episode counter + 1), not the draw of episode 0 again
        u0, u1 = env.start_uniform(2, 0), env.start_uniform(2, 1)
        x0, x1 = float(at_reset["info"][2, 0]), float(first[2]["info"][2, 0])
        assert u0 != u1 and x0 != x1 and (x1 > x0) == (u1 > u0)
    env.close()


# ---- 3: clone across trials, fan-out ------------------------------------------------------------------------------------------------------------
def test_clone_across_trials_and_fan_out(monkeypatch):
    _fresh(monkeypatch, {})
    acts = _actions(6, 8, seed=13)
    after = acts[3:].clone()
    after[:, 1:4] = after[:, 0:1]                                  # envs 1..3 take env 0's actions
    env, ctl = _ship(), _ship()
    for e in (env, ctl):
        e.reset()
        for t in range(3):
            e.step(acts[t])
    before = _snap(env)
    assert not torch.equal(before["bodies"][0], before["bodies"][1]), "envs 0 and 1 hold the same trial"
    assert not torch.equal(before["poly_counts"][0], before["poly_counts"][1])
    env.clone_envs([0, 0, 0], [1, 2, 3])
    now = _snap(env)
    for d in (1, 2, 3):
        _equal(now, now, "clone %d" % d, rows=0, other_rows=d)
    _equal(now, before, "envs that were not named", rows=slice(4, 8))
    for t in range(3):
        env.step(after[t])
        ctl.step(after[t])
        a, c = _snap(env), _snap(ctl)
        for d in (1, 2, 3):
            _equal(a, a, ("clone %d after step" % d, t), rows=0, other_rows=d)
        _equal(a, c, ("control after step", t), rows=slice(4, 8))
        _equal(a, c, ("source after step", t), rows=0)
    assert not torch.equal(a["bodies"][0], before["bodies"][0])
    env.check_errors()
    env.close(); ctl.close()


# ---- 4: one-step look-ahead ---------------------------------------------------------------------------------------------------------------------
def test_lookahead_prediction_is_exact(monkeypatch):
    _fresh(monkeypatch, {})
    env = _ship()
    acts = _actions(4, 8, seed=14)
    env.reset()
    for t in range(3):
        env.step(acts[t])
    s = env.save_state([0])
    env.clone_envs([0] * 7, list(range(1, 8)))
    cand = torch.linspace(-1, 1, 7, dtype=torch.float64, device=DEV).float().double()
    a = torch.zeros(8, dtype=torch.float64, device=DEV)
    a[1:] = cand
    env.step(a)
    pred = _snap(env)
    assert len({float(r) for r in pred["reward"][1:]}) > 1, "the candidates do not differ"
    j = 1 + int(torch.argmax(pred["reward"][1:]).item())
    env.restore_state(s, [0])
    a2 = a.clone()
    a2[0] = a[j]
    env.step(a2)
    real = _snap(env)
    for k in ("obs", "reward", "terminated", "truncated", "info", "bodies", "poly_verts", "poly_counts"):
        assert torch.equal(real[k][0], pred[k][j]), k
    env.close()


# ---- 5: another handle, and a file --------------------------------------------------------------------------------------------------------------
def test_another_handle_and_a_file(monkeypatch, tmp_path):
    from benchpush_amd._lib import BpError
    from benchpush_amd.state import EnvState
    _fresh(monkeypatch, {})
    A, B = _ship(8), _ship(4)
    assert A.state_layout_id() == B.state_layout_id() and A.state_bytes() == B.state_bytes()
    acts = _actions(6, 8, seed=15)
    A.reset(); B.reset()
    for t in range(3):
        A.step(acts[t])
    path = str(tmp_path / "two_envs.pt")
    A.save_state([5, 2]).cpu().save(path)
    state = EnvState.load(path).to(DEV)
    assert state.env_ids.tolist() == [5, 2]
    B.restore_state(state, [0, 3])
    _equal(_snap(A), _snap(B), "after the load", rows=[5, 2], other_rows=[0, 3])
    for t in range(3, 6):
        A.step(acts[t])
        b = torch.zeros(4, dtype=torch.float64, device=DEV)
        b[0], b[3] = acts[t, 5], acts[t, 2]
        B.step(b)
        _equal(_snap(A), _snap(B), ("step", t), rows=[5, 2], other_rows=[0, 3])
    # a handle with another body capacity, and one with other trials, refuse the records and stay as they were
    C = _ship(2, conc=0.2)
    D = _ship(2, trials=_trials(0.3, 3, 9))
    assert C.nb_cap != A.nb_cap and C.state_layout_id() != A.state_layout_id() and D.state_layout_id() != A.state_layout_id()
    for other in (C, D):
        other.reset()
        before = _snap(other)
        with pytest.raises(BpError, match="BP_EINVAL"):
            other.restore_state(state, [0, 1])
        _equal(_snap(other), before, "refusing handle")
        other.close()
    A.close(); B.close()


# ---- 6: envs not named are untouched; bad arguments are refused -----------------------------------------------------------------------------------
def test_unnamed_envs_untouched_and_bad_arguments_refused(monkeypatch):
    from benchpush_amd._lib import BpError
    _fresh(monkeypatch, {})
    env = _ship()
    with pytest.raises(BpError, match="BP_ESTATE"):
        env.save_state()                                             # before the first reset
    with pytest.raises(BpError, match="BP_ESTATE"):
        env.clone_envs([0], [1])
    acts = _actions(5, 8, seed=16)
    env.reset()
    for t in range(2):
        env.step(acts[t])
    s = env.save_state()
    for t in range(2, 5):
        env.step(acts[t])
    before = _snap(env)
    one = env.save_state([2])
    env.restore_state(type(s)(s.records[2:3], s.obs[2:3], s.reward[2:3], s.terminated[2:3], s.truncated[2:3], s.info[2:3], s.layout_id, s.env_ids[2:3]))
    now = _snap(env)
    others = [0, 1, 3, 4, 5, 6, 7]
    _equal(now, before, "envs that were not named", rows=others)
    assert not torch.equal(now["bodies"][2], before["bodies"][2]) and not torch.equal(now["obs"][2], before["obs"][2])
    env.restore_state(one)                                           # forward again: env 2 is back where the batch is
    _equal(_snap(env), before, "after the second restore")
    E = env.num_envs
    bad_calls = [lambda: env.save_state([-1]), lambda: env.save_state([E]), lambda: env.save_state([0, E]),
                 lambda: env.restore_state(one, [-1]), lambda: env.restore_state(one, [E]),
                 lambda: env.restore_state(env.save_state([0, 1]), [3, 3]),                       # a destination twice
                 lambda: env.clone_envs([0], [E]), lambda: env.clone_envs([-1], [1]),
                 lambda: env.clone_envs([0, 1], [2, 2]),                                          # a destination twice
                 lambda: env.clone_envs([0, 1], [1, 2])]                                          # a destination that is also a source
    zeroed, short = one.clone(), one.clone()
    zeroed.records.zero_()
    short.records = short.records[:, : short.records.shape[1] - 16].contiguous()
    flipped = one.clone()
    flipped.records[0, 16] ^= 1                                      # the layout id of the header
    bad_calls += [lambda: env.restore_state(zeroed), lambda: env.restore_state(short), lambda: env.restore_state(flipped)]
    for i, call in enumerate(bad_calls):
        with pytest.raises(BpError, match="BP_EINVAL"):
            call()
        _equal(_snap(env), before, ("refused call", i))
    env.close()


# ---- 7: maze ------------------------------------------------------------------------------------------------------------------------------------
def test_maze_rewind_and_fan_out(monkeypatch):
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    _fresh(monkeypatch, {})
    env = BatchedMazeEnv(8, cfg={"num_obstacles": 20}, num_layouts=4, base_seed=2, device=DEV)
    _, at_save, first, _ = _rewind(env, 3, 4, seed=17)
    # the distance-increment reward of the first replayed step depends on e_prevdist, the sticky wall flag on e_flags: both compared above through info;
    # the increment is a live quantity in this window
    assert any(float(r["info"][:, 7].abs().sum()) > 0 for r in first)
    before = _snap(env)
    assert not torch.equal(before["bodies"][0], before["bodies"][1])
    env.clone_envs([0, 0, 0], [1, 2, 3])
    acts = _actions(3, 8, seed=18)
    acts[:, 1:4] = acts[:, 0:1]
    for t in range(3):
        env.step(acts[t])
        a = _snap(env)
        for d in (1, 2, 3):
            _equal(a, a, ("maze clone %d" % d, t), rows=0, other_rows=d)
        assert torch.equal(a["info"][1:4, 7], a["info"][0:1, 7].expand(3)) and torch.equal(a["info"][1:4, 10], a["info"][0:1, 10].expand(3))
    env.check_errors()
    env.close()


# ---- 8: box-delivery and area-clearing ----------------------------------------------------------------------------------------------------------
def _box_env(task):
    if task == "box_delivery":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(4, num_trials=4, device=DEV)
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    return BatchedAreaClearingEnv(4, num_trials=4, device=DEV)


@pytest.mark.parametrize("task", ["box_delivery", "area_clearing"])
def test_box_tasks_rewind_observe_and_fan_out(monkeypatch, task):
    _fresh(monkeypatch, {})
    env = _box_env(task)
    s, at_save, first, _ = _rewind(env, 3, 3, seed=19, reset_env=1, box=True)
    nb = 6 + env.nbox                                                # robot parts, then the boxes
    assert not torch.equal(first[-1]["bodies"][:, 6:nb, :3], at_save["bodies"][:, 6:nb, :3]), "no box moved inside the window"
    # the observation comes back from the restored state alone (channel 2 reads the robot's distance map, which is part of the record)
    env.restore_state(s)
    env.obs.zero_()
    env.observe()
    assert torch.equal(env.obs, s.obs)
    # fan-out 0 -> 1
    assert not torch.equal(at_save["bodies"][0], at_save["bodies"][1])
    env.clone_envs([0], [1])
    acts = _actions(3, 4, seed=20)
    acts[:, 1] = acts[:, 0]
    for t in range(3):
        env.step(acts[t])
        a = _snap(env, box=True)
        _equal(a, a, (task, "clone", t), rows=0, other_rows=1)
    env.check_errors()
    env.close()


# ---- 9: wrappers --------------------------------------------------------------------------------------------------------------------------------
def test_vec_env_save_and_restore(monkeypatch):
    from benchpush_amd.envs.vec_env import make_ship_ice_vec_env
    _fresh(monkeypatch, {})
    venv = make_ship_ice_vec_env(4, cfg={"concentration": 0.3}, to_numpy=False, trials=_trials(), device=DEV)
    venv.max_episode_steps = 4                                       # a TimeLimit inside the window: the counters matter
    acts = _actions(5, 4, seed=21)
    venv.reset()
    for t in range(2):
        venv.step(acts[t])
    s = venv.save_state()
    steps_at_save = venv._steps.clone()
    assert steps_at_save.tolist() == [2, 2, 2, 2]

    def window():
        out = []
        for t in range(2, 5):
            obs, rew, done, infos = venv.step(acts[t])
            rec = {"obs": obs.clone(), "rew": rew.clone(), "done": done.clone(), "steps": venv._steps.clone()}
            ended = infos.done_indices().tolist()
            if ended:   # the last observation of the episodes that ended in this step, as a learner receives it
                rec["terminal_observation"] = torch.stack([infos[i]["terminal_observation"].clone() for i in ended])
                rec["time_limit"] = torch.tensor([infos[i]["TimeLimit.truncated"] for i in ended])
            out.append(rec)
        return out
    first = window()
    assert any(bool(r["done"].any()) for r in first), "no TimeLimit truncation inside the window"
    venv.restore_state(s)
    assert torch.equal(venv._steps, steps_at_save)
    _equal(first, window(), "vec env window")
    venv.close()


def _deep_equal(a, b, what):
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), what
        for k in a:
            _deep_equal(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _deep_equal(x, y, (what, i))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, np.asarray(b)), what
    else:
        assert a == b, what


def _adapter(name):
    if name == "ship_ice":
        from benchpush_amd.envs.ship_ice import ShipIceEnv
        return ShipIceEnv(cfg={"concentration": 0.3}, trials=_trials(), device=DEV), 1
    if name == "maze":
        from benchpush_amd.envs.maze_namo import MazeNAMO
        return MazeNAMO(cfg={"num_obstacles": 20}, num_layouts=2, base_seed=2, device=DEV), 1
    if name == "box_delivery":
        from benchpush_amd.envs.box_delivery import BoxDeliveryEnv
        return BoxDeliveryEnv(num_trials=2, device=DEV), 1
    from benchpush_amd.envs.area_clearing import AreaClearingEnv
    return AreaClearingEnv(num_trials=2, device=DEV), 1


@pytest.mark.parametrize("name", ["ship_ice", "maze", "box_delivery", "area_clearing"])
def test_single_env_adapters_save_and_restore(monkeypatch, name):
    _fresh(monkeypatch, {})
    env, dim = _adapter(name)
    acts = _actions(4, 1, seed=22).cpu().numpy()
    env.reset()
    for t in range(2):
        env.step(acts[t])
    s = env.save_state()
    t_at_save = env.t

    def window():
        return [env.step(acts[t]) for t in range(2, 4)]
    first = window()
    assert env.t == t_at_save + 2
    env.restore_state(s)
    assert env.t == t_at_save
    second = window()
    for t, (x, y) in enumerate(zip(first, second)):
        assert np.array_equal(x[0], y[0]), (name, "observation", t)
        assert x[1] == y[1] and x[2] == y[2] and x[3] == y[3], (name, "reward / flags", t)
        _deep_equal(x[4], y[4], (name, "info", t))
    if hasattr(env, "total_work"):
        assert len(env.total_work[1]) == 4                           # two steps before the save, two replayed: the list was rewound, not appended to twice
    env.close()
