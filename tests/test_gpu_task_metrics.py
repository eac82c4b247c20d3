"""On-device task-driven episode metrics of box-delivery / area-clearing (k_task_metrics) against the package's host TaskDrivenMetric, fed per env from the
batched outputs (info row, world_polys() at reset, completed flags): every comparison is == (NaN == NaN).  4 envs, hand-built trials whose course the CPU
oracles show (box-delivery, every action 1.0: trial TB delivers two of three boxes in two steps and is truncated by inactivity at step 8, TC delivers none
and is truncated at step 6, TA delivers all three in two steps; area-clearing, clear_env, velocity (1, 0): the box that straddles the boundary side next to
the robot is cleared in the first step)."""
import functools
import types
import warnings

import numpy as np
import pytest
import torch

from benchpush_amd import _lib
from benchpush_amd import area_clearing_scenario as A
from benchpush_amd import box_delivery_scenario as S
from benchpush_amd.config import default_cfg
from benchpush_amd.metrics.task_driven_metric import TaskDrivenMetric, _area_centroid

pytestmark = pytest.mark.gpu
E = 4


def eq(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


class Driver:
    """One batched env plus one host TaskDrivenMetric per env.  `rows[e]` are the host's rows of env e's finished episodes, `bad` every disagreement seen."""

    def __init__(self, env, task):
        self.env, self.task = env, task
        self.tw_col = 3 if task == 1 else 6
        self.goals = [tuple(g) for g in env.goal_points] if task == 1 else [(env.bd_params["recept_x"], env.bd_params["recept_y"])]
        self.m = [TaskDrivenMetric("t", robot_mass=env.cfg.agent.mass) for _ in range(E)]
        self.rows = [[] for _ in range(E)]
        self.boxes = [None] * E
        self.steps, self.work, self.open = [0] * E, [0.0] * E, [False] * E
        self.closed_by_reset, self.bad = 0, []

    def _emit(self, e):
        m = self.m[e]
        self.rows[e].append([float(m.efficiency_scores[-1]), float(m.effort_scores[-1]), float(m.rewards[-1]), float(m.success_rates[-1]),
                             float(self.steps[e]), float(self.work[e])])

    def reset(self, mask=None):
        ids = range(E) if mask is None else np.nonzero(mask)[0]
        for e in ids:
            if self.open[e] and self.steps[e] > 0:      # the reset closes a running episode as truncated: the eps_complete branch of update()
                m = self.m[e]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    m.rewards.append(m.eps_reward)
                    rate, eff = m.compute_efficiency_score(m.compute_mst_cost_for_successful_boxes())
                    m.success_rates.append(rate); m.efficiency_scores.append(eff); m.effort_scores.append(m.compute_effort_score())
                self._emit(e)
                self.closed_by_reset += 1
        self.env.reset(None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)))
        torch.cuda.synchronize()
        info = self.env.info.cpu().numpy()
        verts, cnt = self.env.world_polys()
        verts, cnt = verts.cpu().numpy(), cnt.cpu().numpy()
        for e in ids:
            polys = [verts[e, 6 + k, : cnt[e, 6 + k]].copy() for k in range(self.env.nbox)]
            self.m[e].reset({"state": tuple(round(float(v), 2) for v in info[e, :3]), "obs": polys, "goal_positions": self.goals})
            self.boxes[e] = np.array([[a, c[0], c[1]] for a, c in map(_area_centroid, polys)])
            self.steps[e], self.work[e], self.open[e] = 0, 0.0, True

    def account(self, ids=None):
        """After a step: feeds the host metric of every env in `ids` (None: all) that has an episode running; returns the done flags."""
        torch.cuda.synchronize()
        env = self.env
        info, rew = env.info.cpu().numpy(), env.reward.cpu().numpy()
        done = (env.terminated.cpu().numpy() != 0) | (env.truncated.cpu().numpy() != 0)
        comp = env.box_completed()
        for e in (range(E) if ids is None else ids):
            if not self.open[e]:
                continue
            self.steps[e] += 1
            self.work[e] = float(info[e, self.tw_col])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self.m[e].update({"state": tuple(round(float(v), 2) for v in info[e, :3]), "total_work": float(info[e, self.tw_col]),
                                  "box_completed_statuses": [bool(c) for c in comp[e, : env.nbox]]}, float(rew[e]), eps_complete=bool(done[e]))
            if done[e]:
                self._emit(e)
                self.open[e] = False
        return done

    def check(self, tag):
        rows, cnt = self.env.episode_metrics()
        rows, cnt = rows.cpu().numpy(), cnt.cpu().numpy()
        for e in range(E):
            if cnt[e] != len(self.rows[e]) or (self.rows[e] and not eq(rows[e], self.rows[e][-1])):
                self.bad.append((tag, e, int(cnt[e]), rows[e].tolist(), self.rows[e][-1:]))


def bd_trials():
    cfg = default_cfg("box_delivery")
    cfg.misc.inactivity_cutoff = 6
    base = S.generate_trials(cfg, 1)[0]

    def mk(boxes):
        tr = dict(base)
        tr["start"], tr["boxes"] = np.array([1.5, 1.75, 0.0]), np.array(boxes)
        return tr
    tb = mk([[2.6, 1.75, 0.3], [3.2, 1.75, 0.0], [-3.0, -1.0, 0.0]])
    tc = mk([[-3.0, -1.0, 0.0], [-3.0, 0.0, 0.0], [-3.0, 1.0, 0.0]])
    ta = mk([[2.6, 1.75, 0.3], [3.2, 1.75, 0.0], [3.9, 1.75, 0.0]])
    return [tb, tc, ta]


def bd_env(trials=None):
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    return BatchedBoxDeliveryEnv(E, cfg={"misc": {"inactivity_cutoff": 6}}, trials=trials or bd_trials())


ONES = torch.ones(E, dtype=torch.float64)
RESET_AT = 1      # after this many steps env 1 (in trial TC, nothing delivered, episode running) is reset; its next env step, a drive of 1.2 m, takes many slices


@functools.lru_cache(maxsize=None)
def bd_session():
    """The lock-step run every box-delivery test refers to: 4 envs x 3 or more episodes each, env 1 reset in the middle of its first episode."""
    env = bd_env()
    d = Driver(env, 0)
    d.reset()
    d.first_boxes = (env.episode_boxes().cpu().numpy(), [b.copy() for b in d.boxes])
    d.check("reset")
    for t in range(40):
        env.step(ONES)
        done = d.account()
        d.check("step %d" % t)
        mask = done.copy()
        if t + 1 == RESET_AT:
            mask[1] = True
        if mask.any():
            d.reset(mask)
            d.check("reset after step %d" % t)
        if min(len(r) for r in d.rows) >= 3:
            break
    d.history = [t.cpu().numpy() for t in env.episode_history()]
    d.lists = env.episode_lists()
    d.last_boxes = (env.episode_boxes().cpu().numpy(), [b.copy() for b in d.boxes])
    env.check_errors()
    env.close()
    return d


def test_box_delivery_rows_equal_the_host_metric_after_every_step():
    d = bd_session()
    for e in range(E):
        print("env", e, "rows", d.rows[e])
    assert not d.bad, d.bad[:3]
    rows = [r for e in range(E) for r in d.rows[e]]
    assert any(r[3] * 3 >= 2 for r in rows) and any(r[3] == 0.0 for r in rows) and d.closed_by_reset >= 1     # two or more delivered; none; closed by reset()
    assert d.rows[1][0][4] == RESET_AT and d.rows[1][0][3] == 0.0
    assert all(len(d.rows[e]) >= 3 for e in range(E))


def check_history(d):
    ring, sums, cnt = d.history
    for e in range(E):
        host = np.array(d.rows[e])
        n = len(host)
        assert cnt[e] == n and n >= 3
        for k in range(max(0, n - _lib.EPM_RING), n):
            assert eq(ring[e, k % _lib.EPM_RING], host[k]), (e, k)
        s = np.zeros(6)
        for r in host:
            s = s + r
        assert eq(sums[e], s), (e, sums[e], s)
        assert eq(d.lists[e], host[max(0, n - _lib.EPM_RING):]), e
    for dev, host in (d.first_boxes, d.last_boxes):
        for e in range(E):
            nb = len(host[e])
            assert eq(dev[e, :nb], host[e]) and not dev[e, nb:].any(), e


def test_history_ring_sums_lists_and_reset_boxes_equal_the_host_lists():
    check_history(bd_session())


def ac_cfg():
    cfg = default_cfg("area_clearing")
    cfg.env = "clear_env"
    cfg.agent.action_type = "velocity"
    cfg.sim.t_max = 4
    return cfg


@functools.lru_cache(maxsize=None)
def ac_session():
    from benchpush_amd.envs.area_clearing import AreaClearingEnv, BatchedAreaClearingEnv
    cfg = ac_cfg()
    gen = A.generate_trials(cfg, 3)
    tr = dict(gen[0])
    tr["start"] = np.array([4.6, 0.0, 0.0])                  # facing the boundary side x = 5, the nearest one
    tr["boxes"] = np.array(gen[0]["boxes"])
    tr["boxes"][0] = [5.45, 0.0, 0.0]                        # straddles that side
    env = BatchedAreaClearingEnv(E, cfg={"env": "clear_env", "agent": {"action_type": "velocity"}, "sim": {"t_max": 4}}, trials=[tr, gen[1], gen[2]])
    adapter = types.SimpleNamespace(boundary_vertices=A.env_layout(cfg).boundary)
    d = Driver(env, 1)
    d.status_bad = []
    d.reset()
    d.first_boxes = (env.episode_boxes().cpu().numpy(), [b.copy() for b in d.boxes])
    d.check("reset")
    act = torch.tensor([[1.0, 0.0]] * E, dtype=torch.float64)
    for t in range(30):
        env.step(act)
        done = d.account()
        verts, cnt = env.world_polys()
        verts, cnt, comp = verts.cpu().numpy(), cnt.cpu().numpy(), env.box_completed()
        for e in range(E):                                   # Q.cleared against the adapter's _statuses of the same polygons
            want = AreaClearingEnv._statuses(adapter, [verts[e, 6 + k, : cnt[e, 6 + k]] for k in range(env.nbox)])
            if [bool(c) for c in comp[e, : env.nbox]] != want:
                d.status_bad.append((t, e))
        d.check("step %d" % t)
        if done.any():
            d.reset(done)
            d.check("reset after step %d" % t)
        if min(len(r) for r in d.rows) >= 3:
            break
    d.history = [t.cpu().numpy() for t in env.episode_history()]
    d.lists = env.episode_lists()
    d.last_boxes = (env.episode_boxes().cpu().numpy(), [b.copy() for b in d.boxes])
    env.check_errors()
    env.close()
    return d


def test_area_clearing_rows_flags_and_history_equal_the_host_metric():
    d = ac_session()
    for e in range(E):
        print("env", e, "rows", d.rows[e])
    assert not d.bad, d.bad[:3]
    assert not d.status_bad, d.status_bad[:5]
    assert any(r[3] > 0.0 for e in range(E) for r in d.rows[e])          # an episode that ended with a cleared box
    assert d.rows[0][0][3] == 0.1 and d.rows[0][0][0] > 0.0              # the hand-placed one: 1 of 10 boxes, a spanning tree to show for it
    check_history(d)


def finish(env, d=None, steps=12):
    """Steps all envs with action 1.0 until every env has finished an episode; returns (rows, counts)."""
    for _ in range(steps):
        env.step(ONES)
        torch.cuda.synchronize()
        if bool(((env.terminated != 0) | (env.truncated != 0)).all()):
            break
    rows, cnt = env.episode_metrics()
    return rows.cpu().numpy(), cnt.cpu().numpy()


def test_clones_and_restored_states_carry_the_episode():
    want = bd_session().rows[0][0]                # env 0's first episode: trial TB under action 1.0, uninterrupted
    env = bd_env()
    env.reset()
    env.step(ONES)                                # mid-episode: env 0 has delivered one box
    env.clone_envs([0, 0, 0], [1, 2, 3])
    rows, cnt = finish(env)
    assert all(eq(rows[e], want) for e in range(E)) and cnt.tolist() == [1] * E, (rows, cnt, want)
    # save -> other steps -> restore -> the original actions
    env.reset()                                   # every env starts its second episode: env 2 plays TB ((2 + 1) % 3 = 0)
    env.step(ONES)
    env.step(ONES)
    state = env.save_state()
    for _ in range(3):
        env.step(-0.5 * ONES)
    env.restore_state(state)
    rows, cnt = finish(env)
    assert eq(rows[2], want) and cnt[2] == 2, (rows[2], cnt, want)
    env.close()


def test_async_steps_give_the_rows_of_the_lock_step_run():
    d = bd_session()
    env = bd_env()
    env.reset()
    seen = [[] for _ in range(E)]                 # rows in the order the count went up
    steps_done = np.zeros(E, int)                 # env steps of the running episode
    cancelled = False
    rows0, cnt0 = [t.cpu().numpy() for t in env.episode_metrics()]
    for call in range(4000):
        _, _, term, trunc, _, ready = env.step_async(ONES, budget=50)
        torch.cuda.synchronize()
        rdy = ready.cpu().numpy() != 0
        rows, cnt = [t.cpu().numpy() for t in env.episode_metrics()]
        assert eq(rows[~rdy], rows0[~rdy]) and np.array_equal(cnt[~rdy], cnt0[~rdy]), call      # a busy env's row and count stay
        done = rdy & ((term.cpu().numpy() != 0) | (trunc.cpu().numpy() != 0))
        steps_done[rdy] += 1
        for e in np.nonzero(cnt > cnt0)[0]:
            assert done[e] and cnt[e] == cnt0[e] + 1
            seen[e].append(rows[e].copy())
        mask = done.copy()
        if not cancelled and steps_done[1] == RESET_AT and not rdy[1]:
            mask[1] = cancelled = True            # env 1 is busy with its next env step: the reset cancels that step and closes the episode
        if mask.any():
            env.reset(torch.from_numpy(mask.astype(np.uint8)))
            torch.cuda.synchronize()
            steps_done[mask] = 0
            rows, cnt = [t.cpu().numpy() for t in env.episode_metrics()]
            if mask[1] and not done[1]:
                assert cnt[1] == cnt0[1] + 1 and rows[1][4] == RESET_AT       # one truncated row
                seen[1].append(rows[1].copy())
        rows0, cnt0 = rows, cnt
        if min(len(s) for s in seen) >= 3:
            break
    env.drain()
    env.check_errors()
    env.close()
    assert cancelled
    for e in range(E):
        assert len(seen[e]) >= 3 and eq(np.array(seen[e][:3]), np.array(d.rows[e][:3])), (e, seen[e][:3], d.rows[e][:3])


def test_other_handles_are_refused():
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    env = BatchedShipIceEnv(2, cfg={"concentration": 0.3}, trials=default_trials(0.3, 2, base_seed=7))
    env.reset()
    out = torch.zeros((2, 24, 3), dtype=torch.float64, device=env.device)
    assert env.L.bp_bd_get_episode_boxes(env.h, out.data_ptr(), None) == -1          # BP_EINVAL
    host = np.zeros((2, 24), np.uint8)
    assert env.L.bp_bd_get_completed(env.h, host.ctypes.data) == -1
    rows, cnt = env.episode_metrics()                                                 # the ship-ice path is as it was
    assert rows.shape == (2, 6) and int(cnt.sum()) == 0
    env.close()


def test_planning_baseline_scores_its_envs_side_by_side():
    from benchpush_amd.baselines.area_clearing.planning_based.policy import PlanningBasedPolicy
    cfg = default_cfg("area_clearing")
    cfg.env = "clear_env"
    trial = A.generate_trials(cfg, 1)
    pol = PlanningBasedPolicy(cfg={"env": "clear_env"}, num_envs=E, t_max=3, trials=trial)
    env = pol._ensure_env()
    emitted, step = [], env.step

    def recording_step(actions):
        out = step(actions)
        emitted.append((out[1].cpu().numpy().copy(), ((out[2] != 0) | (out[3] != 0)).cpu().numpy()))
        return out
    env.step = recording_step
    success, eff, effort, rewards, name = pol.evaluate(E)
    pol.close()
    assert name == "GTSP" and all(len(v) >= E for v in (success, eff, effort, rewards))
    assert all(0.0 <= s <= 1.0 for s in success)
    run, want = [0.0] * E, []
    for rew, done in emitted:                      # the sums of the rewards the envs emitted, in the order the episodes finished
        for e in range(E):
            run[e] = run[e] + float(rew[e])
            if done[e]:
                want.append(run[e])
                run[e] = 0.0
    assert rewards == want, (rewards, want)
    # the single-env path -- the host metric on the reference-shaped env, as before -- sees the same trial and must give what each of the four envs gave
    one = PlanningBasedPolicy(cfg={"env": "clear_env"}, num_envs=1, t_max=3, trials=trial)
    s1, e1, f1, r1, _ = one.evaluate(1)
    one.close()
    assert len(s1) == 1
    for k in range(E):
        assert eq([success[k], eff[k], effort[k], rewards[k]], [s1[0], e1[0], f1[0], r1[0]]), (k, success[k], eff[k], effort[k], rewards[k], s1, e1, f1, r1)
