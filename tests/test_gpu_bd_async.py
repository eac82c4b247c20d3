"""box-delivery-v0, asynchronous step (step_async / drain): every transition an env emits against the oracle, bit for bit, whatever the budget and the cut."""
import math

import numpy as np
import pytest
import torch

from benchpush_amd import box_delivery_scenario as S
from benchpush_amd.config import default_cfg

from test_gpu_bd import _oracle

pytestmark = pytest.mark.gpu

SUB = 10   # info column "substeps" (both tasks): sim steps of the env step


class SharedOracle:
    """One oracle per (key, env) for the whole module: an env's transition sequence depends on its own trials and actions only, so the runs that use the same
    action streams (budgets, cuts) replay the recorded steps and resets instead of computing them again; a run that goes further steps the oracle on.  A run
    whose operations differ from the recorded ones fails."""
    _cache = {}

    def __init__(self, key, make):
        if key not in self._cache:
            self._cache[key] = (make(), [])
        self.o, self.ops = self._cache[key]
        self.i = 0
        self.last = None

    def _do(self, op, arg, fn):
        arg = np.asarray(arg, np.float64)
        if self.i < len(self.ops):
            rop, rarg, res = self.ops[self.i]
            assert rop == op and np.array_equal(rarg, arg, equal_nan=True), ("this run's oracle operations differ from the recorded ones", self.i, rop, op)
        else:
            out = fn()
            res = (out, self.o.shape_states().copy(), self.o.alive().copy())
            self.ops.append((op, arg.copy(), res))
        self.i += 1
        self.last = res
        return res[0]

    def step(self, a):
        return self._do("step", a, lambda: self.o.step(a))

    def reset(self, trial):
        return self._do("reset", trial["start"], lambda: self.o.reset(trial))

    def observe(self):
        return self._do("observe", 0.0, lambda: self.o.observe())

    def shape_states(self):
        return self.last[1]

    def alive(self):
        return self.last[2]


class AsyncRun:
    """Drives one handle through step_async / drain / step with a per-env seeded action stream (an action is consumed only when its env is idle) and, if
    `make_oracle` is given, one oracle per env that is stepped with the accepted action whenever the env emits a transition.  Every emitted transition is
    compared with == (observation, reward, flags, info, bodies, alive flags), the rows of the envs that emitted nothing with their contents before the call,
    every reset observation with the oracle's.  `log[e]` is the env's transition sequence."""

    def __init__(self, env, trials, make_oracle, info_keys, seed, first=None, act_shape=(), compare_alive=True):
        self.env, self.trials, self.make_oracle, self.keys = env, trials, make_oracle, info_keys
        E = self.E = env.num_envs
        self.rng = [np.random.RandomState(seed + e) for e in range(E)]
        self.first = {e: list(a) for e, a in (first or {}).items()}
        self.act_shape = act_shape
        self.compare_alive = compare_alive
        self.episode = np.zeros(E, int)
        self.idle = np.ones(E, bool)
        self.accepted = [None] * E
        self.log = [[] for _ in range(E)]
        self.calls = 0
        self.seen = dict(mixed=0, max_slices=0, delivered=0, max_substeps=0.0, resets=0, cancelled=0)
        self.oracles = [make_oracle(e, trials[e % len(trials)]) for e in range(E)] if make_oracle else None
        obs, _ = env.reset()
        torch.cuda.synchronize()
        if self.oracles:
            assert np.array_equal(obs.cpu().numpy(), np.stack([o.observe() for o in self.oracles]))

    def _outputs(self):
        v = self.env
        return [t.clone() for t in (v.obs, v.reward, v.terminated, v.truncated, v.info, v.slices)]

    def _next_action(self, e):
        if self.first.get(e):
            return np.float64(self.first[e].pop(0)) if self.act_shape == () else np.asarray(self.first[e].pop(0), np.float64)
        return self.rng[e].uniform(-1, 1, self.act_shape)

    def _actions(self):
        """Rows of idle envs: the next action of the env's stream (it is accepted by this call); rows of busy envs: NaN -- they must be ignored."""
        a = np.full((self.E,) + self.act_shape, np.nan)
        for e in range(self.E):
            if self.idle[e]:
                self.accepted[e] = self._next_action(e)
                a[e] = self.accepted[e]
        return a

    def _check(self, before, ready, tag, slices_rule=None):
        env = self.env
        after = self._outputs()
        for b, a in zip(before, after):
            assert torch.equal(b[~ready], a[~ready]), (tag, "rows of envs that emitted nothing changed")
        rdy = ready.cpu().numpy()
        if 0 < rdy.sum() < self.E:
            self.seen["mixed"] += 1
        if not rdy.any():
            return rdy
        obs, rew, term, trunc, info, slices = [t.cpu().numpy() for t in after]
        st = env.body_state().cpu().numpy()
        alive = env.box_state()[0]
        n = 6 + env.nbox
        for e in np.nonzero(rdy)[0]:
            self.log[e].append((obs[e].copy(), rew[e], term[e], trunc[e], info[e].copy(), st[e, :n].copy(), alive[e].copy()))
            self.seen["max_slices"] = max(self.seen["max_slices"], int(slices[e]))
            self.seen["max_substeps"] = max(self.seen["max_substeps"], info[e, SUB])
            assert slices[e] >= 1
            if self.oracles:
                o = self.oracles[e]
                oo, orr, ot, otr, oi = o.step(self.accepted[e])
                oiv = np.array([oi[k] for k in self.keys])
                assert np.array_equal(info[e], oiv), (tag, e, np.argwhere(info[e] != oiv)[:5])
                assert rew[e] == orr and bool(term[e]) == ot and bool(trunc[e]) == otr, (tag, e)
                assert np.array_equal(obs[e], oo), (tag, e)
                sel = np.ones(n, bool)
                if self.compare_alive:
                    sel[6:] = o.alive().astype(bool)
                    assert np.array_equal(alive[e, : env.nbox].astype(bool), o.alive().astype(bool)), (tag, e)
                    self.seen["delivered"] = max(self.seen["delivered"], int(oi.get("cumulative_boxes", 0)))
                assert np.array_equal(st[e, :n][sel], o.shape_states()[:n][sel]), (tag, e)
                if slices_rule is not None:
                    assert slices[e] == slices_rule(oi["substeps"]), (tag, e, slices[e], oi["substeps"])
            self.idle[e] = True
        return rdy

    def _reset_done(self, rdy, tag):
        done = rdy.astype(bool) & (self.env.terminated.cpu().numpy().astype(bool) | self.env.truncated.cpu().numpy().astype(bool))
        if done.any():
            self.reset(done, tag)

    def reset(self, mask, tag):
        """reset(mask): the envs of the mask start their next trials; a busy one is cancelled (its accepted action is dropped with the half-done env step)."""
        obs, _ = self.env.reset(torch.from_numpy(mask.astype(np.uint8)))
        torch.cuda.synchronize()
        for e in np.nonzero(mask)[0]:
            self.episode[e] += 1
            self.seen["resets"] += 1
            self.seen["cancelled"] += int(not self.idle[e])
            self.idle[e] = True
            if self.oracles:
                oo = self.oracles[e].reset(self.trials[(e + self.episode[e]) % len(self.trials)])
                assert np.array_equal(obs[e].cpu().numpy(), oo), (tag, "reset obs", e)

    def step_async(self, budget, slices_rule=None):
        before = self._outputs()
        a = self._actions()
        self.idle[:] = False
        ready = self.env.step_async(torch.from_numpy(a), budget)[5]
        torch.cuda.synchronize()
        self.calls += 1
        assert self.env.async_open
        rdy = self._check(before, ready.bool(), ("step_async", self.calls), slices_rule)
        self._reset_done(rdy, ("step_async", self.calls))
        return rdy

    def drain(self):
        before = self._outputs()
        was_busy = ~self.idle
        ready = self.env.drain()[5]
        torch.cuda.synchronize()
        assert not self.env.async_open
        rdy = self._check(before, ready.bool(), ("drain", self.calls))
        assert np.array_equal(rdy.astype(bool), was_busy), "drain() finishes the busy envs and only those"
        self._reset_done(rdy, ("drain", self.calls))
        return rdy

    def step(self):
        """The lock-step step() with the same per-env action streams."""
        before = self._outputs()
        a = self._actions()
        self.env.step(torch.from_numpy(a))
        torch.cuda.synchronize()
        self.env.slices.fill_(1)
        rdy = self._check(before, torch.ones(self.E, dtype=torch.bool, device=self.env.device), ("step", self.calls))
        self._reset_done(rdy, ("step", self.calls))

    def run_async(self, budget, transitions, step_limit, slices_rule=None, drain_after=None):
        # an env step is at most step_limit + 1 sim steps of execute_robot_path (its counter runs over all waypoints) and as many of
        # step_simulation_until_still, so every env emits at least once in ceil(2 (step_limit + 1) / budget) calls
        cap = transitions * math.ceil(2 * (step_limit + 1) / budget)
        while min(len(l) for l in self.log) < transitions:
            assert self.calls < cap, ("an env never became ready", [len(l) for l in self.log])
            self.step_async(budget, slices_rule)
            if drain_after is not None and self.calls == drain_after:
                self.drain()


def same_sequences(a, b, n):
    for e, (la, lb) in enumerate(zip(a.log, b.log)):
        assert len(la) >= n and len(lb) >= n
        for t in range(n):
            for x, y in zip(la[t], lb[t]):
                assert np.array_equal(x, y), ("env", e, "transition", t)


CUTOFF = 6   # misc.inactivity_cutoff lowered as in test_deep_episodes_...: truncations, hence resets, within 20 transitions


def _setup(E=4, step_limit=900, cutoff=CUTOFF):
    """4 envs, 3 trials, the hand-placed delivery of test_two_pass_step_matches_oracle (env 0 drives straight ahead four times), STEP_LIMIT 900."""
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    cfg = default_cfg("box_delivery")
    cfg.misc.inactivity_cutoff = cutoff
    gen = S.generate_trials(cfg, 3)
    tr = dict(gen[0])
    tr["start"] = np.array([1.5, 1.75, 0.0])
    tr["boxes"] = np.array(gen[0]["boxes"])
    tr["boxes"][0] = [2.6, 1.75, 0.3]
    trials = [tr, gen[1], gen[2]]
    env = BatchedBoxDeliveryEnv(E, cfg={"misc": {"inactivity_cutoff": cutoff}}, trials=trials, bd_overrides={"step_limit": step_limit})
    return env, cfg, trials


def _run(env, cfg, trials, with_oracle=True, step_limit=900, shared="bd"):
    """The action streams of every test of the 4-env setup: seeds 1000 + e, env 0 first drives straight ahead four times.  shared: the runs that start with a
    reset of all envs and never cancel an env step replay one oracle sequence per env (SharedOracle)."""
    from oracle.oracle_bd import BD_INFO_KEYS
    mk = None
    if with_oracle:
        real = lambda tr: _oracle(cfg, tr, step_limit=step_limit)
        mk = (lambda e, tr: SharedOracle((shared, e), lambda: real(tr))) if shared else (lambda e, tr: real(tr))
    return AsyncRun(env, trials, mk, BD_INFO_KEYS, seed=1000, first={0: [1.0, 1.0, 1.0, 1.0]})


def test_async_transitions_match_oracle_budgets_120_and_700():
    """Budgets 120 and 700, each until every env has emitted 20 transitions: each transition equals the oracle's step with the action the env accepted.  Each
    run holds calls with a mixed ready mask, a delivery, a forced STEP_LIMIT step and a reset; the test holds a transition that took three calls or more (with
    STEP_LIMIT 900 the env steps of these trials have at most ~903 sim steps -- a path cut at 901 and a short until-still loop --, which are two calls at 700
    and eight at 120)."""
    most = 0
    for budget in (120, 700):
        env, cfg, trials = _setup()
        r = _run(env, cfg, trials)
        r.run_async(budget, 20, 900)
        r.drain()
        env.check_errors()
        env.close()
        s = r.seen
        assert s["mixed"] >= 1 and s["delivered"] >= 1 and s["max_substeps"] >= 900 and s["resets"] >= 1 and s["max_slices"] >= 2, (budget, s)
        most = max(most, s["max_slices"])
    assert most >= 3


@pytest.mark.parametrize("budget", [120, 700])
def test_async_budget_is_honoured(monkeypatch, budget):
    """Without recurrence skips (BP_BD_CYCLE=0) total_sub advances by one per sim step, and the slice kernel leaves after a sim step iff the env step is not over
    and the sim steps of this call have reached the budget: an env step of n sim steps (the oracle's count, info['substeps']) takes max(1, ceil(n / b)) calls."""
    monkeypatch.setenv("BP_BD_CYCLE", "0")
    env, cfg, trials = _setup()
    r = _run(env, cfg, trials)
    r.run_async(budget, 8, 900, slices_rule=lambda n: max(1, math.ceil(n / budget)))
    r.drain()
    env.check_errors()
    assert env.cycle_skips() == (0, 0)
    env.close()
    assert r.seen["max_substeps"] >= 900 and r.seen["max_slices"] == math.ceil(r.seen["max_substeps"] / budget), r.seen


def test_async_is_independent_of_the_cut():
    """The same trials and per-env action streams through step() on one handle, through budget 120, and through budget 700 with a drain() in the middle: the
    three per-env transition sequences are identical."""
    N = 12
    runs = []
    for mode in ("step", 120, 700):
        env, cfg, trials = _setup()
        r = _run(env, cfg, trials, with_oracle=False)
        if mode == "step":
            for _ in range(N):
                r.step()
        else:
            r.run_async(mode, N, 900, drain_after=7 if mode == 700 else None)
            r.drain()
        env.check_errors()
        env.close()
        runs.append(r)
    same_sequences(runs[0], runs[1], N)
    same_sequences(runs[0], runs[2], N)
    assert runs[2].seen["mixed"] >= 1 and runs[1].seen["max_slices"] >= 3


WALL_LIMIT = 3000
# (start pose, heading action) found with the oracle: the robot stands in the lower left corner of the room, is turned towards a set point it cannot reach and put
# back by the boundary every sim step; it neither gets 0.05 m away from where it started nor within the waypoint's tolerances, so execute_robot_path runs all
# WALL_LIMIT + 1 sim steps (3003 with the until-still loop).  Its pose is the same double for every STEP_LIMIT >= 1800: a fixed point well before the limit.
WALL_CASES = [([-4.312474525992533, -2.0189483694970507, 3.872508972290043], -0.9280011272472595),
              ([-4.4114373790342185, -1.950187556244988, 5.610261808055878], 0.8786625607939911)]


def _wall_trials(cfg):
    base = S.generate_trials(cfg, 1)[0]
    trials = []
    for start, _ in WALL_CASES:
        tr = dict(base)
        tr["start"] = np.array(start)
        tr["boxes"] = np.array([[3.0, 1.5, 0.0], [2.0, 1.5, 0.3]])   # out of the robot's way: only the robot moves
        trials.append(tr)
    return trials


def test_async_recurrence_across_slices():
    """execute_robot_path against the walls of a corner until STEP_LIMIT (3000 here), cut by a budget of 400 sim steps: the resumed slices run on the kernel with
    the recurrence test, whole periods are skipped once the robot sits at its fixed point (cycle_skips() grows), and the transition is the oracle's."""
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    from oracle.oracle_bd import BD_INFO_KEYS
    cfg = default_cfg("box_delivery")
    trials = _wall_trials(cfg)
    env = BatchedBoxDeliveryEnv(2, trials=trials, bd_overrides={"step_limit": WALL_LIMIT})
    r = AsyncRun(env, trials, lambda e, t: _oracle(cfg, t, step_limit=WALL_LIMIT), BD_INFO_KEYS, seed=77, first={e: [a] for e, (_, a) in enumerate(WALL_CASES)})
    before = env.cycle_skips()
    r.run_async(400, 1, WALL_LIMIT)
    r.drain()
    env.check_errors()
    after = env.cycle_skips()
    env.close()
    assert r.seen["max_substeps"] > WALL_LIMIT and min(l[0][4][SUB] for l in r.log) > WALL_LIMIT, r.seen
    assert after[0] - before[0] >= 2 and after[1] - before[1] >= 1000, (before, after)
    assert 3 <= r.seen["max_slices"] < math.ceil(WALL_LIMIT / 400), r.seen   # cut several times, and fewer calls than the sim steps would take one by one


def test_async_guards():
    """While a slice is open step(), save_state, restore_state and clone_envs raise BpError and touch nothing; reset(mask) cancels a busy env; drain() emits
    nothing for idle envs and closes the handle, as does a reset of all envs; budget 0 and a damping config are refused."""
    from benchpush_amd._lib import BD_INFO_KEYS, BpError
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    env, cfg, trials = _setup()
    r = _run(env, cfg, trials, shared=None)
    saved = env.save_state()
    with pytest.raises(BpError):
        env.step_async(torch.zeros(4, dtype=torch.float64), 0)
    with pytest.raises(BpError):
        env.step_async(torch.zeros(3, dtype=torch.float64), 100)
    assert not env.async_open
    # one short slice: every env is busy afterwards (an env step is several hundred sim steps)
    rdy = r.step_async(40)
    assert not rdy.any() and env.async_open
    before = r._outputs() + [env.body_state().clone()]
    for call in (lambda: env.step(torch.zeros(4, dtype=torch.float64)), lambda: env.save_state(), lambda: env.restore_state(saved),
                 lambda: env.clone_envs([0], [1])):
        with pytest.raises(BpError):
            call()
    torch.cuda.synchronize()
    for b, a in zip(before, r._outputs() + [env.body_state().clone()]):
        assert torch.equal(b, a)
    # reset(mask) of the busy env 1: no transition for the cancelled step; first observation (checked in reset) and next transitions are a fresh oracle's
    r.reset(np.array([0, 1, 0, 0], bool), "cancel")
    assert r.seen["cancelled"] == 1 and env.async_open
    n1 = len(r.log[1])
    assert n1 == 0
    while min(len(l) for l in r.log) < 2:
        assert r.calls < 2 * math.ceil(2 * 901 / 300) + 4
        r.step_async(300)
    # drain: idle envs emit nothing, their cumulative columns stay; the busy ones finish (AsyncRun.drain checks the mask and the untouched rows)
    k = {n: i for i, n in enumerate(BD_INFO_KEYS)}
    cum = env.info[:, [k["cumulative_reward"], k["cumulative_distance"]]].clone()
    idle = torch.from_numpy(r.idle.copy()).to(env.device)
    r.drain()
    assert torch.equal(env.info[:, [k["cumulative_reward"], k["cumulative_distance"]]][idle], cum[idle])
    assert not env.async_open
    r.drain()   # nothing is busy: nothing happens
    # closed: the lock-step step() matches the oracle again
    r.step()
    r.step()
    env.save_state()
    # a reset of all envs closes the handle too
    r.step_async(40)
    assert env.async_open
    env.reset()
    assert not env.async_open
    env.step(torch.zeros(4, dtype=torch.float64))
    env.check_errors()
    env.close()
    damp = BatchedBoxDeliveryEnv(2, cfg={"sim": {"damping": 0.8}}, num_trials=2)
    damp.reset()
    with pytest.raises(BpError):   # refused by the library (bp_bd_step_async: BP_EINVAL), nothing launched, the handle stays closed
        damp.step_async(torch.zeros(2, dtype=torch.float64), 100)
    assert not damp.async_open
    damp.step(torch.zeros(2, dtype=torch.float64))
    damp.check_errors()
    damp.close()
