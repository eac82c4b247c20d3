"""area-clearing-v0, asynchronous step (step_async / drain): every transition an env emits against the oracle, bit for bit; cancel and drain."""
import math

import numpy as np
import pytest
import torch

from benchpush_amd import area_clearing_scenario as A
from benchpush_amd.config import default_cfg

from test_gpu_bd_async import AsyncRun, SharedOracle

pytestmark = pytest.mark.gpu

STEP_LIMIT = 600   # the path loop's limit, lowered from area_clearing_params' 5000 (bd_overrides, as the box-delivery tests do): most paths of this layout are longer,
#                    so most env steps are forced STEP_LIMIT steps of 601 + 100 sim steps (execute_robot_path to the limit, then cfg's fixed sim steps)
T_MAX = 7          # sim.t_max lowered through the cfg: time truncations, hence resets of ready & done envs, within 20 transitions


def _setup(shared):
    """clear_env (a shipped layout), heading actions, 4 envs on 4 trials."""
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    from oracle.oracle_bd import AC_INFO_KEYS, OracleAreaClearing
    cfg = default_cfg("area_clearing")
    cfg.env = "clear_env"
    cfg.agent.action_type = "heading"
    cfg.sim.t_max = T_MAX
    trials = A.generate_trials(cfg, 4)
    env = BatchedAreaClearingEnv(4, cfg={"env": "clear_env", "agent": {"action_type": "heading"}, "sim": {"t_max": T_MAX}}, trials=trials,
                                 bd_overrides={"step_limit": STEP_LIMIT})
    assert env.bd_params["t_max"] == T_MAX and env.bd_params["step_limit"] == STEP_LIMIT

    def real(tr):
        params = A.area_clearing_params(cfg)
        params["step_limit"] = STEP_LIMIT
        o = OracleAreaClearing(A.area_clearing_physics_params(cfg), params, cfg)
        o.reset(tr, observe=False)
        return o
    mk = (lambda e, tr: SharedOracle((shared, e), lambda: real(tr))) if shared else (lambda e, tr: real(tr))
    return env, AsyncRun(env, trials, mk, AC_INFO_KEYS, seed=2000, compare_alive=False)


def test_area_clearing_async_transitions_match_oracle_budgets_120_and_700():
    """Test 1 of the box-delivery file on area-clearing-v0: budgets 120 and 700, each until every env has emitted 20 transitions; each transition equals the
    oracle's step with the action the env accepted, rows of the other envs stay, ready & done envs are reset and their first observation compared.  Each run
    holds calls with a mixed ready mask, a forced STEP_LIMIT step (701 sim steps) and a reset after a truncation; the test holds a transition that took three
    calls or more (701 sim steps are six calls at 120 and two at 700; no env step of this task is longer than STEP_LIMIT + 1 + the fixed sim steps).  A delivery
    does not exist in this task."""
    most = 0
    for budget in (120, 700):
        env, r = _setup("ac")
        r.run_async(budget, 20, STEP_LIMIT)
        r.drain()
        env.check_errors()
        env.close()
        s = r.seen
        assert s["mixed"] >= 1 and s["max_substeps"] > STEP_LIMIT and s["resets"] >= 1 and s["cancelled"] == 0 and s["max_slices"] >= 2, (budget, s)
        most = max(most, s["max_slices"])
    assert most >= 3


def test_area_clearing_async_cancel_and_drain():
    """reset(mask) of a busy env cancels its env step (no transition; first observation and next transitions are a fresh oracle's); drain() finishes the busy
    envs only and closes the handle; step() matches the oracle afterwards."""
    from benchpush_amd._lib import BpError
    env, r = _setup(None)
    rdy = r.step_async(40)
    assert not rdy.any() and env.async_open
    with pytest.raises(BpError):
        env.step(torch.zeros(4, dtype=torch.float64))
    r.reset(np.array([0, 0, 1, 0], bool), "cancel")
    assert r.seen["cancelled"] == 1 and env.async_open and len(r.log[2]) == 0
    while min(len(l) for l in r.log) < 2:
        assert r.calls < 2 * math.ceil(2 * (STEP_LIMIT + 1) / 300) + 4
        r.step_async(300)
    r.drain()
    assert not env.async_open
    r.step()
    env.check_errors()
    env.close()
