"""The load-time launch plan of a ship-ice / maze handle as one table (-m gpu): scheduler chunk, pairing mode, resident workgroups and the pairing limits
that the loader settles from the policy (bp_policy.hpp) and the BP_* variables, for the smallest handles that take every decision.

Every decision below is taken on the host at load, so 8 envs are enough; BP_PAIR=2 forces the pairing plan at any size, and at 8 envs the default policy
does not pair, so its limits come from the forced case: E / 8 envs start alone, and a half leaves its pair at 16 active arbiters, 9 work units or rate 70.

A plan changes the schedule, never the result: each case then runs reset() and two step()s with fixed seeded actions and must equal, bit for bit
(torch.equal), the BP_SCHED=0 handle of the same environment.  The damping cases have no scheduler; they are compared with a BP_SCHED=0 handle of the
same damping.  The `resident` column assumes the process has the device to itself (BP_LOCK_DIR is a private directory, as in test_gpu_shared_device.py).
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E = 8
PLAN_VARS = ("BP_SCHED", "BP_SCHED_IMAGE", "BP_SCHED_YMASK", "BP_SCHED_PERSIST", "BP_SCHED_DYNPRIO", "BP_PAIR", "BP_PAIR_RESIDENT", "BP_PAIR_SOLO",
             "BP_PAIR_SNAKE", "BP_PP_KEYS", "BP_PP_SLOTS", "BP_PP_MV", "BP_PP_ACT", "BP_PP_WORK", "BP_PP_RATE", "BP_PP_SNAKE", "BP_PP_HEAVY_ONLY")
ZERO = [0] * 8
FORCED = [2, 1, 26, 34, 40, 16, 9, 70]   # mode, solo_first = E / 8, arbiter lanes, velocity slots, moving, active, work, rate
DAMP = {"sim": {"damping": 0.9}}

# (id, environment, variables, extra cfg, chunk, pair_mode, resident, pair_stats[:8])
CASES = [
    ("ship", "ship", {}, {}, 40, 0, 8, ZERO),
    ("ship-sched0", "ship", {"BP_SCHED": "0"}, {}, 0, 0, 0, ZERO),
    ("ship-sched100", "ship", {"BP_SCHED": "100"}, {}, 100, 0, 8, ZERO),
    ("ship-sched10-too-many-levels", "ship", {"BP_SCHED": "10"}, {}, 0, 0, 0, ZERO),
    ("ship-persist0", "ship", {"BP_SCHED_PERSIST": "0"}, {}, 40, 0, 0, ZERO),
    ("ship-pair1", "ship", {"BP_PAIR": "1"}, {}, 40, 1, 8, [1] + [0] * 7),
    ("ship-pair2", "ship", {"BP_PAIR": "2"}, {}, 40, 2, 8, FORCED),
    ("ship-pair2-resident0", "ship", {"BP_PAIR": "2", "BP_PAIR_RESIDENT": "0"}, {}, 40, 2, 0, FORCED),
    ("ship-pair2-sched0", "ship", {"BP_PAIR": "2", "BP_SCHED": "0"}, {}, 0, 0, 0, ZERO),   # pairing needs the scheduler
    ("ship-pair2-limits", "ship", {"BP_PAIR": "2", "BP_PAIR_SOLO": "3", "BP_PP_ACT": "5", "BP_PP_WORK": "7", "BP_PP_RATE": "33"}, {}, 40, 2, 8,
     [2, 3, 26, 34, 40, 5, 7, 33]),
    ("ship-damping", "ship", {}, DAMP, 0, 0, 0, ZERO),
    ("maze", "maze", {}, {}, 40, 0, 8, ZERO),
    ("maze-sched0", "maze", {"BP_SCHED": "0"}, {}, 0, 0, 0, ZERO),
    ("maze-damping", "maze", {}, DAMP, 0, 0, 0, ZERO),
]

_ship_trials = None
_reference = {}   # (environment, damped) -> the record of its BP_SCHED=0 handle, computed once and never changed


def _make(kind, extra):
    global _ship_trials
    if kind == "ship":
        from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
        if _ship_trials is None:
            _ship_trials = default_trials(0.1, 2, base_seed=5)
        return BatchedShipIceEnv(E, cfg=dict({"concentration": 0.1}, **extra), trials=_ship_trials, device=DEV)
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    return BatchedMazeEnv(E, cfg=dict({"num_obstacles": 5}, **extra), num_layouts=2, device=DEV)


def _record(env):
    """reset and two steps with fixed seeded actions: everything the caller reads, after each"""
    acts = torch.from_numpy(np.random.default_rng(11).uniform(-1, 1, (2, E)).astype(np.float32).astype(np.float64)).to(DEV)
    rec = []
    obs, info = env.reset()
    rec.append({"obs": obs.clone(), "info": info.clone(), "bodies": env.body_state().clone()})
    for t in range(2):
        obs, reward, terminated, truncated, info = env.step(acts[t])
        rec.append({"obs": obs.clone(), "reward": reward.clone(), "terminated": terminated.clone(), "truncated": truncated.clone(), "info": info.clone(),
                    "bodies": env.body_state().clone()})
    return rec


def _fresh(monkeypatch, tmp_path, env_vars):
    for k in PLAN_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BP_LOCK_DIR", str(tmp_path))
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    gc.collect()


@pytest.mark.parametrize("kind,env_vars,extra,chunk,pair_mode,resident,stats", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_load_plan(monkeypatch, tmp_path, kind, env_vars, extra, chunk, pair_mode, resident, stats):
    key = (kind, bool(extra))
    if key not in _reference:
        _fresh(monkeypatch, tmp_path, {"BP_SCHED": "0"})
        ref = _make(kind, extra)
        assert ref.sched_chunk() == 0
        _reference[key] = _record(ref)
        ref.check_errors()
        ref.close()
    _fresh(monkeypatch, tmp_path, env_vars)
    env = _make(kind, extra)
    got = (env.sched_chunk(), int(env.L.bp_pair_mode(env.h)), int(env.L.bp_sched_resident(env.h)), list(env.pair_stats().values())[:8])
    print("plan", kind, env_vars, extra, got)
    assert got == (chunk, pair_mode, resident, stats)
    rec = _record(env)
    assert len(rec) == len(_reference[key])
    for t, (a, b) in enumerate(zip(rec, _reference[key])):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (t, k)
    assert float(rec[2]["bodies"].sub(rec[0]["bodies"]).abs().max()) > 0.0   # not an idle window
    env.check_errors()
    env.close()
