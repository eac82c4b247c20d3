"""What bp_bd_load leaves in a box-delivery / area-clearing handle, as one table (-m gpu): body slots, the budget of the two-pass step, the dims of the
static maps, whether two trials share a layout's maps, and the layout id of the state records -- for the smallest handles that take every path of the
loader: one layout shared by both trials, two layouts, both tasks, a damping handle per task (the generic kernels), BP_BD_BUDGET unset / 0 / 120.

The expected columns were read on an MI355X from the library as it was before the loader was split into a host-only scene builder (bp_host_scene.hpp)
and named device steps; the layout ids are a compatibility surface (EnvState records carry them).  The table test passes unchanged with that earlier
library.  Each case also runs reset() and two step()s and checks the capacity flags.

test_refused_load_leaves_the_handle_as_created is the one deliberate behaviour change and fails with the earlier library, whose bp_bd_load pushed the
maps of the trials it had accepted into the handle before it refused a later trial: the retry then found stale maps in front of its own.
"""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E, T = 4, 2
OVERRIDES = {"step_limit": 500}   # the path loop's limit, lowered as the other small tests do
DAMP = {"sim": {"damping": 0.9}}
BD_DIMS, AC_DIMS, ACW_DIMS = [430, 542, 244, 244, 93, 149], [468, 468, 244, 244, 112, 112], [542, 542, 244, 244, 149, 149]

# (id, task, cfg, BP_BD_BUDGET, nb_cap, bp_bd_budget, maps(0) dims = H W SH SW si0 sj0, maps(0).cspace == maps(1).cspace, state_layout_id)
CASES = [
    ("bd-small-empty", "bd", {"env": {"obstacle_config": "small_empty"}}, None, 32, 3000, BD_DIMS, True, 0x7f27e16deaea0355),
    ("bd-small-columns", "bd", {"env": {"obstacle_config": "small_columns"}}, None, 32, 3000, BD_DIMS, False, 0x7ff82919679e54de),
    ("ac-clear-env", "ac", {"env": "clear_env"}, None, 24, 3000, AC_DIMS, True, 0x712c98867c6a1c65),
    ("ac-walled-env-with-columns", "ac", {"env": "walled_env_with_columns"}, None, 32, 3000, ACW_DIMS, True, 0xbec5bb7f99e94a70),
    ("bd-damping", "bd", dict(DAMP, env={"obstacle_config": "small_empty"}), None, 32, 3000, BD_DIMS, True, 0xee00e3d8a322e04b),
    ("ac-damping", "ac", dict(DAMP, env="clear_env"), None, 24, 3000, AC_DIMS, True, 0xa6f0e323eef89573),
    ("bd-budget0", "bd", {"env": {"obstacle_config": "small_empty"}}, "0", 32, 0, BD_DIMS, True, 0x7f27e16deaea0355),
    ("bd-budget120", "bd", {"env": {"obstacle_config": "small_empty"}}, "120", 32, 120, BD_DIMS, True, 0x7f27e16deaea0355),
]


def make(task, cfg):
    if task == "bd":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(E, cfg=cfg, num_trials=T, seed=7, device=DEV, bd_overrides=OVERRIDES)
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    return BatchedAreaClearingEnv(E, cfg=dict(cfg, agent={"action_type": "heading"}), num_trials=T, device=DEV, bd_overrides=OVERRIDES)


def loaded(env):
    """the table's columns of a handle"""
    m0, m1 = env.maps(0), env.maps(1)
    return (env.nb_cap, int(env.L.bp_bd_budget(env.h)), m0["dims"].tolist(), bool(np.array_equal(m0["cspace"], m1["cspace"])), env.state_layout_id())


@pytest.mark.parametrize("task,cfg,budget,nb_cap,bd_budget,dims,same,layout_id", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_bd_load(monkeypatch, task, cfg, budget, nb_cap, bd_budget, dims, same, layout_id):
    monkeypatch.delenv("BP_BD_BUDGET", raising=False)
    if budget is not None:
        monkeypatch.setenv("BP_BD_BUDGET", budget)
    gc.collect()
    env = make(task, cfg)
    got = loaded(env)
    print("loaded", task, cfg, budget, got[:4], "0x%016x" % got[4])
    assert got == (nb_cap, bd_budget, dims, same, layout_id)
    acts = torch.from_numpy(np.random.default_rng(11).uniform(-1, 1, (2, E))).to(DEV)
    env.reset()
    first = env.body_state().clone()
    for t in range(2):
        env.step(acts[t])
    assert float(env.body_state().sub(first).abs().max()) > 0.0   # not an idle window
    env.check_errors()
    env.close()


def test_refused_load_leaves_the_handle_as_created(monkeypatch):
    from benchpush_amd import _lib
    from benchpush_amd.box_delivery_scenario import generate_trials
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv, _bd_cfg
    monkeypatch.delenv("BP_BD_BUDGET", raising=False)
    cfg = {"env": {"obstacle_config": "small_columns"}}
    good = generate_trials(_bd_cfg(cfg), T, 7)
    k = list(good[1]["statics"][4]).index(4)
    bad = [good[0], dict(good[1], statics=tuple(np.concatenate([np.asarray(a), np.asarray(a)[k: k + 1]]) for a in good[1]["statics"]))]   # two receptacles
    fresh = BatchedBoxDeliveryEnv(E, cfg=cfg, trials=good, device=DEV, bd_overrides=OVERRIDES)
    assert not np.array_equal(fresh.maps(0)["cspace"], fresh.maps(1)["cspace"])   # two layouts: trial 0's maps were built when trial 1 is refused
    env = BatchedBoxDeliveryEnv.__new__(BatchedBoxDeliveryEnv)
    with pytest.raises(_lib.BpError, match=r"bp_bd_load failed: BP_EINVAL \(-1\) exactly one receptacle polygon per trial is required"):
        env.__init__(E, cfg=cfg, trials=bad, device=DEV, bd_overrides=OVERRIDES)
    env._load(good)   # the same handle
    assert env.state_layout_id() == fresh.state_layout_id()
    for t in range(T):
        a, b = env.maps(t), fresh.maps(t)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a), t
    assert torch.equal(env.reset()[0], fresh.reset()[0])
    for e in (env, fresh):
        e.check_errors()
        e.close()
