"""Device rollout buffer and the PPO networks, the parts that need no GPU: the index rule (bp_rollout_index against the model, a bijection), the GAE
model against an independent float64 evaluation, the C surface and its refusals, and the names and shapes of ActorCriticCnn."""
import ctypes as C
import os

import numpy as np
import pytest

from rollout_ref import RolloutModel, gae, rollout_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bp_sizeof_rollout_desc", "bp_sizeof_rollout_batch", "bp_rollout_index", "bp_rollout_begin", "bp_rollout_pick_rows", "bp_rollout_end",
         "bp_rollout_finish", "bp_rollout_minibatch")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 210, 1025, 4097])
def test_rollout_index_equals_the_model_and_is_a_permutation(n):
    from benchpush_amd import _lib
    L = _lib.load()
    perms = []
    for seed, epoch in ((0, 0), (0, 1), (2 ** 64 - 1, 7), (12345, 2 ** 40 + 3)):
        got = [L.bp_rollout_index(seed, epoch, i, n) for i in range(n)]
        assert got == [rollout_index(seed, epoch, i, n) for i in range(n)], (seed, epoch, n)
        assert sorted(got) == list(range(n)), "a bijection of range(n)"
        perms.append(got)
    if n >= 64:
        assert perms[0] != perms[1], "two epochs give different permutations"
        assert perms[0] != list(range(n))
    for bad_i, bad_n in ((0, 0), (0, -1), (0, 2 ** 31), (n, n), (-1, n)):
        assert L.bp_rollout_index(0, 0, bad_i, bad_n) == -1


def test_rollout_index_at_the_largest_size():
    from benchpush_amd import _lib
    L = _lib.load()
    n = 2 ** 31 - 1
    for i in (0, 1, 4097, n - 1):
        got = L.bp_rollout_index(3, 5, i, n)
        assert got == rollout_index(3, 5, i, n) and 0 <= got < n


def test_gae_model_equals_a_float64_evaluation_of_the_two_lines():
    """[3, 2] with an episode boundary in the middle (env 0 starts an episode at t = 1; env 1 is done after the last step)."""
    reward = np.array([[1.0, 0.5], [-0.25, 2.0], [0.75, -1.5]], np.float32)
    value = np.array([[0.3, -0.2], [0.9, 0.4], [-0.6, 1.1]], np.float32)
    start = np.array([[1, 1], [1, 0], [0, 0]], np.uint8)
    last_values, last_done = np.array([0.7, -0.8], np.float32), np.array([0, 1], np.uint8)
    gamma, lam = 0.97, 0.95
    adv, ret = gae(reward, value, start, last_values, last_done, gamma, lam)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    want = np.zeros((3, 2))
    last = np.zeros(2)
    for step in reversed(range(3)):                         # written independently, in float64
        if step == 2:
            non_terminal, next_values = 1.0 - last_done.astype(np.float64), last_values.astype(np.float64)
        else:
            non_terminal, next_values = 1.0 - start[step + 1].astype(np.float64), value[step + 1].astype(np.float64)
        delta = reward[step].astype(np.float64) + gamma * next_values * non_terminal - value[step].astype(np.float64)
        last = delta + gamma * lam * non_terminal * last
        want[step] = last
    eps = float(np.finfo(np.float32).eps)
    # each of the at most 3 * 6 float32 operations behind an entry rounds once, on magnitudes below 8
    assert np.all(np.abs(adv - want) <= 18 * 8 * eps)
    assert np.all(np.abs(ret - (want + value)) <= 19 * 8 * eps)
    assert adv[0, 0] == np.float32(np.float32(np.float32(1.0) + np.float32(0)) - np.float32(0.3)), "the boundary cuts the bootstrap and the trace"
    assert adv[2, 1] == np.float32(np.float32(-1.5) - np.float32(1.1)), "done after the last step: no last value"


def test_model_compaction_bootstrap_and_minibatch_rules():
    m = RolloutModel(2, 5, (16,), 1, 0.5, 0.95, seed=3)
    obs = np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    m.begin(0, obs, np.arange(5.), np.ones(5), -np.ones(5))
    ids, rows = m.pick_rows(np.array([0, 1, 0, 1, 1]), obs, 2)
    assert ids.tolist() == [1, 3] and m.hdr[0] == 1 and rows[1, 2] == np.float32(50) / np.float32(255)
    m.end(0, np.arange(5.) * 0.5, np.array([0, 1, 0, 1, 1]), ids, np.array([2.0, 4.0], np.float32))
    assert m.reward[0].tolist() == [0.0, 1.5, 1.0, 3.5, 2.0] and m.last_done.tolist() == [0, 1, 0, 1, 1] and m.hdr[1] == 5
    ids, rows = m.pick_rows(np.array([0, 0, 1, 0, 0]), obs, 3)
    assert ids.tolist() == [2, -1, -1] and not rows[1:].any() and m.hdr[0] == 1
    m.begin(1, obs, np.arange(5.), np.ones(5), -np.ones(5))
    assert m.episode_start[1].tolist() == [0, 1, 0, 1, 1]
    m.end(1, np.zeros(5), np.zeros(5))
    m.finish(np.zeros(5, np.float32))
    seen = []
    for j in range(3):
        b = m.minibatch(0, j, 4)
        seen += b["index"][b["valid"] != 0].tolist()
    assert sorted(seen) == list(range(10)) and b["valid"].tolist() == [1, 1, 0, 0] and not b["obs"][2:].any()


def test_rollout_abi_declared_and_exported_and_the_layouts_match():
    from benchpush_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "benchpush_amd.h")).read()
    L = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and (n + "(") in hdr and hasattr(L, n), n
    assert "#define BP_ABI_VERSION 11" in hdr and L.bp_abi_version() == 11
    assert L.bp_sizeof_rollout_desc() == C.sizeof(_lib.BpRolloutDesc) == 104
    assert L.bp_sizeof_rollout_batch() == C.sizeof(_lib.BpRolloutBatch) == 64


def _desc(_lib, **over):
    d = _lib.BpRolloutDesc()
    d.n_steps, d.num_envs, d.device, d.action_dim, d.row_bytes = 4, 3, 0, 1, 16
    for i, (n, _) in enumerate(_lib.BpRolloutDesc._fields_[5:]):
        setattr(d, n, 4096 * (i + 1))       # never dereferenced: every call below is refused before anything is launched
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_rollout_calls_refuse_bad_sizes_before_launching():
    from benchpush_amd import _lib
    L = _lib.load()
    p = C.c_void_p(4096)
    out = _lib.BpRolloutBatch()
    for n, _ in _lib.BpRolloutBatch._fields_:
        setattr(out, n, 4096)
    calls = {
        "begin": lambda d, t=0, a=p: L.bp_rollout_begin(C.byref(d), t, a, p, p, p, None),
        "pick": lambda d, K=2, a=p: L.bp_rollout_pick_rows(C.byref(d), a, p, K, p, p, None),
        "end": lambda d, t=0, K=2, a=p: L.bp_rollout_end(C.byref(d), t, a, p, p, p, K, 0.9, None),
        "finish": lambda d, a=p: L.bp_rollout_finish(C.byref(d), a, 0.9, 0.85, None),
        "minibatch": lambda d, j=0, B=2, o=out: L.bp_rollout_minibatch(C.byref(d), 0, 0, j, B, C.byref(o), None),
    }
    for over in (dict(row_bytes=24), dict(row_bytes=0), dict(n_steps=0), dict(num_envs=0), dict(action_dim=0), dict(obs=None), dict(ret=None),
                 dict(last_done=None), dict(hdr=None), dict(obs=4104)):
        d = _desc(_lib, **over)
        for name, call in calls.items():
            assert call(d) == -1, (name, over)
    d = _desc(_lib)
    for name, call in calls.items():
        assert call(d, a=None) == -1 if name != "minibatch" else call(d, o=_lib.BpRolloutBatch()) == -1, name + ": NULL arrays"
    assert calls["begin"](d, t=4) == -1 and calls["begin"](d, t=-1) == -1
    assert calls["end"](d, t=4) == -1 and calls["end"](d, t=-1) == -1 and calls["end"](d, K=0) == -1
    assert L.bp_rollout_end(C.byref(d), 0, p, p, p, None, 2, 0.9, None) == -1, "boot_ids without boot_values"
    assert calls["pick"](d, K=0) == -1 and calls["pick"](d, K=-3) == -1
    assert calls["minibatch"](d, B=0) == -1 and calls["minibatch"](d, j=-1) == -1 and calls["minibatch"](d, j=6, B=2) == -1
    assert L.bp_rollout_begin(None, 0, p, p, p, p, None) == -1


# -- the networks --------------------------------------------------------------------------------------------------
def _block(prefix, w_in, w, down):
    keys = {prefix + "conv1.weight": (w, w_in, 3, 3), prefix + "conv2.weight": (w, w, 3, 3)}
    for bn, width in (("bn1", w), ("bn2", w)) + ((("downsample.1", w),) if down else ()):
        keys.update({prefix + bn + ".weight": (width,), prefix + bn + ".bias": (width,), prefix + bn + ".running_mean": (width,),
                     prefix + bn + ".running_var": (width,), prefix + bn + ".num_batches_tracked": ()})
    if down:
        keys[prefix + "downsample.0.weight"] = (w, w_in, 1, 1)
    return keys


def _expected_keys(channels, action_dim):
    fe = "features_extractor.resnet."
    keys = {fe + "0.weight": (64, channels, 7, 7), fe + "1.weight": (64,), fe + "1.bias": (64,), fe + "1.running_mean": (64,),
            fe + "1.running_var": (64,), fe + "1.num_batches_tracked": ()}
    w_in = 64
    for stage, w in zip((4, 5, 6, 7), (64, 128, 256, 512)):
        keys.update(_block("%s%d.0." % (fe, stage), w_in, w, w != w_in))
        keys.update(_block("%s%d.1." % (fe, stage), w, w, False))
        w_in = w
    for net in ("policy_net", "value_net"):
        keys.update({"mlp_extractor.%s.0.weight" % net: (512, 512), "mlp_extractor.%s.0.bias" % net: (512,),
                     "mlp_extractor.%s.2.weight" % net: (256, 512), "mlp_extractor.%s.2.bias" % net: (256,)})
    keys.update({"action_net.weight": (action_dim, 256), "action_net.bias": (action_dim,), "value_net.weight": (1, 256), "value_net.bias": (1,),
                 "log_std": (action_dim,)})
    return keys


def test_actor_critic_key_names_and_shapes():
    import torch
    from benchpush_amd.baselines.feature_extractors import ActorCriticCnn
    torch.manual_seed(0)
    net = ActorCriticCnn(num_input_channels=4, action_dim=1)
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == _expected_keys(4, 1)
    assert len(got) == 6 + 8 * 12 + 3 * 6 + 8 + 5, "stem, eight blocks, three downsample paths, the two heads' layers, heads and log_std"
    assert float(net.log_std.detach().abs().sum()) == 0.0 and float(net.action_net.bias.detach().abs().sum()) == 0.0
    assert [type(m).__name__ for m in net.features_extractor.resnet] == ["Conv2d", "BatchNorm2d", "ReLU", "MaxPool2d", "Sequential", "Sequential",
                                                                          "Sequential", "Sequential", "AdaptiveAvgPool2d"]


def test_actor_critic_float64_forward_is_deterministic_and_finite():
    import torch
    from benchpush_amd.baselines.feature_extractors import ActorCriticCnn
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        net = ActorCriticCnn(num_input_channels=4, action_dim=1).double().eval()
        x = torch.rand(2, 4, 32, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        with torch.no_grad():
            mean, value = net(x)
            logp = net.log_prob(mean, mean + 0.5)
        assert mean.shape == (2, 1) and value.shape == (2,) and logp.shape == (2,)
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(value).all())
        assert torch.allclose(logp, torch.full((2,), -0.125 - 0.5 * float(np.log(2 * np.pi)), dtype=torch.float64), atol=1e-12)
        assert torch.equal(net.value(x), value)
        outs.append((mean, value))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_ppo_defaults_are_the_reference_signatures():
    from benchpush_amd.baselines.maze_NAMO.ppo import MazeNAMOPPO
    from benchpush_amd.baselines.ship_ice_nav.ppo import ShipIcePPO
    s = ShipIcePPO("m", "/nonexistent", None).train_params()
    assert (s["n_steps"], s["batch_size"], s["n_epochs"], s["learning_rate"], s["gamma"]) == (256, 128, 10, 5e-4, 0.97)
    m = MazeNAMOPPO("m", "/nonexistent", {"train": {"n_epochs": 3}}).train_params()
    assert (m["n_steps"], m["batch_size"], m["n_epochs"], m["learning_rate"], m["gamma"]) == (320, 160, 3, 5e-4, 0.995)
    assert (s["gae_lambda"], s["clip_range"], s["ent_coef"], s["vf_coef"], s["max_grad_norm"], s["adam_eps"]) == (0.95, 0.2, 0.0, 0.5, 0.5, 1e-5)


def test_ppo_loss_restricts_every_mean_to_the_valid_rows():
    import torch
    from benchpush_amd.baselines.feature_extractors import ActorCriticCnn
    from benchpush_amd.baselines.ppo import ppo_loss
    from benchpush_amd.rollout import RolloutBatch
    torch.manual_seed(2)
    net = ActorCriticCnn(4, 1).double().eval()
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)   # noqa: E731
    full = RolloutBatch(obs=torch.rand(3, 4, 32, 32, dtype=torch.float64, generator=g), action=r(3, 1), value=r(3), logp=r(3) - 1, advantage=r(3),
                        ret=r(3), index=torch.arange(3, dtype=torch.int32), valid=torch.ones(3, dtype=torch.uint8))
    pad = lambda t: torch.cat([t, torch.zeros_like(t[:2])])   # noqa: E731
    padded = RolloutBatch(*(pad(t) for t in full))
    with torch.no_grad():
        a, _ = ppo_loss(net, full)
        b, info = ppo_loss(net, padded)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12) and set(info) == {"loss", "policy_loss", "value_loss"}
    with torch.no_grad():                                    # stable-baselines3's lines on the valid rows
        mean, values = net(full.obs)
        logp = net.log_prob(mean, full.action)
        adv = (full.advantage - full.advantage.mean()) / (full.advantage.std() + 1e-8)
        ratio = torch.exp(logp - full.logp)
        want = -torch.min(adv * ratio, adv * torch.clamp(ratio, 0.8, 1.2)).mean() + 0.5 * torch.nn.functional.mse_loss(full.ret, values)
    assert torch.allclose(a, want, rtol=1e-12, atol=1e-12)
