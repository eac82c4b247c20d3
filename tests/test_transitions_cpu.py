"""Device transition buffer and the SAC learner, the parts that need no GPU: the C surface and its refusals, the numpy model's own invariants, the
losses against a hand-written float64 restatement on a small stub network, the squashed Gaussian's log-probability, the polyak update, and the names
of SacPolicy."""
import copy
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import pytest

from transitions_ref import TransitionModel, image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bp_sizeof_transitions_desc", "bp_sizeof_transitions_batch", "bp_transitions_add", "bp_transitions_sample")


def test_transitions_abi_declared_and_exported_and_the_layouts_match():
    from benchpush_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "benchpush_amd.h")).read()
    L = _lib.load()
    for n in NAMES:
        assert n in _lib.ABI and n in _lib.EXPORTS and (n + "(") in hdr and hasattr(L, n), n
        assert _lib.ABI[n][2] == "bp_transitions_add"
    assert "#define BP_ABI_VERSION 11" in hdr and L.bp_abi_version() == 11
    assert L.bp_sizeof_transitions_desc() == C.sizeof(_lib.BpTransitionsDesc) == 80
    assert L.bp_sizeof_transitions_batch() == C.sizeof(_lib.BpTransitionsBatch) == 56
    assert {"bp_sizeof_transitions_desc", "bp_sizeof_transitions_batch"} <= {fn for fn, _, _ in _lib.LAYOUTS}


def _desc(_lib, **over):
    d = _lib.BpTransitionsDesc()
    d.steps, d.num_envs, d.device, d.action_dim, d.row_bytes = 4, 3, 0, 1, 16
    for i, (n, _) in enumerate(_lib.BpTransitionsDesc._fields_[5:]):
        setattr(d, n, 4096 * (i + 1))       # never dereferenced: every call below is refused before anything is launched
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_transitions_calls_refuse_bad_arguments_before_launching():
    from benchpush_amd import _lib
    L = _lib.load()
    p = C.c_void_p(4096)

    def out(**over):
        o = _lib.BpTransitionsBatch()
        for n, _ in _lib.BpTransitionsBatch._fields_:
            setattr(o, n, 4096)
        for k, v in over.items():
            setattr(o, k, v)
        return o

    def add(d, args=None):
        return L.bp_transitions_add(C.byref(d), *(args or [p] * 7), None)

    def sample(d, B=2, o=None):
        return L.bp_transitions_sample(C.byref(d), 0, B, C.byref(o if o is not None else out()), None)

    for over in (dict(row_bytes=24), dict(row_bytes=0), dict(steps=0), dict(num_envs=0), dict(action_dim=0), dict(device=-1), dict(obs=None),
                 dict(next_obs=None), dict(action=None), dict(reward=None), dict(done=None), dict(timeout=None), dict(hdr=None), dict(obs=4104),
                 dict(next_obs=4104), dict(steps=2 ** 16, num_envs=2 ** 15)):
        d = _desc(_lib, **over)
        assert add(d) == -1 and sample(d) == -1, over
    d = _desc(_lib)
    for i in range(7):
        args = [p] * 7
        args[i] = None
        assert add(d, args) == -1, "NULL argument %d" % i
    for i in range(3):
        args = [p] * 7
        args[i] = C.c_void_p(4104)
        assert add(d, args) == -1, "observation argument %d is not 16-byte aligned" % i
    assert sample(d, B=0) == -1 and sample(d, B=-4) == -1
    for n, _ in _lib.BpTransitionsBatch._fields_:
        assert sample(d, o=out(**{n: None})) == -1, n
    assert sample(d, o=out(obs=4104)) == -1 and sample(d, o=out(next_obs=4104)) == -1
    assert L.bp_transitions_add(None, p, p, p, p, p, p, p, None) == -1 and L.bp_transitions_sample(None, 0, 2, C.byref(out()), None) == -1
    assert L.bp_transitions_sample(C.byref(d), 0, 2, None, None) == -1


def _feed(m, rng, done=None, trunc=None):
    E, A, shape = m.E, m.A, m.obs_shape
    obs, nxt, term = (rng.randint(0, 256, (E,) + shape, dtype=np.uint8) for _ in range(3))
    done = (rng.rand(E) < 0.4) if done is None else done
    trunc = (rng.rand(E) < 0.5) if trunc is None else trunc
    inp = (obs, nxt, term, rng.randn(E, A).astype(np.float32), rng.randn(E), done, trunc)
    m.add(*inp)
    return inp


def test_model_ring_order_select_and_timeout_rule():
    """T = 3, E = 4: after T + 2 adds the two oldest step rows have been overwritten, in ring order, and row 2 still holds add 2."""
    rng = np.random.RandomState(0)
    m = TransitionModel(4, 13, (16,), 2, seed=5)
    assert m.T == 3 and TransitionModel(4, 3, (16,), 1).T == 1, "T = max(1, buffer_size // num_envs)"
    out = m.sample(5)
    assert not out["valid"].any() and (out["slot"] == -1).all() and not out["obs"].any() and m.hdr.tolist() == [0, 1]
    feeds = []
    for s in range(5):
        done = np.array([s % 2, 1, 0, 0], bool)
        trunc = np.array([1, 0, 1, 0], bool)                 # env 2 is truncated without being done: no timeout
        feeds.append(_feed(m, rng, done, trunc))
        assert m.stored() == min(s + 1, 3) * 4
    assert m.hdr.tolist() == [5, 1]
    for row, s in ((0, 3), (1, 4), (2, 2)):
        obs, nxt, term, action, reward, done, trunc = feeds[s]
        assert np.array_equal(m.obs[row], obs) and np.array_equal(m.action[row], action) and np.array_equal(m.reward[row], reward.astype(np.float32))
        for e in range(4):
            assert np.array_equal(m.next_obs[row, e], term[e] if done[e] else nxt[e])
        assert m.done[row].tolist() == [s % 2, 1, 0, 0] and m.timeout[row].tolist() == [s % 2, 0, 0, 0]
    out = m.sample(64)
    assert out["valid"].all() and out["slot"].min() >= 0 and out["slot"].max() < 12 and len(set(out["slot"].tolist())) > 6
    for b in range(64):
        t, e = divmod(int(out["slot"][b]), 4)
        assert out["done"][b] == (1.0 if (m.done[t, e] and not m.timeout[t, e]) else 0.0)
        assert np.array_equal(out["next_obs"][b], image(m.next_obs[t, e])) and out["reward"][b] == m.reward[t, e]
    again = TransitionModel(4, 13, (16,), 2, seed=5)
    again.hdr[1] = 1
    for f in feeds:
        again.add(*f)
    assert np.array_equal(again.sample(64)["slot"], out["slot"]), "the draw is a function of the seed, the draw number and the stored count"
    assert m.hdr.tolist() == [5, 2]


# -- the learner ---------------------------------------------------------------------------------------------------
Batch = namedtuple("Batch", ("obs", "next_obs", "action", "reward", "done"))
B, R, A, GAMMA = 6, 12, 2, 0.97


def _stub_policy(torch, seed=0):
    """SacPolicy with a flat 12 -> 8 extractor and [6, 5] hidden layers: the structure of the real one at a size a float64 restatement can walk."""
    from benchpush_amd.baselines.feature_extractors import SacPolicy
    torch.manual_seed(seed)
    pol = SacPolicy(action_dim=A, net_arch=(6, 5), make_extractor=lambda: torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(R, 8)), features_dim=8)
    with torch.no_grad():                                    # a target that differs from the critic, as after some updates
        for p in pol.critic_target.parameters():
            p.add_(0.05 * torch.randn(p.shape))
    return pol


def _stub_batch(torch, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    done = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])      # rows 0 and 3 ended; row 1 stands for a timeout: done * (1 - timeout) = 0
    return Batch(obs=torch.rand(B, R, generator=g), next_obs=torch.rand(B, R, generator=g), action=torch.tanh(r(B, A)), reward=r(B), done=done), (r(B, A), r(B, A))


def _restated_losses(torch, pol, log_ent_coef, batch, noise, gamma, target_entropy):
    """stable-baselines3's lines, written out in float64 with the layers applied by hand."""
    d = lambda t: t.detach().double()   # noqa: E731

    def mlp(x, seq):
        for layer in seq:
            x = x @ d(layer.weight).T + d(layer.bias) if isinstance(layer, torch.nn.Linear) else torch.relu(x)
        return x

    def sample(obs, eps):
        latent = mlp(mlp(obs.reshape(obs.shape[0], -1), [pol.actor.features_extractor[1]]), pol.actor.latent_pi)
        mean = latent @ d(pol.actor.mu.weight).T + d(pol.actor.mu.bias)
        log_std = torch.clamp(latent @ d(pol.actor.log_std.weight).T + d(pol.actor.log_std.bias), -20.0, 2.0)
        u = mean + torch.exp(log_std) * eps
        logp = torch.distributions.Normal(mean, torch.exp(log_std)).log_prob(u).sum(1) - torch.log(1.0 - torch.tanh(u) ** 2 + 1e-6).sum(1)
        return torch.tanh(u), logp

    def q(critic, obs, act):
        x = torch.cat([mlp(obs.reshape(obs.shape[0], -1), [critic.features_extractor[1]]), act], 1)
        return mlp(x, critic.qf0), mlp(x, critic.qf1)

    obs, nxt, act, rew, done = (d(t) for t in batch)
    a_pi, logp = sample(obs, d(noise[0]))
    lec = d(log_ent_coef)
    alpha = torch.exp(lec)
    ent_loss = -(lec * (logp + target_entropy)).mean()
    a_next, logp_next = sample(nxt, d(noise[1]))
    q0t, q1t = q(pol.critic_target, nxt, a_next)
    target = rew[:, None] + (1.0 - done[:, None]) * gamma * (torch.minimum(q0t, q1t) - alpha * logp_next[:, None])
    q0, q1 = q(pol.critic, obs, act)
    critic_loss = 0.5 * (((q0 - target) ** 2).mean() + ((q1 - target) ** 2).mean())
    q0p, q1p = q(pol.critic, obs, a_pi)
    actor_loss = (alpha * logp[:, None] - torch.minimum(q0p, q1p)).mean()
    return ent_loss, critic_loss, actor_loss, target


def test_sac_losses_equal_a_float64_restatement_and_done_masks_the_bootstrap():
    import torch
    from benchpush_amd.baselines.sac import sac_losses
    pol = _stub_policy(torch)
    batch, noise = _stub_batch(torch)
    log_ent_coef = torch.tensor([0.3], requires_grad=True)
    got = sac_losses(pol.actor, pol.critic, pol.critic_target, log_ent_coef, batch, GAMMA, -float(A), noise=noise)
    want = _restated_losses(torch, pol, log_ent_coef, batch, noise, GAMMA, -float(A))
    for name, g, w in zip(("ent_coef_loss", "critic_loss", "actor_loss"), got[:3], want[:3]):
        print(name, float(g.detach()), float(w))
        assert g.dtype == torch.float32 and torch.allclose(g.detach().double(), w, rtol=1e-5), (name, float(g.detach()), float(w))
    assert set(got[3]) == {"ent_coef_loss", "critic_loss", "actor_loss", "ent_coef"} and torch.equal(got[3]["ent_coef"], torch.exp(log_ent_coef.detach()))
    # done = 1: the target is the reward, whatever the next observation; a timeout row (done 0) keeps its bootstrap
    assert torch.equal(want[3][0, 0], batch.reward[0].double()) and torch.equal(want[3][3, 0], batch.reward[3].double())
    assert not torch.equal(want[3][1, 0], batch.reward[1].double())

    def critic_loss_with_next_row(row):
        nxt = batch.next_obs.clone()
        nxt[row] = 1.0 - nxt[row]
        return sac_losses(pol.actor, pol.critic, pol.critic_target, log_ent_coef, batch._replace(next_obs=nxt), GAMMA, -float(A), noise=noise)[1]
    assert torch.equal(critic_loss_with_next_row(0), got[1]) and torch.equal(critic_loss_with_next_row(3), got[1])
    assert not torch.equal(critic_loss_with_next_row(1), got[1])
    # the gradients go where the three optimisers step: the entropy loss to log_ent_coef alone, the critic loss to the critic alone
    got[0].backward()
    assert log_ent_coef.grad is not None and all(p.grad is None for p in pol.parameters())
    got[1].backward()
    assert all(p.grad is not None for p in pol.critic.parameters()) and all(p.grad is None for p in pol.actor.parameters())
    assert all(not p.requires_grad for p in pol.critic_target.parameters())


def test_update_steps_in_the_stated_order_and_mixes_the_target_by_tau():
    import torch
    from benchpush_amd.baselines.sac import SacLearner, sac_losses
    pol = _stub_policy(torch, seed=3)
    batch, noise = _stub_batch(torch, seed=4)
    learner = SacLearner(pol, 5e-4, GAMMA, tau=0.005)
    assert float(learner.log_ent_coef.detach()) == 0.0 and learner.target_entropy == -float(A)
    ref = copy.deepcopy(pol)
    target0 = [p.clone() for p in pol.critic_target.parameters()]
    actor0 = [p.detach().clone() for p in pol.actor.parameters()]
    info = learner.update(batch, noise=noise)
    # the same step by hand on a copy: entropy coefficient and critic first, the actor loss through the stepped critic
    lec = torch.zeros(1, requires_grad=True)
    opts = [torch.optim.Adam(ps, lr=5e-4) for ps in ([lec], ref.critic.parameters(), ref.actor.parameters())]

    def between(ent_loss, critic_loss):
        for opt, loss in zip(opts[:2], (ent_loss, critic_loss)):
            opt.zero_grad()
            loss.backward()
            opt.step()
    actor_loss = sac_losses(ref.actor, ref.critic, ref.critic_target, lec, batch, GAMMA, -float(A), noise=noise, between=between)[2]
    opts[2].zero_grad()
    actor_loss.backward()
    opts[2].step()
    assert torch.equal(lec.detach(), learner.log_ent_coef.detach()) and float(lec.detach()) != 0.0
    for a, b in zip(ref.critic.parameters(), pol.critic.parameters()):
        assert torch.equal(a, b)
    for a, b, a0 in zip(ref.actor.parameters(), pol.actor.parameters(), actor0):
        assert torch.equal(a, b) and not torch.equal(b.detach(), a0)
    assert torch.equal(info["actor_loss"], actor_loss.detach())
    for t0, t, p in zip(target0, pol.critic_target.parameters(), pol.critic.parameters()):
        want = (1.0 - 0.005) * t0.double() + 0.005 * p.detach().double()
        assert torch.allclose(t.double(), want, rtol=1e-6, atol=1e-9) and not torch.equal(t, p.detach())


def test_squashed_gaussian_log_prob_is_the_change_of_variables():
    """a = tanh(u): log p(a) = log N(u; mean, std) - sum log(da/du), da/du = 1 - tanh(u)^2 = 4 / (e^u + e^-u)^2.  The function adds 1e-6 inside the
    log; with |u| <= 2, 1 - tanh^2 >= 0.07, so each column differs by at most 1e-6 / 0.07 from the exact formula."""
    import torch
    from benchpush_amd.baselines.feature_extractors import SacActor, squashed_gaussian_log_prob
    g = torch.Generator().manual_seed(7)
    N, cols = 50, 3
    mean = torch.randn(N, cols, dtype=torch.float64, generator=g)
    log_std = torch.rand(N, cols, dtype=torch.float64, generator=g) * 2.0 - 1.5
    u = torch.rand(N, cols, dtype=torch.float64, generator=g) * 4.0 - 2.0
    got = squashed_gaussian_log_prob(mean, log_std, u)
    z = (u - mean) / torch.exp(log_std)
    gauss = (-0.5 * z ** 2 - log_std - 0.5 * math.log(2.0 * math.pi)).sum(1)
    jac = (math.log(4.0) - 2.0 * torch.log(torch.exp(u) + torch.exp(-u))).sum(1)
    assert got.shape == (N,) and float((got - (gauss - jac)).abs().max()) <= cols * 1e-6 / 0.07 + 1e-12
    assert bool((got <= gauss - jac + 1e-12).all()), "the epsilon only lowers the density"
    # the actor's sample: tanh(mean + std * noise) with this log-probability, log_std clamped to [-20, 2]
    torch.manual_seed(0)
    actor = SacActor(action_dim=cols, net_arch=(6, 5), features_extractor=torch.nn.Linear(4, 8), features_dim=8).double()
    with torch.no_grad():
        actor.log_std.bias.copy_(torch.tensor([50.0, -50.0, 0.0], dtype=torch.float64))
        obs, eps = torch.randn(N, 4, dtype=torch.float64, generator=g), torch.randn(N, cols, dtype=torch.float64, generator=g)
        m, ls = actor(obs)
        assert float(ls[:, 0].max()) == 2.0 and float(ls[:, 1].min()) == -20.0
        a, lp = actor.action_log_prob(obs, noise=eps)
        assert torch.equal(a, torch.tanh(m + torch.exp(ls) * eps)) and torch.equal(lp, squashed_gaussian_log_prob(m, ls, m + torch.exp(ls) * eps))
        assert torch.equal(actor.deterministic(obs), torch.tanh(m)) and float(a.abs().max()) <= 1.0


def test_polyak_update_with_tau_one_copies_and_tau_zero_keeps():
    import torch
    from benchpush_amd.baselines.sac import polyak_update
    g = torch.Generator().manual_seed(2)
    params = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    target = [torch.randn(3, 4, generator=g), torch.randn(5, generator=g)]
    keep = [t.clone() for t in target]
    polyak_update(params, target, 0.0)
    assert all(torch.equal(t, k) for t, k in zip(target, keep))
    polyak_update(params, target, 0.25)
    assert all(torch.allclose(t, 0.75 * k + 0.25 * p, rtol=1e-6, atol=1e-7) for t, k, p in zip(target, keep, params))
    polyak_update(params, target, 1.0)
    assert all(torch.equal(t, p) for t, p in zip(target, params))


def test_sac_policy_part_names_and_shapes():
    import torch
    from benchpush_amd.baselines.feature_extractors import SacPolicy
    torch.manual_seed(0)
    pol = SacPolicy(num_input_channels=4, action_dim=1)
    sd = {k: tuple(v.shape) for k, v in pol.state_dict().items()}
    heads = {"actor.latent_pi.0.weight": (512, 512), "actor.latent_pi.2.weight": (256, 512), "actor.mu.weight": (1, 256), "actor.mu.bias": (1,),
             "actor.log_std.weight": (1, 256), "actor.log_std.bias": (1,)}
    for part in ("critic", "critic_target"):
        for q in ("qf0", "qf1"):
            heads.update({"%s.%s.0.weight" % (part, q): (512, 513), "%s.%s.2.weight" % (part, q): (256, 512), "%s.%s.4.weight" % (part, q): (1, 256)})
    for k, shape in heads.items():
        assert sd.get(k) == shape, k
    for part in ("actor", "critic", "critic_target"):
        assert sd[part + ".features_extractor.resnet.0.weight"] == (64, 4, 7, 7)
    assert {k.split(".")[0] for k in sd} == {"actor", "critic", "critic_target"}
    assert {k.split(".")[1] for k in sd if k.startswith("actor.")} == {"features_extractor", "latent_pi", "mu", "log_std"}
    assert {k.split(".")[1] for k in sd if k.startswith("critic.")} == {"features_extractor", "qf0", "qf1"}
    assert pol.actor.features_extractor is not pol.critic.features_extractor, "share_features_extractor=False"
    assert all(torch.equal(a, b) for a, b in zip(pol.critic.state_dict().values(), pol.critic_target.state_dict().values()))
    pol.train()
    assert pol.actor.training and pol.critic.training and not pol.critic_target.training and not any(p.requires_grad for p in pol.critic_target.parameters())


def test_sac_defaults_are_the_reference_signatures():
    from benchpush_amd.baselines.maze_NAMO.sac import MazeNAMOSAC
    from benchpush_amd.baselines.ship_ice_nav.sac import ShipIceSAC
    keys = ("batch_size", "buffer_size", "learning_starts", "learning_rate", "gamma", "total_timesteps", "checkpoint_freq")
    s = ShipIceSAC("m", "/nonexistent", None).train_params()
    assert tuple(s[k] for k in keys) == (128, 15000, 200, 5e-4, 0.97, 200000, 10000)
    m = MazeNAMOSAC("m", "/nonexistent", {"train": {"batch_size": 32}}).train_params()
    assert tuple(m[k] for k in keys) == (32, 15000, 200, 5e-4, 0.995, 200000, 10000)
    assert (s["tau"], s["action_noise"], s["gradient_steps"], tuple(s["net_arch"])) == (0.005, 0.05, 1, (512, 256))
    assert ShipIceSAC.alg_name == "SAC" and ShipIceSAC("m").model_name == "m" and MazeNAMOSAC().model_name == "sac_model"
