"""The SAC baselines of ship-ice-v0 and maze-NAMO-v0 (benchpush_amd/baselines/sac.py) end to end on the device: a few steps of collection with an update
each once past ``learning_starts``, checkpoints that reload, one update held against the polyak rule, ``evaluate`` and ``act``.  The first test of a
process pays for the first use of the convolutions (about 10 s, as the SAM tests note)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN = dict(total_timesteps=48, learning_starts=8, batch_size=8, buffer_size=32, checkpoint_freq=16)
E = 4


def _one_update_follows_the_polyak_rule(pol):
    """A fresh learner, one update on a random batch: every target parameter is (1 - tau) * initial + tau * the critic's after its step."""
    from benchpush_amd.transitions import TransitionBatch
    g = torch.Generator(device=pol.device).manual_seed(5)
    learner = pol.build_learner((4, 32, 32), 1, g)
    net = learner.policy
    f = lambda *s: torch.rand(*s, device=pol.device, generator=g)   # noqa: E731
    batch = TransitionBatch(obs=f(8, 4, 32, 32), next_obs=f(8, 4, 32, 32), action=f(8, 1) * 2 - 1, reward=f(8) - 0.5, done=(f(8) < 0.3).float(),
                            slot=torch.zeros(8, dtype=torch.int32, device=pol.device), valid=torch.ones(8, dtype=torch.uint8, device=pol.device))
    target0 = {n: p.detach().clone() for n, p in net.critic_target.named_parameters()}
    net.train()
    info = learner.update(batch)
    assert all(bool(torch.isfinite(v).all()) for v in info.values())
    tau = learner.tau
    assert tau == 0.005
    critic = dict(net.critic.named_parameters())
    for n, t in net.critic_target.named_parameters():
        want = (1.0 - tau) * target0[n].double() + tau * critic[n].detach().double()
        # two float32 roundings (the scaling, the sum) on magnitudes of the parameter's own
        assert torch.allclose(t.double(), want, rtol=1e-6, atol=1e-9), n
    n = "qf0.4.bias"
    assert not torch.equal(critic[n].detach(), target0[n]) and not torch.equal(dict(net.critic_target.named_parameters())[n], target0[n])
    for (bn, a), (_, b) in zip(net.critic.named_buffers(), net.critic_target.named_buffers()):
        assert "running_" not in bn or torch.equal(a, b), "batch-norm running statistics are copied"
    assert float(learner.log_ent_coef.detach()) != 0.0


def _run(policy_cls, cfg, tmp_path, **env_kwargs):
    pol = policy_cls("sac_test", str(tmp_path), cfg, num_envs=E, **env_kwargs)
    torch.manual_seed(0)
    _one_update_follows_the_polyak_rule(pol)
    out = pol.train(**TRAIN)
    steps = 48 // E
    assert out["timesteps"] >= 48 and out["timesteps"] == steps * E and out["steps"] == steps, out
    assert out["updates"] == sum(1 for k in range(1, steps + 1) if k * E > TRAIN["learning_starts"]) == 10, out   # the steps taken past learning_starts
    assert all(np.isfinite(v) for v in out["losses"].values()) and set(out["losses"]) == {"ent_coef_loss", "critic_loss", "actor_loss", "ent_coef"}, out
    assert out["buffer"] == {"adds": steps, "draws": out["updates"], "size": 32}, out
    assert [os.path.basename(c) for c in out["checkpoints"]] == ["sac_test_16_steps.pt", "sac_test_32_steps.pt", "sac_test_48_steps.pt"]
    assert os.path.exists(out["model"]) and os.path.basename(out["model"]) == "sac_test.pt"
    assert float(pol.learner.log_ent_coef.detach()) != 0.0, "the entropy coefficient has moved"
    critic, target = pol.model.critic.state_dict(), pol.model.critic_target.state_dict()
    assert not torch.equal(critic["qf0.0.weight"], target["qf0.0.weight"]) and not torch.equal(critic["features_extractor.resnet.0.weight"],
                                                                                              target["features_extractor.resnet.0.weight"])
    assert all(bool(torch.isfinite(p).all()) for p in pol.model.parameters())
    for path in out["checkpoints"] + [out["model"]]:
        sd = torch.load(path, map_location="cpu")
        assert set(sd) == {"actor", "critic", "critic_target", "log_ent_coef"} and sd["log_ent_coef"].shape == (1,)
    early, last = torch.load(out["checkpoints"][0], map_location="cpu"), torch.load(out["model"], map_location="cpu")
    assert not torch.equal(early["actor"]["mu.weight"], last["actor"]["mu.weight"]) and float(last["log_ent_coef"]) == float(pol.learner.log_ent_coef.detach())

    # the final model reloads into a fresh policy: act is deterministic, float32 [1] in [-1, 1], and equal on two calls
    fresh = policy_cls("sac_test", str(tmp_path), cfg, num_envs=E, **env_kwargs)
    obs = torch.randint(0, 256, (4, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).numpy()
    a0, a1 = fresh.act(obs), fresh.act(obs)
    assert a0.shape == (1,) and a0.dtype == np.float32 and np.all(np.abs(a0) <= 1) and np.array_equal(a0, a1)
    for part in ("actor", "critic", "critic_target"):
        assert all(torch.equal(v.cpu(), last[part][k]) for k, v in getattr(fresh.model, part).state_dict().items()), part
    want = pol.predict_batch(torch.from_numpy(obs).to(pol.device)[None])[0].cpu().numpy()
    assert np.array_equal(a0, want), "the trained policy and the reloaded one act alike"
    other = policy_cls("sac_test", str(tmp_path), cfg, num_envs=E, **env_kwargs)
    other.act(obs, model_eps="16")
    assert not torch.equal(other.model.actor.mu.weight, fresh.model.actor.mu.weight)

    res = fresh.evaluate(2)
    assert isinstance(res, tuple) and len(res) == 4 and res[3] == "SAC"
    assert all(isinstance(l, list) and len(l) == 2 and all(isinstance(v, float) for v in l) for l in res[:3])
    assert all(np.isfinite(res[2]))


def test_ship_ice_sac_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.ship_ice_nav.sac import ShipIceSAC
    _run(ShipIceSAC, {"concentration": 0.1}, tmp_path, num_trials=4)


def test_maze_sac_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.maze_NAMO.sac import MazeNAMOSAC
    _run(MazeNAMOSAC, {}, tmp_path, num_layouts=4)
