"""The PPO baselines of ship-ice-v0 and maze-NAMO-v0 (benchpush_amd/baselines/ppo.py) end to end on the device: two tiny rollouts with an update each,
a checkpoint that reloads into a fresh policy, and ``evaluate``.  The first test of a process pays for the first use of the convolutions (about 10 s,
as the SAM tests note)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN = dict(n_steps=4, batch_size=16, n_epochs=1, total_timesteps=64, checkpoint_freq=32)


def _run(policy_cls, cfg, tmp_path, **env_kwargs):
    cfg = dict(cfg, train=TRAIN)
    pol = policy_cls("ppo_test", str(tmp_path), cfg, num_envs=8, **env_kwargs)
    torch.manual_seed(0)
    before = None

    build = pol.build_network

    def spy(*a, **k):                                     # the parameters the training starts from
        nonlocal before
        net = build(*a, **k)
        if before is None:
            before = {n: p.detach().clone() for n, p in net.named_parameters()}
        return net
    pol.build_network = spy
    out = pol.train()
    pol.build_network = build
    assert out["timesteps"] == 64 and out["updates"] == 2 * 2, out           # two rollouts of 32 transitions, two minibatches of 16 each
    assert np.isfinite(out["loss"]), out
    assert out["buffer"]["unbootstrapped"] == 0 and out["buffer"]["stored"] == 64, out
    after = dict(pol.model.named_parameters())
    changed = [n for n in before if not torch.equal(before[n], after[n].detach())]
    assert "log_std" in changed and "action_net.weight" in changed and "features_extractor.resnet.0.weight" in changed, changed
    assert all(bool(torch.isfinite(p).all()) for p in after.values())
    assert [os.path.basename(c) for c in out["checkpoints"]] == ["ppo_test_32_steps.pt", "ppo_test_64_steps.pt"]
    assert os.path.exists(out["model"]) and os.path.basename(out["model"]) == "ppo_test.pt"

    # the final model reloads into a fresh policy with identical deterministic actions; the first checkpoint is another network
    obs = torch.randint(0, 256, (3,) + tuple(pol.model.features_extractor.resnet[0].weight.shape[1:2]) + (64, 64), dtype=torch.uint8, device=pol.device)
    want = pol.predict_batch(obs)
    fresh = policy_cls("ppo_test", str(tmp_path), cfg, num_envs=8, **env_kwargs)
    got = np.stack([fresh.act(o.cpu().numpy()) for o in obs])
    assert got.shape == (3, 1) and got.dtype == np.float32 and np.all(np.abs(got) <= 1)
    assert torch.equal(fresh.predict_batch(obs), want)
    assert np.allclose(got, want.cpu().numpy(), rtol=0, atol=1e-5), "one row at a time: the convolutions may pick another algorithm"
    early = policy_cls("ppo_test", str(tmp_path), cfg, num_envs=8, **env_kwargs)
    early.act(obs[0].cpu().numpy(), model_eps="32")
    assert not torch.equal(early.model.action_net.weight, fresh.model.action_net.weight)

    res = fresh.evaluate(2)
    assert isinstance(res, tuple) and len(res) == 4 and res[3] == "PPO"
    assert all(isinstance(l, list) and len(l) == 2 and all(isinstance(v, float) for v in l) for l in res[:3])
    assert all(np.isfinite(res[2]))


def test_ship_ice_ppo_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.ship_ice_nav.ppo import ShipIcePPO
    _run(ShipIcePPO, {"concentration": 0.1}, tmp_path, num_trials=4)


def test_maze_ppo_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.maze_NAMO.ppo import MazeNAMOPPO
    _run(MazeNAMOPPO, {}, tmp_path, num_layouts=4)
