"""The SAM baseline end to end at the smallest sizes: a training run through the ready queue and the device replay buffer, its checkpoint with the
buffer, a resumed run, evaluate and act -- for box-delivery and for area-clearing.  The ResNet at 96 px is the cost here, not the env."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TRAIN = dict(replay_buffer_size=32, learning_starts=8, batch_size=4, total_timesteps=16, target_update_freq=8, checkpoint_freq=1000, log_freq=8)


def _smoke(cls, tmp_path):
    from benchpush_amd.baselines.box_delivery.SAM.policy import DenseActionSpacePolicy
    from benchpush_amd.replay import DeviceReplayBuffer
    from test_gpu_replay import _stub_env
    kw = dict(model_name="tiny", model_path=str(tmp_path / "models"), checkpoint_root=str(tmp_path / "checkpoint"), num_envs=8, queue_batch=4,
              budget=1000, num_trials=4, bd_overrides={"step_limit": 600})
    P = 96
    torch.manual_seed(123)
    init = DenseActionSpacePolicy(P * P, 4, 0.01, device="cuda:0").policy_net.state_dict()
    torch.manual_seed(123)
    pol = cls(cfg={"train": dict(TRAIN)}, **kw)
    out = pol.train("job0")
    assert out["timesteps"] == 24 and out["updates"] == 5 and math.isfinite(out["loss"])
    assert out["buffer"]["stored"] > 0 and out["buffer"]["rejected"] == 0 and out["buffer"]["draws"] == 5
    assert os.path.exists(out["checkpoint"]) and os.path.exists(out["model"])
    model = torch.load(out["model"], map_location="cuda:0")
    assert model["timestep"] == 24 and list(model["state_dict"].keys()) == list(init.keys())
    fc, stem = "module.resnet18.fc.weight", "module.resnet18.conv1.weight"
    assert torch.equal(model["state_dict"][fc], init[fc]), "same initial weights (the unused classifier gets no gradient)"
    assert not torch.equal(model["state_dict"][stem], init[stem]) and not torch.equal(model["state_dict"]["module.conv3.weight"], init["module.conv3.weight"])
    assert all(bool(torch.isfinite(v).all()) for v in model["state_dict"].values())
    # the checkpoint carries the buffer: a fresh buffer takes it, flags re-armed
    ck = torch.load(out["checkpoint"], map_location="cuda:0")
    assert ck["timestep"] == 24 and ck["updates"] == 5 and set(ck) >= {"optimizer", "replay_buffer", "state_dict", "episode"}
    buf = DeviceReplayBuffer(_stub_env(8, P), 32)
    buf.load_state_dict(ck["replay_buffer"])
    assert buf.stats()["stored"] == out["buffer"]["stored"] and not (buf.pend_flags & 6).any()
    assert torch.equal(buf.state, ck["replay_buffer"]["state"])
    # a resumed run starts from it
    pol2 = cls(cfg={"train": dict(TRAIN, total_timesteps=20)}, **kw)
    out2 = pol2.train("job0")
    assert out2["timesteps"] == 28 and out2["updates"] == 6 and math.isfinite(out2["loss"]) and out2["buffer"]["stored"] >= out["buffer"]["stored"]
    # evaluate and act
    res = pol2.evaluate(2, max_episode_steps=3)
    assert len(res) == 5 and res[4] == "SAM_tiny"
    success, eff, effort, rewards = res[:4]
    assert len(rewards) >= 2 and len(success) == len(eff) == len(effort) == len(rewards) and all(math.isfinite(r) for r in rewards[:2])
    obs = np.random.RandomState(0).randint(0, 256, (P, P, 4)).astype(np.uint8)
    fresh = cls(cfg=None, **kw)
    with pytest.raises(ValueError):
        fresh.act(obs)
    a = fresh.act(obs, action_space=P * P, num_channels=4)
    assert type(a) is int and 0 <= a < P * P and a == pol2.act(obs)


def test_box_delivery_sam_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.box_delivery.SAM import BoxDeliverySAM
    _smoke(BoxDeliverySAM, tmp_path)


def test_area_clearing_sam_trains_checkpoints_and_evaluates(tmp_path):
    from benchpush_amd.baselines.area_clearing.sam import AreaClearingSAM
    _smoke(AreaClearingSAM, tmp_path)
