"""BoxDeliverySAM: the reference's spatial-action-map baseline (benchpush/baselines/box_delivery/SAM/policy.py) -- a double DQN whose Q-network gives one
value per pixel of the 96-px observation, the action being the pixel to drive to -- on the batched env and the ready queue.

The rollout is ``env.async_queue(M)`` with a ``DeviceReplayBuffer`` attached (benchpush_amd/replay.py): recv -> ``predict_batch`` -> send, with resets of
the finished envs inside the send, then `updates_per_recv` updates on ``buf.sample(batch_size)``.  Nothing in that loop waits for the device.  A *timestep*
is one delivered row slot: the host counter ``calls * M``, an upper bound of the rows actually delivered (a recv may hand out fewer than M rows).

Differences from the reference's loop, all stated: many envs feed one buffer and the learner does `updates_per_recv` updates per M row slots instead of one
per env step; the buffer samples with replacement; a terminated step has no next state (``nonfinal``), which for a truncated episode (the env sets both
flags then) is what the reference does too.  Whether this batched schedule learns as well as the reference's one-env loop has not been measured.
tensorboard is optional: scalars go to ``logging``, and to a ``SummaryWriter`` where one can be imported.
"""
import copy
import logging
import os
from datetime import datetime

import numpy as np
import torch
from torch.nn.functional import smooth_l1_loss

from ...base_class import BasePolicy
from ...feature_extractors import DenseActionSpaceDQN

__all__ = ["BoxDeliverySAM", "DenseActionSpacePolicy", "SpatialActionMapBaseline", "TRAIN_DEFAULTS", "double_dqn_target", "to_float_planes"]

log = logging.getLogger(__name__)

# the reference's `train:` values (box_delivery/config.yaml), merged under cfg.train; the two schedule keys below them are this project's
TRAIN_DEFAULTS = dict(batch_size=32, learning_rate=0.01, gamma=0.99, replay_buffer_size=10000, learning_starts=1000, exploration_timesteps=6000,
                      final_exploration=0.01, target_update_freq=1000, grad_norm_clipping=10, weight_decay=1e-4, total_timesteps=60000,
                      checkpoint_freq=6000, resume_training=False, job_id_to_resume=None,
                      updates_per_recv=1, log_freq=1000)


def to_float_planes(obs_u8):
    """uint8 [N, P, P, 4] -> float32 [N, 4, P, P] in [0, 1]: what ToTensor() gives, and what ``DeviceReplayBuffer.sample`` returns.  The divisor is a
    tensor on the observation's device: for a scalar divisor torch's device kernel multiplies by the reciprocal, which rounds 126 of the 256 byte values
    differently from the division that ToTensor() performs on the host."""
    return obs_u8.permute(0, 3, 1, 2).float() / torch.full((), 255.0, dtype=torch.float32, device=obs_u8.device)


def double_dqn_target(reward, ministeps, nonfinal, q_policy_next, q_target_next, gamma):
    """r + gamma ** ministeps * nonfinal * Q_target(s', argmax_a Q_policy(s', a)); the Q tensors are [B, A]."""
    best = q_policy_next.argmax(dim=1, keepdim=True)
    nxt = q_target_next.gather(1, best).squeeze(1)
    return reward + torch.pow(torch.tensor(gamma, dtype=reward.dtype, device=reward.device), ministeps) * nonfinal.to(reward.dtype) * nxt


def _writer(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=log_dir)
    except Exception:
        return None


class DenseActionSpacePolicy:
    """The Q-network and the epsilon-greedy choice over its map.  action_space: the number of actions, P * P.  The network sits in a ``DataParallel`` on
    one device, so its ``state_dict`` has the reference's ``module.`` names.  A model file is ``{'timestep', 'state_dict'}``."""

    def __init__(self, action_space, num_input_channels, final_exploration, train=False, model_file=None, random_seed=None, device=None):
        self.action_space = int(np.asarray(action_space).reshape(-1)[0])
        self.num_input_channels = int(num_input_channels)
        self.final_exploration = float(final_exploration)
        self.train = train
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.policy_net = self.build_network()
        if model_file is not None:
            ck = torch.load(model_file, map_location=self.device)
            self.policy_net.load_state_dict(ck["state_dict"])
            log.info("=> loaded model '%s'", model_file)
        self.policy_net.train(bool(train))
        seed = 0 if random_seed is None else int(random_seed)
        self.rng = np.random.RandomState(seed)                                   # predict: one observation, on the host
        self.generator = torch.Generator(device=self.device).manual_seed(seed)   # predict_batch: on the device

    def build_network(self):
        net = DenseActionSpaceDQN(num_input_channels=self.num_input_channels).to(self.device)
        ids = [self.device.index if self.device.index is not None else torch.cuda.current_device()] if self.device.type == "cuda" else None
        return torch.nn.DataParallel(net, device_ids=ids)

    def apply_transform(self, s):
        return to_float_planes(torch.as_tensor(np.ascontiguousarray(s))[None])

    def predict(self, state, exploration_eps=None, debug=False):
        """One observation (numpy uint8 [P, P, 4]) -> (action, info), the reference's return: the action an int in [0, P * P)."""
        if exploration_eps is None:
            exploration_eps = self.final_exploration
        with torch.no_grad():
            output = self.policy_net(self.apply_transform(state).to(self.device)).squeeze(0)
        if self.rng.random_sample() < exploration_eps:
            action = int(self.rng.randint(self.action_space))
        else:
            action = int(output.reshape(1, -1).argmax(1).item())
        return action, ({"output": output.squeeze(0)} if debug else {})

    def predict_batch(self, obs_u8, exploration_eps=None):
        """uint8 [M, P, P, 4] on the policy's device -> int64 [M]: the argmax over each row's flattened map, or -- per row, with probability
        `exploration_eps` -- a uniform action; the draws come from the policy's seeded device generator.  No host synchronisation."""
        if exploration_eps is None:
            exploration_eps = self.final_exploration
        M = obs_u8.shape[0]
        with torch.no_grad():
            greedy = self.policy_net(to_float_planes(obs_u8)).reshape(M, -1).argmax(1)
        if exploration_eps <= 0:
            return greedy
        explore = torch.rand(M, device=self.device, generator=self.generator) < float(exploration_eps)
        uniform = torch.randint(self.action_space, (M,), device=self.device, generator=self.generator)
        return torch.where(explore, uniform, greedy)


class SpatialActionMapBaseline(BasePolicy):
    """Shared by BoxDeliverySAM and AreaClearingSAM.
    cfg             the env's configuration (dict / DotDict / None); ``train`` holds the hyper-parameters (TRAIN_DEFAULTS where absent)
    model_name      model files are ``<model_path>/<model_name>.pt``; model_path defaults to ./models, checkpoint_root to ./checkpoint
    num_envs        envs of the rollout and of ``evaluate``; queue_batch: rows per recv, M (None: num_envs // 2, at least 1)
    env_kwargs      further keyword arguments of the env (trials, num_trials, device, bd_overrides)"""

    task = None          # "box_delivery" / "area_clearing"
    alg_name = "SAM"

    def __init__(self, cfg=None, model_name="sam_model", model_path=None, num_envs=64, queue_batch=None, budget=None, checkpoint_root=None,
                 **env_kwargs) -> None:
        super().__init__()
        self.cfg = cfg
        self.model_name = model_name
        self.model_path = model_path if model_path is not None else os.path.join(os.getcwd(), "models")
        self.checkpoint_root = checkpoint_root if checkpoint_root is not None else os.path.join(os.getcwd(), "checkpoint")
        self.num_envs = int(num_envs)
        self.queue_batch = int(queue_batch) if queue_batch is not None else max(1, self.num_envs // 2)
        self.budget, self.env_kwargs = budget, env_kwargs
        self.model = None
        self.device = torch.device(env_kwargs.get("device", "cuda:0") if torch.cuda.is_available() else "cpu")

    # -- configuration -----------------------------------------------------------------------------------------
    def sam_cfg(self):
        """A copy of the cfg as the reference's SAM job sets it: position actions, job type 'sam' (96-px observations and the SAM reward / inactivity
        values where the task has them) and the train defaults under ``train``."""
        from ....config import DotDict, default_cfg, merge_user_cfg
        c = merge_user_cfg(default_cfg(self.task), copy.deepcopy(self.cfg))
        c.agent.action_type = "position"
        train = DotDict(TRAIN_DEFAULTS)
        train.update(c.get("train") or {})
        train.job_type = "sam"
        c.train = train
        return self._task_cfg(c)

    def _task_cfg(self, c):
        return c

    def _make_env(self, num_envs, cfg):
        raise NotImplementedError

    # -- one learner update ---------------------------------------------------------------------------------------
    def update_policy(self, policy_net, target_net, optimizer, batch):
        """One double-DQN step on a ``ReplayBatch``: smooth-L1 between Q(s, a) and ``double_dqn_target``, each sample weighted by ``valid``."""
        B = batch.action.shape[0]
        output = policy_net(batch.state)
        q = output.reshape(B, -1).gather(1, batch.action.unsqueeze(1)).squeeze(1)
        with torch.no_grad():
            target = double_dqn_target(batch.reward, batch.ministeps, batch.nonfinal, policy_net(batch.next_state).reshape(B, -1),
                                       target_net(batch.next_state).reshape(B, -1), self.gamma)
        valid = batch.valid.to(q.dtype)
        loss = (smooth_l1_loss(q, target, reduction="none") * valid).mean()
        optimizer.zero_grad()
        loss.backward()
        if self.grad_norm_clipping is not None:
            torch.nn.utils.clip_grad_norm_(policy_net.parameters(), self.grad_norm_clipping)
        optimizer.step()
        return {"q_value_min": output.detach().min(), "q_value_max": output.detach().max(),
                "td_error": ((q - target).abs() * valid).detach().mean(), "loss": loss.detach()}

    # -- training ---------------------------------------------------------------------------------------------------
    def train(self, job_id):
        """Trains for ``train.total_timesteps + train.learning_starts`` timesteps (row slots, see the module's docstring) and returns a summary dict:
        timesteps, updates, the last update's loss, the checkpoint and model paths.  Checkpoints -- model, optimizer and the replay buffer -- go to
        ``<checkpoint_root>/<job_id>/`` every ``checkpoint_freq`` timesteps and at the end; the final model also to ``<model_path>/<model_name>.pt``."""
        from ....replay import DeviceReplayBuffer
        cfg = self.sam_cfg()
        p = cfg.train
        self.batch_size, self.gamma, self.grad_norm_clipping = int(p.batch_size), float(p.gamma), p.grad_norm_clipping
        self.final_exploration = float(p.final_exploration)
        learning_starts, exploration_timesteps = int(p.learning_starts), int(p.exploration_timesteps)
        target_update_freq, checkpoint_freq, log_freq = int(p.target_update_freq), int(p.checkpoint_freq), int(p.log_freq)
        total = int(p.total_timesteps) + learning_starts
        ck_dir = os.path.join(self.checkpoint_root, str(job_id))
        ck_path = os.path.join(ck_dir, "checkpoint-%s.pt" % self.model_name)
        os.makedirs(ck_dir, exist_ok=True)
        log.info("starting training, job %s", job_id)

        env = self._make_env(self.num_envs, cfg)
        seed = int(cfg.misc.random_seed) if "misc" in cfg and cfg.misc.get("random_seed") is not None else 0
        P = env.obs_shape[0]
        policy = DenseActionSpacePolicy(P * P, env.obs_shape[2], self.final_exploration, train=True, random_seed=seed, device=env.device)
        optimizer = torch.optim.SGD(policy.policy_net.parameters(), lr=float(p.learning_rate), momentum=0.9, weight_decay=float(p.weight_decay))
        buf = DeviceReplayBuffer(env, int(p.replay_buffer_size), seed=seed)
        timestep, updates = 0, 0
        load_from = ck_path
        if p.resume_training and p.job_id_to_resume is not None:
            load_from = os.path.join(self.checkpoint_root, str(p.job_id_to_resume), "checkpoint-%s.pt" % self.model_name)
        if os.path.exists(load_from):
            ck = torch.load(load_from, map_location=env.device)
            timestep, updates = int(ck["timestep"]), int(ck.get("updates", 0))
            policy.policy_net.load_state_dict(ck["state_dict"])
            optimizer.load_state_dict(ck["optimizer"])
            buf.load_state_dict(ck["replay_buffer"])
            log.info("=> loaded checkpoint '%s' (timestep %d)", load_from, timestep)
        target_net = policy.build_network()
        target_net.load_state_dict(policy.policy_net.state_dict())
        target_net.eval()
        writer = _writer(os.path.join(ck_dir, "logs"))

        def save(ts):
            model = {"timestep": ts, "state_dict": policy.policy_net.state_dict()}
            torch.save(model, os.path.join(ck_dir, "model-%s%d.pt" % (self.model_name, ts)))
            tmp = os.path.join(ck_dir, "checkpoint-temp.pt")
            torch.save({"timestep": ts, "updates": updates, "episode": int(env.episode_metrics()[1].sum().item()),
                        "state_dict": policy.policy_net.state_dict(), "optimizer": optimizer.state_dict(), "replay_buffer": buf.state_dict()}, tmp)
            os.replace(tmp, ck_path)     # the checkpoint is either the old or the new one, never half of one
            log.info("%s: checkpoint saved at %s", datetime.now().strftime("%Y-%m-%d %H:%M:%S"), ck_path)
            return model

        env.reset()
        M = self.queue_batch
        q = env.async_queue(M, self.budget)
        batch, info, model = None, None, None
        try:
            while timestep < total:
                ids, obs, _, terminated, truncated, _ = buf.recv(q)
                if exploration_timesteps > 0:
                    eps = 1 - min(max(timestep - learning_starts, 0) / exploration_timesteps, 1) * (1 - self.final_exploration)
                else:
                    eps = self.final_exploration
                actions = policy.predict_batch(obs, eps)
                buf.send(q, actions.to(torch.float64), ids, reset=terminated | truncated)
                before, timestep = timestep, min(timestep + M, total)
                if timestep >= learning_starts:
                    for _ in range(int(p.updates_per_recv)):
                        batch = buf.sample(self.batch_size, out=batch)
                        info = self.update_policy(policy.policy_net, target_net, optimizer, batch)
                        updates += 1
                if timestep // target_update_freq != before // target_update_freq:
                    target_net.load_state_dict(policy.policy_net.state_dict())
                if info is not None and timestep // log_freq != before // log_freq:
                    vals = {k: float(v) for k, v in info.items()}           # the loop's only device reads, every log_freq timesteps
                    log.info("timestep %d eps %.3f %s %s", timestep, eps, vals, buf.stats())
                    if writer is not None:
                        for k, v in vals.items():
                            writer.add_scalar(k, v, timestep)
                if timestep // checkpoint_freq != before // checkpoint_freq or timestep == total:
                    model = save(timestep)
            q.close()
            env.check_errors()
        finally:
            env.close()
            if writer is not None:
                writer.close()
        os.makedirs(self.model_path, exist_ok=True)
        model_file = os.path.join(self.model_path, "%s.pt" % self.model_name)
        if model is not None:
            torch.save(model, model_file)
        self.model = policy
        policy.policy_net.eval()
        return {"timesteps": timestep, "updates": updates, "loss": float(info["loss"]) if info is not None else float("nan"),
                "checkpoint": ck_path, "model": model_file, "buffer": buf.stats()}

    # -- evaluation -------------------------------------------------------------------------------------------------
    def _load_model(self, action_space, num_channels, model_eps="latest"):
        name = self.model_name if model_eps == "latest" else "%s_%s_steps" % (self.model_name, model_eps)
        return DenseActionSpacePolicy(action_space, num_channels, 0.0, train=False, model_file=os.path.join(self.model_path, name + ".pt"),
                                      device=self.device)

    def evaluate(self, num_eps: int, model_eps: str = "latest", max_episode_steps=None):
        """Returns (success rates, efficiency scores, effort scores, rewards, 'SAM_<model_name>') of `num_eps` finished episodes: the policy's `num_envs`
        envs side by side with ``step()`` at epsilon 0, every finished env starting its next episode at once; the four lists come from the on-device
        episode metrics (``episode_metrics()``, the reference's TaskDrivenMetric), in the order the episodes finished (env order within a step).  An episode
        ends when the env terminates or truncates, or after `max_episode_steps` steps (None: no limit beside the env's own); the reset that follows
        closes it as truncated."""
        cfg = self.sam_cfg()
        env = self._make_env(self.num_envs, cfg)
        try:
            P = env.obs_shape[0]
            self.model = self._load_model(P * P, env.obs_shape[2], model_eps)
            obs, _ = env.reset()
            age = torch.zeros(env.num_envs, dtype=torch.int64, device=env.device)
            success, eff, effort, rewards = [], [], [], []
            while len(eff) < num_eps:
                obs, _, term, trunc, _ = env.step(self.model.predict_batch(obs, 0.0).to(torch.float64))
                age += 1
                done = term.bool() | trunc.bool()
                if max_episode_steps is not None:
                    done = done | (age >= int(max_episode_steps))
                if bool(done.any()):
                    env.reset(done)
                    rows, _ = env.episode_metrics()
                    for r in rows[done].cpu().numpy():
                        eff.append(float(r[0])), effort.append(float(r[1])), rewards.append(float(r[2])), success.append(float(r[3]))
                    age = torch.where(done, torch.zeros_like(age), age)
                    obs = env.obs
            env.check_errors()
        finally:
            env.close()
        return success, eff, effort, rewards, f"SAM_{self.model_name}"

    def act(self, observation, action_space: int = None, num_channels: int = None, model_eps="latest"):
        """The reference's call: the greedy action (an int) for one observation (numpy uint8 [P, P, 4]); the first call loads the model and needs
        `action_space` (P * P) and `num_channels`."""
        if self.model is None:
            if action_space is None or num_channels is None:
                raise ValueError("action_space and num_channels must be provided")
            self.model = self._load_model(action_space, num_channels, model_eps)
        action, _ = self.model.predict(observation, 0.0)
        return action


class BoxDeliverySAM(SpatialActionMapBaseline):
    task = "box_delivery"

    def _make_env(self, num_envs, cfg):
        from ....envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(num_envs, cfg=cfg, **self.env_kwargs)
