"""The PPO baselines of ship-ice-v0 and maze-NAMO-v0 (benchpush/baselines/{ship_ice_nav,maze_NAMO}/ppo/policy.py in the reference, where they are
stable-baselines3 wrappers) as one learner on the batched env and the device rollout buffer (benchpush_amd/rollout.py).

The loop steps `num_envs` envs of ``make_*_vec_env(to_numpy=False)``; per step: ``begin`` -> env step -> ``truncated_rows`` -> value forward on the K
bootstrap rows -> ``end``; then ``finish`` and `n_epochs` passes over the rollout's minibatches.  Nothing in the collection loop waits for the device.  A
*timestep* is one env transition, so a rollout is ``n_steps * num_envs`` of them.  The update is the clipped-surrogate PPO of stable-baselines3 2.x with
its defaults where the reference does not set a value: per-minibatch advantage normalisation, value loss MSE against the returns, ent_coef 0, vf_coef 0.5,
clip_range 0.2, max_grad_norm 0.5, Adam with eps 1e-5, gae_lambda 0.95; actions are sampled unclipped and clipped to [-1, 1] only for the env; rollouts
are collected with the network in eval mode and updates run in train mode (the extractor has batch norm).

Deviations from the reference, all stated: many envs feed one rollout instead of one; the reference unwraps the env and so never truncates, here the
TimeLimit of the registered id stays on, because an untruncated maze episode need not end (truncated steps bootstrap from V(terminal observation), as
stable-baselines3 does under a TimeLimit); an epoch's order is the rollout buffer's keyed bijection, not a ``randperm``; a model file is the
``state_dict`` of the network (``torch.save``), not stable-baselines3's zip archive.  Whether this batched schedule learns as well as the reference's
one-env loop has not been measured.
"""
import logging
import os
from typing import List, Tuple

import numpy as np
import torch

from .base_class import BasePolicy
from .feature_extractors import ActorCriticCnn

__all__ = ["DevicePPO", "PPO_DEFAULTS", "TRAIN_DEFAULTS", "ppo_loss", "to_float_rows"]

log = logging.getLogger(__name__)

# the reference's train() signatures, merged under cfg.train
TRAIN_DEFAULTS = {
    "ship_ice": dict(n_steps=256, batch_size=128, n_epochs=10, learning_rate=5e-4, gamma=0.97, total_timesteps=int(2e5), checkpoint_freq=10000),
    "maze_namo": dict(n_steps=320, batch_size=160, n_epochs=10, learning_rate=5e-4, gamma=0.995, total_timesteps=int(2e5), checkpoint_freq=10000),
}
# stable-baselines3's PPO defaults that the reference leaves alone
PPO_DEFAULTS = dict(gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, adam_eps=1e-5, bootstrap_rows=None)


def to_float_rows(obs_u8):
    """uint8 [N, ...] -> float32 in [0, 1], the rows ``DeviceRolloutBuffer`` deals.  The divisor is a tensor on the observation's device: for a scalar
    divisor torch's device kernel multiplies by the reciprocal, which rounds some byte values differently from the division."""
    return obs_u8.float() / torch.full((), 255.0, dtype=torch.float32, device=obs_u8.device)


def ppo_loss(net, batch, clip_range=0.2, ent_coef=0.0, vf_coef=0.5):
    """The loss of one minibatch (a ``RolloutBatch``) as stable-baselines3 2.x computes it, every mean and the advantage normalisation restricted to the
    rows with ``valid``.  Returns (loss, dict of detached scalars)."""
    w = batch.valid.to(torch.float32)
    n = w.sum().clamp(min=1.0)
    mean, values = net(batch.obs)
    logp = net.log_prob(mean, batch.action)
    adv = batch.advantage
    adv_mean = (adv * w).sum() / n
    adv_std = torch.sqrt((w * (adv - adv_mean) ** 2).sum() / (n - 1.0).clamp(min=1.0))      # the unbiased estimate, torch.std's default
    adv = (adv - adv_mean) / (adv_std + 1e-8)
    ratio = torch.exp(logp - batch.logp)
    policy_loss = -(torch.min(adv * ratio, adv * torch.clamp(ratio, 1.0 - clip_range, 1.0 + clip_range)) * w).sum() / n
    value_loss = (((batch.ret - values) ** 2) * w).sum() / n
    entropy = (0.5 + 0.5 * float(np.log(2.0 * np.pi)) + net.log_std).sum()                  # of the state-independent Gaussian
    loss = policy_loss - ent_coef * entropy + vf_coef * value_loss
    return loss, {"loss": loss.detach(), "policy_loss": policy_loss.detach(), "value_loss": value_loss.detach()}


class DevicePPO(BasePolicy):
    """Shared by ShipIcePPO and MazeNAMOPPO.
    model_name      model files are ``<model_path>/<model_name>.pt`` and ``<model_name>_<n>_steps.pt``; model_path defaults to ./models
    cfg             the env's configuration (dict / DotDict / None); ``train`` holds the hyper-parameters (TRAIN_DEFAULTS and PPO_DEFAULTS where absent)
    num_envs        envs of the rollout and of ``evaluate``
    env_kwargs      further keyword arguments of the batched env (trials, num_trials, layouts, device, base_seed)"""

    task = None          # "ship_ice" / "maze_namo"
    alg_name = "PPO"

    def __init__(self, model_name="ppo_model", model_path=None, cfg=None, num_envs=64, **env_kwargs) -> None:
        super().__init__()
        self.model_name = model_name
        self.model_path = model_path if model_path is not None else os.path.join(os.getcwd(), "models")
        self.cfg, self.num_envs, self.env_kwargs = cfg, int(num_envs), env_kwargs
        self.model = None
        self.device = torch.device(env_kwargs.get("device", "cuda:0"))

    # -- configuration and the pieces -----------------------------------------------------------------------------
    def train_params(self):
        p = dict(TRAIN_DEFAULTS[self.task], **PPO_DEFAULTS)
        p.update(dict((self.cfg or {}).get("train") or {}))
        return p

    def _env_cfg(self):
        return None if self.cfg is None else {k: v for k, v in dict(self.cfg).items() if k != "train"}

    def _make_vec_env(self, num_envs):
        raise NotImplementedError

    def _max_episode_steps(self):
        raise NotImplementedError

    def build_network(self, obs_shape, action_dim=1):
        return ActorCriticCnn(num_input_channels=obs_shape[0], action_dim=action_dim).to(self.device)

    def _model_file(self, model_eps="latest"):
        name = self.model_name if model_eps in (None, "latest") else "%s_%s_steps" % (self.model_name, model_eps)
        return os.path.join(self.model_path, name + ".pt")

    def _load_model(self, obs_shape, model_eps="latest"):
        net = self.build_network(obs_shape)
        net.load_state_dict(torch.load(self._model_file(model_eps), map_location=self.device))
        net.eval()
        return net

    def predict_batch(self, obs_u8):
        """uint8 [N, C, H, W] on the policy's device -> the deterministic actions float32 [N, A] (the mean, clipped to [-1, 1]).  No host read.
        The forward runs with ``torch.backends.cudnn.deterministic`` set: the convolution library's default choice for the stride-2 stages sums in an
        order that changes from call to call (the same network on the same batch differs in the last bits), and a deterministic action should not."""
        was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            with torch.no_grad():
                mean, _ = self.model(to_float_rows(obs_u8))
        finally:
            torch.backends.cudnn.deterministic = was
        return mean.clamp(-1.0, 1.0)

    # -- training ---------------------------------------------------------------------------------------------------
    def train(self, **overrides):
        """Trains for ``train.total_timesteps`` timesteps (rounded up to whole rollouts) and returns a summary dict: timesteps, updates, the last
        minibatch's loss, the model path, the checkpoint paths and the rollout buffer's ``stats()``.  Keyword arguments override ``cfg.train``."""
        from ..rollout import DeviceRolloutBuffer
        p = self.train_params()
        p.update(overrides)
        n_steps, batch_size, n_epochs, total = int(p["n_steps"]), int(p["batch_size"]), int(p["n_epochs"]), int(p["total_timesteps"])
        checkpoint_freq = int(p["checkpoint_freq"])
        os.makedirs(self.model_path, exist_ok=True)
        venv = self._make_vec_env(self.num_envs)
        E, dv = venv.num_envs, venv.env.device
        seed = int(p.get("seed", 0))
        net = self.build_network(venv.env.obs_shape)
        optimizer = torch.optim.Adam(net.parameters(), lr=float(p["learning_rate"]), eps=float(p["adam_eps"]))
        buf = DeviceRolloutBuffer(venv, n_steps, float(p["gamma"]), float(p["gae_lambda"]), seed=seed, bootstrap_rows=p["bootstrap_rows"])
        gen = torch.Generator(device=dv).manual_seed(seed)
        N = n_steps * E
        timestep, updates, epochs, info, checkpoints = 0, 0, 0, None, []
        try:
            obs = venv.reset()
            buf.reset_episode_starts()
            while timestep < total:
                net.eval()
                for _ in range(n_steps):
                    with torch.no_grad():
                        mean, values = net(to_float_rows(obs))
                        actions = mean + torch.exp(net.log_std) * torch.randn(mean.shape, device=dv, generator=gen)
                        logp = net.log_prob(mean, actions)
                    buf.begin(obs, actions, values, logp)
                    obs, reward, done, infos = venv.step(actions.clamp(-1.0, 1.0))
                    ids, rows = buf.truncated_rows(infos.truncated_mask, infos.terminal_rows)
                    with torch.no_grad():
                        boot = net.value(rows)
                    buf.end(reward, done, ids, boot)
                with torch.no_grad():
                    last_values = net.value(to_float_rows(obs))
                buf.finish(last_values)
                net.train()
                for _ in range(n_epochs):
                    for j, batch in enumerate(buf.minibatches(batch_size, epochs)):
                        nv = min(batch_size, N - j * batch_size)       # the valid rows are the first nv: a host number, batch norm sees no padding
                        loss, info = ppo_loss(net, type(batch)(*(t[:nv] for t in batch)), float(p["clip_range"]), float(p["ent_coef"]), float(p["vf_coef"]))
                        optimizer.zero_grad()
                        loss.backward()
                        torch.nn.utils.clip_grad_norm_(net.parameters(), float(p["max_grad_norm"]))
                        optimizer.step()
                        updates += 1
                    epochs += 1
                buf.clear()
                before, timestep = timestep, timestep + N
                if checkpoint_freq > 0 and timestep // checkpoint_freq != before // checkpoint_freq:
                    checkpoints.append(os.path.join(self.model_path, "%s_%d_steps.pt" % (self.model_name, timestep)))
                    torch.save(net.state_dict(), checkpoints[-1])
                log.info("timestep %d updates %d %s", timestep, updates, {k: float(v) for k, v in info.items()})   # one device read per rollout
            venv.env.check_errors()
            stats = buf.stats()
        finally:
            venv.close()
        model_file = self._model_file()
        torch.save(net.state_dict(), model_file)
        net.eval()
        self.model = net
        return {"timesteps": timestep, "updates": updates, "loss": float(info["loss"]) if info is not None else float("nan"), "model": model_file,
                "checkpoints": checkpoints, "buffer": stats}

    # -- evaluation -------------------------------------------------------------------------------------------------
    def evaluate(self, num_eps: int, model_eps: str = "latest") -> Tuple[List[float], List[float], List[float], str]:
        """Returns the reference's (efficiency scores, effort scores, rewards, 'PPO') of `num_eps` finished episodes: `num_envs` envs side by side with
        deterministic actions, every finished env starting its next episode at once; the lists come from the on-device episode metrics, in the order
        the episodes finished (env order within a step).  An episode ends when the env terminates or truncates, or at the TimeLimit of the registered id."""
        venv = self._make_vec_env(self.num_envs)
        env = venv.env
        try:
            self.model = self._load_model(env.obs_shape, model_eps)
            obs, _ = env.reset()
            age = torch.zeros(env.num_envs, dtype=torch.int64, device=env.device)
            eff, effort, rewards = [], [], []
            while len(eff) < num_eps:
                obs, _, term, trunc, _ = env.step(self.predict_batch(obs).to(torch.float64))
                age += 1
                done = term.bool() | trunc.bool() | (age >= self._max_episode_steps())
                if bool(done.any()):
                    env.reset(done)                       # a reset of a running episode closes it as truncated
                    rows, _ = env.episode_metrics()
                    for r in rows[done].cpu().numpy():
                        eff.append(float(r[0])), effort.append(float(r[1])), rewards.append(float(r[2]))
                    age = torch.where(done, torch.zeros_like(age), age)
                    obs = env.obs
            env.check_errors()
        finally:
            venv.close()
        return eff[:num_eps], effort[:num_eps], rewards[:num_eps], self.alg_name

    def act(self, observation, **kwargs):
        """The reference's call: the deterministic action (numpy float32 [A], clipped to [-1, 1]) for one observation (uint8 [C, H, W]); the first call
        loads the model (``model_eps``: a checkpoint's step count as a string, default the final model)."""
        obs = torch.as_tensor(np.ascontiguousarray(observation), dtype=torch.uint8).to(self.device)
        if self.model is None:
            self.model = self._load_model(tuple(obs.shape), kwargs.get("model_eps") or "latest")
        return self.predict_batch(obs[None])[0].cpu().numpy()
