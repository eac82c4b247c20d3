"""DeviceRolloutBuffer: the on-policy learner's half of the step loop, on the device (bp_rollout_*; DESIGN.md "Rollout buffer").

``BatchedVecEnv(to_numpy=False)`` hands out E device-resident transitions per step.  This class keeps `n_steps` of them -- the observation batch the
policy acted on, actions, values, log-probabilities, rewards, episode starts --, bootstraps the reward of time-limit truncations, computes advantages and
returns by generalised advantage estimation and deals shuffled float minibatches, with one library call each and no host read:

    buf = DeviceRolloutBuffer(vec_env, n_steps, gamma, gae_lambda)
    obs = vec_env.reset()
    for t in range(n_steps):
        buf.begin(obs, actions, values, logp)                         # before the env step: the env rewrites `obs` in place
        obs, reward, done, infos = vec_env.step(clipped_actions)
        ids, rows = buf.truncated_rows(infos.truncated_mask, infos.terminal_rows)
        buf.end(reward, done, ids, value_of(rows))                    # reward += gamma * V(terminal observation) where the time limit cut the episode
    buf.finish(value_of(obs))
    for epoch in range(n_epochs):
        for batch in buf.minibatches(batch_size, epoch): ...
    buf.clear()

The rules are those of stable-baselines3's RolloutBuffer and ``collect_rollouts`` (float32 GAE in its order of operations, the truncation bootstrap);
an epoch's order is a keyed bijection of range(n_steps * num_envs) (``bp_rollout_index``) instead of a ``randperm``.  ``stats()`` is the only host read.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .envs.batched import _ptr

__all__ = ["DeviceRolloutBuffer", "RolloutBatch"]

RolloutBatch = namedtuple("RolloutBatch", ("obs", "action", "value", "logp", "advantage", "ret", "index", "valid"))
_F32 = ("action", "reward", "value", "logp", "advantage", "ret")
_TENSORS = (("obs", torch.uint8),) + tuple((n, torch.float32) for n in _F32) + (("episode_start", torch.uint8), ("last_done", torch.uint8),
                                                                                  ("hdr", torch.int64))
_U8 = (torch.uint8, torch.bool)


class DeviceRolloutBuffer:
    """`n_steps` steps of the `num_envs` envs of a batched env (or the BatchedVecEnv around it) with uint8 observations.  Tensors, all on the env's device:
    obs uint8 [T, E, *obs_shape]; action float32 [T, E, A]; reward, value, logp, advantage, ret float32 [T, E]; episode_start uint8 [T, E]; last_done
    uint8 [E]; hdr int64 [2] = truncated rows left without a bootstrap (more than `bootstrap_rows` envs truncated in one step), rows stored.
    bootstrap_rows (K, default num_envs: nothing overflows) is the size of the fixed batch ``truncated_rows`` returns."""

    def __init__(self, env, n_steps, gamma, gae_lambda, seed=0, bootstrap_rows=None):
        env = env.env if hasattr(env, "step_wait") else env          # a BatchedVecEnv: the batched env inside
        if bool(getattr(getattr(env, "cfg", None), "low_dim_state", False)) or env.obs.dtype != torch.uint8:
            raise ValueError("DeviceRolloutBuffer: only uint8 image observations are supported (low_dim_state observations are not)")
        self.n_steps, self.gamma, self.gae_lambda, self.seed = int(n_steps), float(gamma), float(gae_lambda), int(seed)
        self.L, self.device = env.L, env.device
        self.num_envs, self.obs_shape = int(env.num_envs), tuple(env.obs_shape)
        self.action_dim = int(getattr(env, "action_dim", 1))
        self.row_bytes = int(np.prod(self.obs_shape))
        self.bootstrap_rows = self.num_envs if bootstrap_rows is None else int(bootstrap_rows)
        T, E, A = self.n_steps, self.num_envs, self.action_dim
        if T < 1 or T * E > 0x7FFFFFFF:
            raise ValueError("DeviceRolloutBuffer: n_steps must be at least 1 and n_steps * num_envs at most 2^31 - 1")
        if self.row_bytes % 16:
            raise ValueError("DeviceRolloutBuffer: observation rows of %s are %d bytes, not a multiple of 16" % (self.obs_shape, self.row_bytes))
        if not 1 <= self.bootstrap_rows <= E:
            raise ValueError("DeviceRolloutBuffer: bootstrap_rows must be 1 .. num_envs")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)   # noqa: E731
        self.obs = z((T, E) + self.obs_shape, torch.uint8)
        self.action = z((T, E, A), torch.float32)
        self.reward, self.value, self.logp, self.advantage, self.ret = (z((T, E), torch.float32) for _ in range(5))
        self.episode_start, self.last_done, self.hdr = z((T, E), torch.uint8), z(E, torch.uint8), z(2, torch.int64)
        self._boot_ids = z(self.bootstrap_rows, torch.int32)
        self._boot_rows = z((self.bootstrap_rows,) + self.obs_shape, torch.float32)
        self._batch = None
        self.t, self._open, self._finished = 0, False, False      # steps stored; a begin awaits its end; advantages are computed
        d = _lib.BpRolloutDesc()
        d.n_steps, d.num_envs, d.action_dim, d.row_bytes = T, E, A, self.row_bytes
        d.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        for n, _ in _TENSORS:
            setattr(d, n, getattr(self, n).data_ptr())
        self._desc = d

    @staticmethod
    def storage_bytes(num_envs, n_steps, obs_shape, action_dim=1):
        """Bytes of the rollout's tensors (the [K] bootstrap batch and the minibatch outputs are extra)."""
        E, T = int(num_envs), int(n_steps)
        return T * E * (int(np.prod(obs_shape)) + 4 * int(action_dim) + 5 * 4 + 1) + E + 16

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _need(self, fn, name, t, dtypes, shape):
        dv = self.device
        if not isinstance(t, torch.Tensor) or t.device.type != dv.type or (dv.index is not None and t.device.index != dv.index):
            raise ValueError("%s: %s must be a tensor on %s" % (fn, name, dv))
        if t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor of shape %s" % (fn, name, " / ".join(str(d) for d in dtypes), list(shape)))

    # -- one step ----------------------------------------------------------------------------------------------
    def begin(self, obs, actions, values, logp):
        """Before the env step: stores the uint8 [E, *obs_shape] batch the policy acted on, its float32 actions [E, A] (or [E] with A = 1), values [E] and
        log-probabilities [E] in row t, and marks the envs whose previous step ended an episode.  Synchronises nothing."""
        E, A = self.num_envs, self.action_dim
        if self.t >= self.n_steps:
            raise ValueError("begin: the rollout is full (%d steps); call clear() after the update" % self.n_steps)
        if self._open:
            raise ValueError("begin: the previous begin has no end yet")
        self._need("begin", "obs", obs, (torch.uint8,), (E,) + self.obs_shape)
        self._need("begin", "actions", actions, (torch.float32,), (E,) if (A == 1 and isinstance(actions, torch.Tensor) and actions.dim() == 1) else (E, A))
        self._need("begin", "values", values, (torch.float32,), (E,))
        self._need("begin", "logp", logp, (torch.float32,), (E,))
        rc = self.L.bp_rollout_begin(C.byref(self._desc), self.t, _ptr(obs), _ptr(actions), _ptr(values), _ptr(logp), self._stream())
        _lib.check(self.L, None, rc, "bp_rollout_begin")
        self._open = True

    def truncated_rows(self, truncated, terminal_obs):
        """The fixed-size batch for V(terminal observation): (ids int32 [K], rows float32 [K, *obs_shape]) of the first K = bootstrap_rows envs, in ascending
        order, with truncated[e] != 0; rows are ``terminal_obs[e] / 255``; unused rows have id -1 and zeros.  More than K truncated envs count in
        ``hdr[0]``.  The two tensors are overwritten by the next call.  Synchronises nothing."""
        E = self.num_envs
        self._need("truncated_rows", "truncated", truncated, _U8, (E,))
        self._need("truncated_rows", "terminal_obs", terminal_obs, (torch.uint8,), (E,) + self.obs_shape)
        rc = self.L.bp_rollout_pick_rows(C.byref(self._desc), _ptr(truncated), _ptr(terminal_obs), self.bootstrap_rows, _ptr(self._boot_ids),
                                         _ptr(self._boot_rows), self._stream())
        _lib.check(self.L, None, rc, "bp_rollout_pick_rows")
        return self._boot_ids, self._boot_rows

    def end(self, reward, done, boot_ids=None, boot_values=None):
        """After the env step: stores float64 rewards [E] as float32, adds ``gamma * boot_values[k]`` to the reward of env ``boot_ids[k] >= 0`` (both
        [K'], any K' >= 1, or both None) and remembers `done` (uint8 / bool [E]) as the next row's episode starts.  Synchronises nothing."""
        E = self.num_envs
        if not self._open:
            raise ValueError("end: no begin awaits its end")
        self._need("end", "reward", reward, (torch.float64,), (E,))
        self._need("end", "done", done, _U8, (E,))
        K = 0
        if (boot_ids is None) != (boot_values is None):
            raise ValueError("end: boot_ids and boot_values come together")
        if boot_ids is not None:
            if not isinstance(boot_ids, torch.Tensor) or boot_ids.dim() != 1 or boot_ids.numel() < 1:
                raise ValueError("end: boot_ids must be an int32 tensor of shape [K], K >= 1")
            K = int(boot_ids.shape[0])
            self._need("end", "boot_ids", boot_ids, (torch.int32,), (K,))
            self._need("end", "boot_values", boot_values, (torch.float32,), (K,))
        rc = self.L.bp_rollout_end(C.byref(self._desc), self.t, _ptr(reward), _ptr(done), _ptr(boot_ids), _ptr(boot_values), K, self.gamma, self._stream())
        _lib.check(self.L, None, rc, "bp_rollout_end")
        self._open = False
        self.t += 1

    # -- the update ----------------------------------------------------------------------------------------------
    def _need_full(self, fn):
        if self.t < self.n_steps or self._open:
            raise ValueError("%s: the rollout holds %d of %d steps" % (fn, self.t, self.n_steps))

    def finish(self, last_values):
        """Advantages and returns of the full rollout from the float32 values [E] of the observation after the last step (GAE, float32, stable-baselines3's
        order of operations).  Synchronises nothing."""
        self._need_full("finish")
        self._need("finish", "last_values", last_values, (torch.float32,), (self.num_envs,))
        gl = float(np.float64(self.gamma) * np.float64(self.gae_lambda))
        _lib.check(self.L, None, self.L.bp_rollout_finish(C.byref(self._desc), _ptr(last_values), self.gamma, gl, self._stream()), "bp_rollout_finish")
        self._finished = True

    def minibatches(self, batch_size, epoch):
        """Generator over the ceil(N / B) minibatches of epoch `epoch`, N = n_steps * num_envs: RolloutBatch(obs float32 [B, *obs_shape] = u8 / 255, action
        float32 [B, A], value, logp, advantage, ret float32 [B], index int32 [B] = t * num_envs + e, valid uint8 [B]).  Every stored transition occurs
        exactly once per epoch; the samples past N of the last minibatch have valid 0 and zeros.  All minibatches are the same tensors, overwritten by the
        next one.  Synchronises nothing."""
        B = int(batch_size)
        if B < 1:
            raise ValueError("minibatches: batch_size must be at least 1")
        self._need_full("minibatches")
        if not self._finished:
            raise ValueError("minibatches: call finish() first")
        return self._minibatches(B, int(epoch))

    def _minibatches(self, B, epoch):
        N, A, dv = self.n_steps * self.num_envs, self.action_dim, self.device
        if self._batch is None or self._batch.valid.shape[0] != B:
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=dv)   # noqa: E731
            self._batch = RolloutBatch(obs=f(B, *self.obs_shape), action=f(B, A), value=f(B), logp=f(B), advantage=f(B), ret=f(B),
                                       index=torch.empty(B, dtype=torch.int32, device=dv), valid=torch.empty(B, dtype=torch.uint8, device=dv))
        out = self._batch
        b = _lib.BpRolloutBatch()
        for n in RolloutBatch._fields:
            setattr(b, n, getattr(out, n).data_ptr())
        for j in range((N + B - 1) // B):
            rc = self.L.bp_rollout_minibatch(C.byref(self._desc), C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), epoch, j, B, C.byref(b), self._stream())
            _lib.check(self.L, None, rc, "bp_rollout_minibatch")
            yield out

    def clear(self):
        """Starts the next rollout at step 0; ``last_done`` carries over, as the env goes on where it was."""
        if self._open:
            raise ValueError("clear: a begin awaits its end")
        self.t, self._finished = 0, False

    def reset_episode_starts(self):
        """After an ``env.reset()`` from outside: the next row starts an episode in every env."""
        self.last_done.fill_(1)

    # -- host reads ------------------------------------------------------------------------------------------------
    def stats(self):
        """Host summary (one device read): truncated rows left without a bootstrap, rows ever stored, steps of the current rollout."""
        h = self.hdr.tolist()
        return {"unbootstrapped": int(h[0]), "stored": int(h[1]), "steps": self.t}

    # -- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self):
        """All tensors (clones on the device), the step counter and the shapes."""
        if self._open:
            raise ValueError("state_dict: a begin awaits its end")
        sd = {n: getattr(self, n).clone() for n, _ in _TENSORS}
        sd.update(n_steps=self.n_steps, num_envs=self.num_envs, obs_shape=self.obs_shape, action_dim=self.action_dim, seed=self.seed, t=self.t,
                  finished=self._finished)
        return sd

    def load_state_dict(self, sd):
        """Takes the tensors of a ``state_dict()`` of a buffer with the same steps, envs, observation shape and action width."""
        if (int(sd["n_steps"]), int(sd["num_envs"]), tuple(sd["obs_shape"]), int(sd["action_dim"])) != \
                (self.n_steps, self.num_envs, self.obs_shape, self.action_dim):
            raise ValueError("load_state_dict: the buffer was saved with %s steps, %s envs, observations %s and %s action columns" %
                             (sd["n_steps"], sd["num_envs"], tuple(sd["obs_shape"]), sd["action_dim"]))
        for n, dt in _TENSORS:
            t = sd[n]
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != tuple(getattr(self, n).shape):
                raise ValueError("load_state_dict: %s has the wrong dtype or shape" % n)
        for n, _ in _TENSORS:
            getattr(self, n).copy_(sd[n])
        self.seed, self.t, self._open, self._finished = int(sd.get("seed", self.seed)), int(sd["t"]), False, bool(sd["finished"])
