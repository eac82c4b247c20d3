"""DeviceTransitionBuffer: the off-policy learner's half of the lock-step loop, on the device (bp_transitions_*; DESIGN.md "Transition buffer").

``BatchedVecEnv(to_numpy=False)`` hands out E device-resident transitions per step.  This class keeps the last ``buffer_size // num_envs`` steps of them
in a ring -- the observation batch the policy acted on, the next observation (the terminal observation of an env whose episode ended in the step, not
the observation its reset wrote), actions, rewards, done flags and whether the time limit caused the done -- and draws float batches with replacement,
one library call each and no host read:

    buf = DeviceTransitionBuffer(vec_env, buffer_size=15000, seed=0)
    obs = vec_env.reset()
    while ...:
        held.copy_(obs)                                               # the env rewrites `obs` in place
        obs, reward, done, infos = vec_env.step(actions)
        buf.add(held, obs, infos.terminal_rows, actions, reward, done, infos.truncated_mask)
        batch = buf.sample(128)                                       # TransitionBatch; batch.done is 0 where the time limit ended the episode

The rules are those of stable-baselines3's ReplayBuffer (``handle_timeout_termination``, sampling with replacement); the draw is the counter RNG of
``DeviceReplayBuffer`` (``bp_replay_index``) keyed by the seed and the number of draws so far.  ``size()`` and ``stats()`` are the only host reads.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .envs.batched import _ptr

__all__ = ["DeviceTransitionBuffer", "TransitionBatch"]

TransitionBatch = namedtuple("TransitionBatch", ("obs", "next_obs", "action", "reward", "done", "slot", "valid"))
_TENSORS = (("obs", torch.uint8), ("next_obs", torch.uint8), ("action", torch.float32), ("reward", torch.float32), ("done", torch.uint8),
            ("timeout", torch.uint8), ("hdr", torch.int64))
_U8 = (torch.uint8, torch.bool)


class DeviceTransitionBuffer:
    """A ring of T = max(1, buffer_size // num_envs) step rows (stable-baselines3's rule) of the `num_envs` envs of a batched env (or the BatchedVecEnv
    around it) with uint8 observations.  Tensors, all on the env's device: obs, next_obs uint8 [T, E, *obs_shape]; action float32 [T, E, A]; reward
    float32 [T, E]; done, timeout uint8 [T, E]; hdr int64 [2] = adds ever made, sample draws made.  Transition (s, e) of the s-th add lives in slot
    (s % T) * E + e."""

    def __init__(self, env, buffer_size, seed=0):
        env = env.env if hasattr(env, "step_wait") else env          # a BatchedVecEnv: the batched env inside
        if bool(getattr(getattr(env, "cfg", None), "low_dim_state", False)) or env.obs.dtype != torch.uint8:
            raise ValueError("DeviceTransitionBuffer: only uint8 image observations are supported (low_dim_state observations are not)")
        self.buffer_size, self.seed = int(buffer_size), int(seed)
        self.L, self.device = env.L, env.device
        self.num_envs, self.obs_shape = int(env.num_envs), tuple(env.obs_shape)
        self.action_dim = int(getattr(env, "action_dim", 1))
        self.row_bytes = int(np.prod(self.obs_shape))
        if self.buffer_size < 1:
            raise ValueError("DeviceTransitionBuffer: buffer_size must be at least 1")
        self.steps = max(1, self.buffer_size // self.num_envs)
        T, E, A = self.steps, self.num_envs, self.action_dim
        if T * E > 0x7FFFFFFF:
            raise ValueError("DeviceTransitionBuffer: steps * num_envs must be at most 2^31 - 1")
        if self.row_bytes % 16:
            raise ValueError("DeviceTransitionBuffer: observation rows of %s are %d bytes, not a multiple of 16" % (self.obs_shape, self.row_bytes))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)   # noqa: E731
        self.obs, self.next_obs = z((T, E) + self.obs_shape, torch.uint8), z((T, E) + self.obs_shape, torch.uint8)
        self.action, self.reward = z((T, E, A), torch.float32), z((T, E), torch.float32)
        self.done, self.timeout, self.hdr = z((T, E), torch.uint8), z((T, E), torch.uint8), z(2, torch.int64)
        self._batch = self._batch_desc = None
        d = _lib.BpTransitionsDesc()
        d.steps, d.num_envs, d.action_dim, d.row_bytes = T, E, A, self.row_bytes
        d.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        for n, _ in _TENSORS:
            setattr(d, n, getattr(self, n).data_ptr())
        self._desc = d

    @staticmethod
    def storage_bytes(num_envs, buffer_size, obs_shape, action_dim=1):
        """Bytes of the buffer's tensors (the sample outputs are extra)."""
        E = int(num_envs)
        T = max(1, int(buffer_size) // E)
        return T * E * (2 * int(np.prod(obs_shape)) + 4 * int(action_dim) + 4 + 2) + 16

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _need(self, fn, name, t, dtypes, shape):
        dv = self.device
        if not isinstance(t, torch.Tensor) or t.device.type != dv.type or (dv.index is not None and t.device.index != dv.index):
            raise ValueError("%s: %s must be a tensor on %s" % (fn, name, dv))
        if t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor of shape %s" % (fn, name, " / ".join(str(d) for d in dtypes), list(shape)))

    def add(self, obs, next_obs, terminal_obs, actions, reward, done, truncated):
        """One env step of all envs: `obs` the uint8 [E, *obs_shape] batch the policy acted on (a copy: the env rewrites its own), `next_obs` the batch
        the step returned, `terminal_obs` the rows ``LazyInfos.terminal_rows`` (read where ``done``), float32 actions [E, A] (or [E] with A = 1), float64
        rewards [E], `done` and `truncated` uint8 / bool [E].  Stores them in step row ``adds % T``; the arguments are consumed in stream order.
        Synchronises nothing."""
        E, A = self.num_envs, self.action_dim
        rows = (E,) + self.obs_shape
        self._need("add", "obs", obs, (torch.uint8,), rows)
        self._need("add", "next_obs", next_obs, (torch.uint8,), rows)
        self._need("add", "terminal_obs", terminal_obs, (torch.uint8,), rows)
        self._need("add", "actions", actions, (torch.float32,), (E,) if (A == 1 and isinstance(actions, torch.Tensor) and actions.dim() == 1) else (E, A))
        self._need("add", "reward", reward, (torch.float64,), (E,))
        self._need("add", "done", done, _U8, (E,))
        self._need("add", "truncated", truncated, _U8, (E,))
        rc = self.L.bp_transitions_add(C.byref(self._desc), _ptr(obs), _ptr(next_obs), _ptr(terminal_obs), _ptr(actions), _ptr(reward), _ptr(done),
                                       _ptr(truncated), self._stream())
        _lib.check(self.L, None, rc, "bp_transitions_add")

    def sample(self, batch_size):
        """TransitionBatch(obs, next_obs float32 [B, *obs_shape] = u8 / 255, action float32 [B, A], reward float32 [B], done float32 [B] = done * (1 -
        timeout), slot int32 [B], valid uint8 [B]) of B stored transitions drawn with replacement.  Before the first add every row is zeros with valid 0
        and slot -1.  Every call returns the same tensors, overwritten by the next one.  Synchronises nothing."""
        B = int(batch_size)
        if B < 1:
            raise ValueError("sample: batch_size must be at least 1")
        if self._batch is None or self._batch.valid.shape[0] != B:
            A, dv = self.action_dim, self.device
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=dv)   # noqa: E731
            self._batch = TransitionBatch(obs=f(B, *self.obs_shape), next_obs=f(B, *self.obs_shape), action=f(B, A), reward=f(B), done=f(B),
                                          slot=torch.empty(B, dtype=torch.int32, device=dv), valid=torch.empty(B, dtype=torch.uint8, device=dv))
            self._batch_desc = _lib.BpTransitionsBatch()
            for n in TransitionBatch._fields:
                setattr(self._batch_desc, n, getattr(self._batch, n).data_ptr())
        rc = self.L.bp_transitions_sample(C.byref(self._desc), C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), B, C.byref(self._batch_desc), self._stream())
        _lib.check(self.L, None, rc, "bp_transitions_sample")
        return self._batch

    # -- host reads ------------------------------------------------------------------------------------------------
    def size(self):
        """Stored transitions (one device read)."""
        return min(int(self.hdr[0]), self.steps) * self.num_envs

    def stats(self):
        """Host summary (one device read): adds ever made, sample draws made, stored transitions."""
        h = self.hdr.tolist()
        return {"adds": int(h[0]), "draws": int(h[1]), "size": min(int(h[0]), self.steps) * self.num_envs}

    # -- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self):
        """All tensors (clones on the device), the seed and the shapes."""
        sd = {n: getattr(self, n).clone() for n, _ in _TENSORS}
        sd.update(steps=self.steps, num_envs=self.num_envs, obs_shape=self.obs_shape, action_dim=self.action_dim, seed=self.seed)
        return sd

    def load_state_dict(self, sd):
        """Takes the tensors of a ``state_dict()`` of a buffer with the same steps, envs, observation shape and action width."""
        if (int(sd["steps"]), int(sd["num_envs"]), tuple(sd["obs_shape"]), int(sd["action_dim"])) != \
                (self.steps, self.num_envs, self.obs_shape, self.action_dim):
            raise ValueError("load_state_dict: the buffer was saved with %s steps, %s envs, observations %s and %s action columns" %
                             (sd["steps"], sd["num_envs"], tuple(sd["obs_shape"]), sd["action_dim"]))
        for n, dt in _TENSORS:
            t = sd[n]
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != tuple(getattr(self, n).shape):
                raise ValueError("load_state_dict: %s has the wrong dtype or shape" % n)
        for n, _ in _TENSORS:
            getattr(self, n).copy_(sd[n])
        self.seed = int(sd.get("seed", self.seed))
