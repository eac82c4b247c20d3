"""DeviceReplayBuffer: the learner's half of the ready-queue loop, on the device (bp_replay_*; DESIGN.md "Replay buffer").

The queue of ``env.async_queue(M)`` delivers dense [M, ...] rows with a data-dependent number of valid ones; the state of a transition is the row the
*same env* delivered some recvs earlier.  This class pairs them, stores (state, action, reward, ministeps, next_state) in a ring of `capacity`
transitions and samples float batches from it, with three library calls and no host read:

    buf = DeviceReplayBuffer(env, capacity)
    q = env.async_queue(M)
    ids, obs, reward, terminated, truncated, info = buf.recv(q)          # q.recv() + observe
    buf.send(q, actions, ids, reset=terminated.bool() | truncated.bool())   # record + q.send()
    batch = buf.sample(32)                                               # namedtuple of device tensors

Deviations from the reference's ReplayBuffer (SAM/policy.py): sampling is *with* replacement (without would need the number of stored transitions on
the host); a transition whose step terminated has ``nonfinal == 0`` and a stored next_state that is not used.  Only position actions are supported.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from .envs.ship_ice import _ptr

__all__ = ["DeviceReplayBuffer", "ReplayBatch"]

ReplayBatch = namedtuple("ReplayBatch", ("state", "action", "reward", "ministeps", "next_state", "nonfinal", "slot", "valid"))
_RING = (("state", torch.uint8), ("next_state", torch.uint8), ("action", torch.int32), ("reward", torch.float32), ("ministeps", torch.float32),
         ("nonfinal", torch.uint8), ("env", torch.int32))
_PEND = (("pend_obs", torch.uint8), ("pend_action", torch.int32), ("pend_flags", torch.uint8))


def _ministeps_col(env):
    from .envs.area_clearing import AC_INFO_KEYS, BatchedAreaClearingEnv
    keys = AC_INFO_KEYS if isinstance(env, BatchedAreaClearingEnv) else _lib.BD_INFO_KEYS
    return keys.index("ministeps")


class DeviceReplayBuffer:
    """Ring of `capacity` transitions of a BatchedBoxDeliveryEnv / BatchedAreaClearingEnv with position actions.  Tensors (all on the env's device):
    state, next_state uint8 [C, P, P, 4]; action int32 [C]; reward, ministeps float32 [C]; nonfinal uint8 [C]; env int32 [C]; pend_obs uint8 [E, P, P, 4];
    pend_action int32 [E]; pend_flags uint8 [E] (bit 0 an observation is held, bit 1 an action is recorded, bit 2 the env awaits a record);
    hdr int64 [4] = transitions ever stored, sample draws made, transition rows dropped for want of a pending state or action, rejected record rows.
    ``size()`` and ``stats()`` are the only host reads."""

    def __init__(self, env, capacity, seed=0):
        if env.cfg.agent.action_type != "position" or env.action_dim != 1:
            raise ValueError("DeviceReplayBuffer: only position actions are supported (agent.action_type is %r)" % env.cfg.agent.action_type)
        self.capacity, self.seed = int(capacity), int(seed)
        if self.capacity < 1 or self.capacity > 0x7FFFFFFF:
            raise ValueError("DeviceReplayBuffer: capacity must be 1 .. 2^31 - 1")
        self.L, self.device = env.L, env.device
        self.num_envs, self.obs_shape = int(env.num_envs), tuple(env.obs_shape)
        self.ministeps_col = _ministeps_col(env)
        P = self.obs_shape[0]
        self.row_bytes = P * P * 4
        if self.obs_shape != (P, P, 4) or self.row_bytes % 16:
            raise ValueError("DeviceReplayBuffer: observation rows of %s are not [P, P, 4] with P * P * 4 a multiple of 16" % (self.obs_shape,))
        C_, E, dv = self.capacity, self.num_envs, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dv)   # noqa: E731
        self.state, self.next_state = z((C_,) + self.obs_shape, torch.uint8), z((C_,) + self.obs_shape, torch.uint8)
        self.action, self.reward, self.ministeps = z(C_, torch.int32), z(C_, torch.float32), z(C_, torch.float32)
        self.nonfinal, self.env = z(C_, torch.uint8), z(C_, torch.int32)
        self.pend_obs, self.pend_action, self.pend_flags = z((E,) + self.obs_shape, torch.uint8), z(E, torch.int32), z(E, torch.uint8)
        self.hdr = z(4, torch.int64)
        self._win = z(E, torch.int32)
        self._row_slot = None
        self._actions = None
        self._desc = None
        self._ensure_rows(1)

    def _ensure_rows(self, M):
        if self._row_slot is None or self._row_slot.numel() < M:
            self._row_slot = torch.zeros(M, dtype=torch.int32, device=self.device)
            self._actions = torch.zeros(M, dtype=torch.float64, device=self.device)
            d = _lib.BpReplayDesc()
            d.capacity, d.num_envs, d.action_dim, d.row_bytes, d.max_rows = self.capacity, self.num_envs, 1, self.row_bytes, M
            d.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
            for n, _ in _RING + _PEND:
                setattr(d, n, getattr(self, n).data_ptr())
            d.hdr, d.row_slot, d.win = self.hdr.data_ptr(), self._row_slot.data_ptr(), self._win.data_ptr()
            self._desc = d

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _need(self, fn, name, t, dtypes, shape):
        dv = self.device
        if not isinstance(t, torch.Tensor) or t.device.type != dv.type or (dv.index is not None and t.device.index != dv.index):
            raise ValueError("%s: %s must be a tensor on %s" % (fn, name, dv))
        if t.dtype not in dtypes or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor of shape %s" % (fn, name, " / ".join(str(d) for d in dtypes), list(shape)))

    # -- the two bookkeeping calls ---------------------------------------------------------------------------
    def observe(self, q):
        """Stores the transitions of the rows the queue's last recv delivered (``q.ids``, ``q.obs``, ...) and makes every delivered observation its env's
        pending one.  Synchronises nothing."""
        return self.observe_rows(q.ids, q.obs, q.reward, q.terminated, q.truncated, q.info, q.slices)

    def observe_rows(self, ids, obs, reward, terminated, truncated, info, slices):
        """``observe`` on explicit [M, ...] tensors shaped as an AsyncQueue's outputs; the ids >= 0 of one call must be distinct, as the queue's are."""
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.numel() < 1:
            raise ValueError("observe: ids must be an int32 tensor of shape [M], M >= 1")
        M = int(ids.shape[0])
        u8 = (torch.uint8, torch.bool)
        for name, t, dts, shape in (("ids", ids, (torch.int32,), (M,)), ("obs", obs, (torch.uint8,), (M,) + self.obs_shape),
                                    ("reward", reward, (torch.float64,), (M,)), ("terminated", terminated, u8, (M,)),
                                    ("truncated", truncated, u8, (M,)), ("info", info, (torch.float64,), (M, _lib.INFO_COUNT)),
                                    ("slices", slices, (torch.int32,), (M,))):
            self._need("observe", name, t, dts, shape)
        self._ensure_rows(M)
        rc = self.L.bp_replay_observe(C.byref(self._desc), _ptr(ids), _ptr(obs), _ptr(reward), _ptr(terminated), _ptr(truncated), _ptr(info),
                                      _ptr(slices), M, self.ministeps_col, self._stream())
        _lib.check(self.L, None, rc, "bp_replay_observe")

    def record(self, actions, ids, reset=None):
        """Notes what is passed to ``AsyncQueue.send``: actions [M] (any real dtype; position indices), ids int32 [M], reset uint8 / bool [M] or None.
        A row is accepted if its env awaits a record and no smaller row names it; an accepted reset row makes the env forget its pending observation.
        Raises ValueError, before anything is launched, for tensors of the wrong shape, dtype or device.  Synchronises nothing."""
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.numel() < 1:
            raise ValueError("record: ids must be an int32 tensor of shape [M], M >= 1")
        M = int(ids.shape[0])
        self._need("record", "ids", ids, (torch.int32,), (M,))
        if not isinstance(actions, torch.Tensor) or actions.is_complex() or actions.numel() != M:
            raise ValueError("record: actions must be a real tensor of %d elements (position actions)" % M)
        self._need("record", "actions", actions, (actions.dtype,), tuple(actions.shape))
        if reset is not None:
            self._need("record", "reset", reset, (torch.uint8, torch.bool), (M,))
            reset = reset.view(torch.uint8)
        self._ensure_rows(M)
        a = self._actions[:M]
        a.copy_(actions.reshape(-1), non_blocking=True)
        _lib.check(self.L, None, self.L.bp_replay_record(C.byref(self._desc), _ptr(a), _ptr(ids), _ptr(reset), M, self._stream()), "bp_replay_record")

    # -- the queue's calls with the bookkeeping attached --------------------------------------------------------
    def recv(self, q, block=False):
        """``q.recv(block)`` followed by ``observe(q)``; returns the queue's six tensors."""
        out = q.recv(block)
        self.observe(q)
        return out

    def send(self, q, actions, ids, reset=None):
        """``record(actions, ids, reset)`` followed by ``q.send(actions, ids, reset)``.  Both apply the same winner rule, so a row the queue accepts is a
        row the buffer accepts as long as every recv went through ``recv`` above."""
        self.record(actions, ids, reset)
        q.send(actions.to(torch.float64) if not actions.is_floating_point() else actions, ids, reset)

    # -- sampling ------------------------------------------------------------------------------------------------
    def sample(self, batch_size, out=None):
        """Draws `batch_size` stored transitions with replacement: ReplayBatch(state f32 [B, 4, P, P], action i64 [B], reward f32 [B], ministeps f32 [B],
        next_state f32 [B, 4, P, P], nonfinal u8 [B], slot i32 [B], valid u8 [B]); the images are ``u8 / 255`` channel first, what ToTensor() gives.
        With nothing stored yet every output is zero and ``valid`` is 0 -- multiply the loss by it.  out: a ReplayBatch of a previous call with the same
        batch size, to be overwritten.  Synchronises nothing."""
        B = int(batch_size)
        if B < 1:
            raise ValueError("sample: batch_size must be at least 1")
        P, dv = self.obs_shape[0], self.device
        shapes = dict(state=((B, 4, P, P), torch.float32), next_state=((B, 4, P, P), torch.float32), action=((B,), torch.int64),
                      reward=((B,), torch.float32), ministeps=((B,), torch.float32), nonfinal=((B,), torch.uint8), slot=((B,), torch.int32),
                      valid=((B,), torch.uint8))
        if out is None:
            out = ReplayBatch(**{n: torch.empty(s, dtype=dt, device=dv) for n, (s, dt) in shapes.items()})
        else:
            for n, (s, dt) in shapes.items():
                self._need("sample", "out." + n, getattr(out, n), (dt,), s)
        b = _lib.BpReplayBatch()
        for n in shapes:
            setattr(b, n, getattr(out, n).data_ptr())
        rc = self.L.bp_replay_sample(C.byref(self._desc), B, C.c_uint64(self.seed & 0xFFFFFFFFFFFFFFFF), C.byref(b), self._stream())
        _lib.check(self.L, None, rc, "bp_replay_sample")
        return out

    # -- host reads ------------------------------------------------------------------------------------------------
    def size(self):
        """Transitions available to ``sample`` (one device read)."""
        return min(int(self.hdr[0].item()), self.capacity)

    def stats(self):
        """Host summary (one device read): transitions ever stored, sample draws, dropped transition rows, rejected record rows."""
        h = self.hdr.tolist()
        return {"stored": int(h[0]), "size": min(int(h[0]), self.capacity), "draws": int(h[1]), "dropped": int(h[2]), "rejected": int(h[3])}

    # -- checkpoints ---------------------------------------------------------------------------------------------
    def state_dict(self):
        """All tensors and ``hdr`` (clones on the device), plus capacity, num_envs, obs_shape and seed."""
        sd = {n: getattr(self, n).clone() for n, _ in _RING + _PEND}
        sd["hdr"] = self.hdr.clone()
        sd.update(capacity=self.capacity, num_envs=self.num_envs, obs_shape=self.obs_shape, seed=self.seed)
        return sd

    def load_state_dict(self, sd):
        """Takes the tensors of a ``state_dict()`` of a buffer with the same capacity, envs and observation shape.  Bits 1 and 2 of every env are cleared:
        the queue the actions were sent to is gone, so the first transition row of each env after a reload is counted as dropped (``hdr[2]``) instead of
        being paired with a stale action."""
        if (int(sd["capacity"]), int(sd["num_envs"]), tuple(sd["obs_shape"])) != (self.capacity, self.num_envs, self.obs_shape):
            raise ValueError("load_state_dict: the buffer was saved with capacity %s, %s envs and observations %s" %
                             (sd["capacity"], sd["num_envs"], tuple(sd["obs_shape"])))
        for n, dt in _RING + _PEND + (("hdr", torch.int64),):
            t = sd[n]
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != tuple(getattr(self, n).shape):
                raise ValueError("load_state_dict: %s has the wrong dtype or shape" % n)
        for n, _ in _RING + _PEND + (("hdr", torch.int64),):
            getattr(self, n).copy_(sd[n])
        self.pend_flags.bitwise_and_(1)
        self.seed = int(sd.get("seed", self.seed))
