"""box-delivery-v0 on MI355X: batched tensor environment + the reference-shaped single-env adapter.

Reference: benchpush/environments/box_delivery/box_delivery_env.py (BoxDeliveryEnv) with ``agent.action_type: 'heading'`` (what
its PPO/SAC baselines use, config.yaml:170): one step = PositionController waypoints + execute_robot_path (a variable number
of 2 ms sim steps under the DP controller) + step_simulation_until_still, rewards from spfa path-length deltas of every box,
boxes inside the receptacle are removed, observation uint8 [224, 224, 4] (channels last).

Episodes: the reference keeps one ``np.random.RandomState(cfg.misc.random_seed)`` per env and draws start pose / boxes at every
reset; here the same stream generates ``num_trials`` consecutive episodes once and env e plays episode
``(global_env_id + episode) % num_trials``.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..box_delivery_scenario import box_delivery_params, box_delivery_physics_params, generate_trials
from ..config import default_cfg, merge_user_cfg
from ..gym_shim import spaces
from ..scenario import poly_centroid
from .batched import _AdapterBase
from .ship_ice import BatchedShipIceEnv, _ptr

__all__ = ["BatchedBoxDeliveryEnv", "BoxDeliveryEnv", "AsyncQueue", "BD_INFO_KEYS"]
BD_INFO_KEYS = _lib.BD_INFO_KEYS


def _bd_cfg(cfg):
    c = merge_user_cfg(default_cfg("box_delivery"), cfg)
    if c.agent.action_type not in ("heading", "position", "velocity"):
        raise ValueError("agent.action_type must be heading, position or velocity")
    if c.teleop_mode:
        raise NotImplementedError("teleop mode (keyboard / pygame) is outside the accelerated path")
    return c


def _out_ptrs(v):
    """The five output pointers of the library's step calls, from an env's [E, ...] tensors or an AsyncQueue's [M, ...] ones."""
    return _ptr(v.obs), _ptr(v.reward), _ptr(v.terminated), _ptr(v.truncated), _ptr(v.info)


class BatchedBoxDeliveryEnv(BatchedShipIceEnv):
    """E independent box-delivery environments on one GPU: reset(mask) / step(actions) with device tensors."""

    render_task = "box_delivery"
    # what differs between the two tasks: BatchedAreaClearingEnv overrides these and _bd_config, and passes its base_seed as `seed`
    _task_cfg = staticmethod(_bd_cfg)
    _physics_params = staticmethod(box_delivery_physics_params)
    _task_params = staticmethod(box_delivery_params)
    _generate_trials = staticmethod(generate_trials)
    _same_box_count = True   # all trials must hold the same number of boxes

    def _bd_config(self):
        return _lib.make_bd_config(self.params, self.bd_params, self.cfg)

    def __init__(self, num_envs, cfg=None, trials=None, device="cuda:0", env_id_offset=0, num_trials=32, seed=None, bd_overrides=None):
        self._open(num_envs, device, env_id_offset)
        self.cfg = self._task_cfg(cfg)
        self.params = self._physics_params(self.cfg)
        self.bd_params = self._task_params(self.cfg)
        if bd_overrides:   # constants of the reference that are not in its config (e.g. STEP_LIMIT, box_delivery_env.py:62): tests shorten them
            self.bd_params.update(bd_overrides)
        if trials is None:
            trials = self._generate_trials(self.cfg, num_trials, seed)
        self.trials = trials
        self.nbox = nbox = len(trials[0]["boxes"])
        if self._same_box_count and any(len(t["boxes"]) != nbox for t in trials):
            raise ValueError("all trials must hold the same number of boxes")
        self.bd_params["num_boxes"] = nbox
        self._create(self.L.bp_bd_create, self._bd_config())
        self._load(trials)

    def _load(self, trials):
        """bp_bd_load with its arguments packed from the trial dicts, then the output tensors.  A refused load (BpError) leaves the handle as it was created,
        so it may be called again with other trials of the same box count."""
        self.trials, nbox = trials, self.nbox
        ns = max(len(t["statics"][1]) for t in trials)
        c = lambda a, dt: np.ascontiguousarray(a, dt)
        starts = c(np.stack([t["start"] for t in trials]), np.float64)
        boxes = c(np.stack([t["boxes"] for t in trials]), np.float64)
        def pad(a, fill=0):   # trials may hold different numbers of columns: unused slots have vertex count 0
            out = np.full((ns,) + a.shape[1:], fill, a.dtype)
            out[: len(a)] = a
            return out
        sv = c(np.stack([pad(t["statics"][0]) for t in trials]), np.float64)
        sc = c(np.stack([pad(t["statics"][1]) for t in trials]), np.int32)
        sp = c(np.stack([pad(t["statics"][2]) for t in trials]), np.float64)
        sr = c(np.stack([pad(t["statics"][3]) for t in trials]), np.float64)
        st = c(np.stack([pad(t["statics"][4], 3) for t in trials]), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.L, self.h, self.L.bp_bd_load(self.h, len(trials), nbox, p(starts), p(boxes), ns, p(sv), p(sc), p(sp), p(sr), p(st)), "bp_bd_load")
        lp = self.L.bp_obs_height(self.h)
        self.action_dim = 2 if self.cfg.agent.action_type == "velocity" else 1
        self._alloc_io((lp, lp, 4), self.action_dim)

    def step(self, actions):
        """actions: [E] heading in [-1, 1] / position index, or [E, 2] = (linear, angular) speed for 'velocity'."""
        self._actions.copy_(actions.reshape(-1).to(self.device), non_blocking=True)
        _lib.check(self.L, self.h, self.L.bp_step(self.h, _ptr(self._actions), *_out_ptrs(self), self._stream()), "bp_step")
        return self.obs, self.reward, self.terminated, self.truncated, self.info

    # -- asynchronous step (DESIGN.md "Asynchronous step") -------------------------------------------------
    ASYNC_BUDGET = 500    # default budget of step_async in sim steps: the best of the measured sweep 500 / 1000 / 2000 / 3000 at 4096 envs (profiles/async/README.md)

    def _async_io(self):
        if getattr(self, "_ready", None) is None:
            self._ready = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            self._slices = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        return self._ready, self._slices

    @property
    def slices(self):
        """int32 [E] on the device: how many step_async / drain calls the transition an env emitted last took."""
        return self._async_io()[1]

    @property
    def async_open(self):
        """True from a step_async until a drain() or a reset of all envs: envs may be in the middle of an env step (a host flag, no device read)."""
        return bool(self.L.bp_bd_async_open(self.h))

    def step_async(self, actions, budget=ASYNC_BUDGET):
        """Opt-in asynchronous step: every env is idle or busy (in the middle of an env step).  An idle env takes its row of `actions` (shaped as for step) and
        starts an env step, a busy env ignores its row and resumes; every env then runs at most `budget` >= 1 sim steps.  Returns (obs, reward, terminated,
        truncated, info, ready): ready is uint8 [E] on the device; an env with ready[e] = 1 finished its env step in this call, wrote its rows exactly as step()
        would have and is idle again (``slices[e]`` = calls the step took); the rows of every other env are untouched and its step goes on in the next call.
        The transitions an env emits do not depend on the budget or on the other envs: they are step()'s for the actions the env accepted, bit for bit.  What
        does depend on them is which envs emit: short env steps are sampled more often than long ones.  Nothing synchronises with the host.  While a slice is
        open step(), save_state, restore_state and clone_envs raise BpError; reset(mask) cancels the busy envs of the mask.  Raises BpError, with nothing
        launched, for budget < 1, actions of the wrong size and configs with sim.damping != 0."""
        budget = int(budget)
        if budget < 1:
            raise _lib.BpError("step_async failed: BP_EINVAL (-1) budget %d < 1 sim step" % budget)
        if not isinstance(actions, torch.Tensor) or actions.numel() != self._actions.numel() or actions.is_complex():
            raise _lib.BpError("step_async failed: BP_EINVAL (-1) actions must be a real tensor of %d elements" % self._actions.numel())
        ready, slices = self._async_io()   # (a config with sim.damping != 0 is refused by the library, before it launches anything)
        self._actions.copy_(actions.reshape(-1).to(self.device), non_blocking=True)
        _lib.check(self.L, self.h, self.L.bp_bd_step_async(self.h, _ptr(self._actions), budget, *_out_ptrs(self), _ptr(ready), _ptr(slices), self._stream()),
                   "bp_bd_step_async")
        return self.obs, self.reward, self.terminated, self.truncated, self.info, ready

    def drain(self):
        """Runs the busy envs, and only those, to the end of their env steps (no budget) and closes the slice; returns the six-tuple of step_async with `ready`
        marking the envs it finished.  Idle envs do nothing and emit nothing.  Afterwards step(), save_state, restore_state and clone_envs work again."""
        ready, slices = self._async_io()
        _lib.check(self.L, self.h, self.L.bp_bd_async_drain(self.h, *_out_ptrs(self), _ptr(ready), _ptr(slices), self._stream()), "bp_bd_async_drain")
        return self.obs, self.reward, self.terminated, self.truncated, self.info, ready

    def async_queue(self, batch_size, budget=None):
        """Opens a device-resident ready queue on the asynchronous step and returns it (``AsyncQueue``): ``recv()`` hands out exactly `batch_size` rows -- env
        ids and their transitions, densely packed -- and ``send(actions, ids)`` gives those envs their next actions; no call reads anything back.  The env
        must have been reset and have no open slice.  budget: sim steps per env and recv (None: the task's ASYNC_BUDGET).  Until the queue's close() or a
        reset() of all envs, step, step_async, drain, reset(mask), save_state, restore_state and clone_envs raise BpError."""
        return AsyncQueue(self, batch_size, self.ASYNC_BUDGET if budget is None else budget)

    def stragglers(self):
        """(env steps finished by the second pass of the two-pass step, env steps whose path / until-still loop ran into STEP_LIMIT), cumulative since load."""
        out = np.zeros(2, np.uint32)
        _lib.check(self.L, self.h, self.L.bp_bd_get_stragglers(self.h, out.ctypes.data_as(C.c_void_p)), "bp_bd_get_stragglers")
        return int(out[0]), int(out[1])

    def cycle_skips(self):
        """(exact recurrences found in execute_robot_path, sim steps they skipped), cumulative since load (bp_bd_get_cycle_skips)."""
        out = np.zeros(2, np.uint32)
        _lib.check(self.L, self.h, self.L.bp_bd_get_cycle_skips(self.h, out.ctypes.data_as(C.c_void_p)), "bp_bd_get_cycle_skips")
        return int(out[0]), int(out[1])

    def maps(self, trial=0):
        dims = np.zeros(6, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.L, self.h, self.L.bp_bd_get_maps(self.h, trial, p(dims), None, None, None, None, None), "bp_bd_get_maps")
        SH, SW = int(dims[2]), int(dims[3])
        out = dict(dims=dims, cspace=np.zeros((SH, SW), np.uint8), cspace_thin=np.zeros((SH, SW), np.uint8), edt=np.zeros((SH, SW, 2), np.uint16),
                   recept=np.zeros((SH, SW), np.float32), small_free=np.zeros((SH, SW), np.uint8))
        _lib.check(self.L, self.h, self.L.bp_bd_get_maps(self.h, trial, p(dims), p(out["cspace"]), p(out["cspace_thin"]), p(out["edt"]), p(out["recept"]),
                                                        p(out["small_free"])), "bp_bd_get_maps")
        return out

    def episode_boxes(self):
        """float64 [E, 24, 3] on the device: (area, cx, cy) of every box polygon as it stood after the env's last reset, zeros in unused slots -- the snapshot
        the episode metrics (``episode_metrics()``, ``episode_history()``, ``episode_lists()``: the reference's TaskDrivenMetric) take the boxes' goal
        distances and the spanning tree from."""
        out = torch.zeros((self.num_envs, _lib.BD_MAXBOX, 3), dtype=torch.float64, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_bd_get_episode_boxes(self.h, _ptr(out), self._stream()), "bp_bd_get_episode_boxes")
        return out

    def box_completed(self):
        """uint8 [E, 24] (host copy): info['box_completed_statuses'] of every env -- box k delivered (box-delivery) / cleared (area-clearing) after the last
        step; what the episode metrics count as completed."""
        out = np.zeros((self.num_envs, _lib.BD_MAXBOX), np.uint8)
        _lib.check(self.L, self.h, self.L.bp_bd_get_completed(self.h, out.ctypes.data_as(C.c_void_p)), "bp_bd_get_completed")
        return out

    def box_state(self):
        """(alive uint8 [E, 24], waypoints [E, 64, 3], number of waypoints [E]) of the last step (host copies).  While an asynchronous slice is open a
        busy env shows the waypoints of the env step it is in, and the alive flags from before that step."""
        alive = np.zeros((self.num_envs, _lib.BD_MAXBOX), np.uint8)
        wp = np.zeros((self.num_envs, _lib.BD_MAXWP, 3), np.float64)
        nwp = np.zeros(self.num_envs, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.L, self.h, self.L.bp_bd_get_state(self.h, p(alive), p(wp), p(nwp)), "bp_bd_get_state")
        return alive, wp, nwp


class AsyncQueue:
    """Fixed-size recv / send batches over the asynchronous step of a BatchedBoxDeliveryEnv / BatchedAreaClearingEnv (``env.async_queue(M)``; DESIGN.md
    "Asynchronous step").  The queue between the two lives on the device: a FIFO ring of env ids, filled by the envs that emit a transition (and by reset
    envs, as *fresh* rows), in the order (call, env id).  All outputs are device tensors allocated once at open and reused by every recv:

    ids int32 [M] (-1 beyond the count), obs uint8 [M, 224, 224, 4], reward float64 [M], terminated / truncated uint8 [M], info float64 [M, 16],
    slices int32 [M] (calls the transition took; 0 = fresh row: a reset observation with reward 0 and flags 0), emitted uint8 [E] (the slice call's ready
    mask), counts int32 [5] = rows delivered, ids still queued, busy envs, envs taken and not sent yet, rejected send rows so far."""

    def __init__(self, env, batch_size, budget):
        self.env, self.batch_size, self.budget = env, int(batch_size), int(budget)
        if self.budget < 1:
            raise _lib.BpError("async_queue failed: BP_EINVAL (-1) budget %d < 1 sim step" % self.budget)
        _lib.check(env.L, env.h, env.L.bp_bd_queue_open(env.h, self.batch_size, env._stream()), "bp_bd_queue_open")
        M, dv = self.batch_size, env.device
        env._async_io()
        self.ids = torch.full((M,), -1, dtype=torch.int32, device=dv)
        self.obs = torch.zeros((M,) + tuple(env.obs_shape), dtype=torch.uint8, device=dv)
        self.reward = torch.zeros(M, dtype=torch.float64, device=dv)
        self.terminated = torch.zeros(M, dtype=torch.uint8, device=dv)
        self.truncated = torch.zeros(M, dtype=torch.uint8, device=dv)
        self.info = torch.zeros((M, _lib.INFO_COUNT), dtype=torch.float64, device=dv)
        self.slices = torch.zeros(M, dtype=torch.int32, device=dv)
        self.emitted = torch.zeros(env.num_envs, dtype=torch.uint8, device=dv)
        self.counts = torch.zeros(5, dtype=torch.int32, device=dv)
        self._counts_sum = torch.zeros(5, dtype=torch.int64, device=dv)   # running sums for stats()
        self._actions = torch.zeros(M * env.action_dim, dtype=torch.float64, device=dv)
        self._calls = 0

    @property
    def is_open(self):
        """True until close() or a reset() of all envs (a host flag, no device read)."""
        return bool(self.env.h) and int(self.env.L.bp_bd_queue_batch(self.env.h)) > 0

    def _recv_once(self, flags):
        v = self.env
        _lib.check(v.L, v.h, v.L.bp_bd_queue_recv(v.h, self.budget, flags, *_out_ptrs(v), _ptr(self.emitted), _ptr(v._slices), _ptr(self.ids),
                                                  *_out_ptrs(self), _ptr(self.slices), _ptr(self.counts), v._stream()), "bp_bd_queue_recv")
        self._calls += 1
        self._counts_sum += self.counts

    def recv(self, block=False):
        """One slice call of `budget` sim steps per env, then up to M queued rows: returns (ids, obs, reward, terminated, truncated, info), the queue's own
        [M, ...] tensors (overwritten by the next recv); ``slices``, ``emitted`` and ``counts`` are attributes.  block=False is one library call and
        synchronises nothing: the batch may be partly filled (ids -1, zero rows).  block=True repeats the call until it delivers a full batch or no env is
        busy any more, taking nothing in between; it reads the 5-int ``counts`` once per iteration, and that is its only host read."""
        if not block:
            self._recv_once(0)
        else:
            while True:
                self._recv_once(_lib.QUEUE_FULL_ONLY)
                c = self.counts.tolist()
                if c[0] > 0 or c[2] == 0:
                    break
        return self.ids, self.obs, self.reward, self.terminated, self.truncated, self.info

    def send(self, actions, ids, reset=None):
        """actions [M] (or [M, 2] for velocity actions), ids int32 [M] as a recv returned them, reset uint8 / bool [M] or None: row j hands env ids[j] its
        next action, or -- reset[j] != 0 -- resets it (next trial, as reset(mask)) and queues its reset observation as a fresh row.  Rows with id -1 are
        ignored; a row whose env is not awaiting a send, or that a smaller row of the same send already named, is ignored and counted (``counts[4]``).
        Raises ValueError, before anything is launched, for tensors of the wrong shape, dtype or device.  Synchronises nothing."""
        v, M = self.env, self.batch_size
        for name, t in (("actions", actions), ("ids", ids)) + ((("reset", reset),) if reset is not None else ()):
            if not isinstance(t, torch.Tensor) or t.device.type != v.device.type or (v.device.index is not None and t.device.index != v.device.index):
                raise ValueError("send: %s must be a tensor on %s" % (name, v.device))
        if not actions.is_floating_point() or actions.numel() != M * v.action_dim:
            raise ValueError("send: actions must be a floating-point tensor of %d elements" % (M * v.action_dim))
        if ids.dtype != torch.int32 or tuple(ids.shape) != (M,):
            raise ValueError("send: ids must be an int32 tensor of shape [%d]" % M)
        if reset is not None:
            if reset.dtype not in (torch.uint8, torch.bool) or tuple(reset.shape) != (M,):
                raise ValueError("send: reset must be a uint8 or bool tensor of shape [%d]" % M)
            reset = reset.contiguous().view(torch.uint8)
        self._actions.copy_(actions.reshape(-1), non_blocking=True)
        _lib.check(v.L, v.h, v.L.bp_bd_queue_send(v.h, _ptr(self._actions), _ptr(ids.contiguous()), _ptr(reset), _ptr(v.obs), _ptr(v.info), v._stream()),
                   "bp_bd_queue_send")

    def close(self):
        """Runs the busy envs to the end of their env steps (the drain), discards the queue and closes the slice; returns drain()'s six-tuple on the env's
        [E] rows.  Afterwards every env is idle and step(), save_state and the rest work again."""
        v = self.env
        ready, slices = v._async_io()
        _lib.check(v.L, v.h, v.L.bp_bd_queue_close(v.h, *_out_ptrs(v), _ptr(ready), _ptr(slices), v._stream()), "bp_bd_queue_close")
        return v.obs, v.reward, v.terminated, v.truncated, v.info, ready

    def stats(self):
        """Host summary (one device read): recv calls, rows delivered, mean fill of the batch, rejected send rows."""
        s = self._counts_sum.tolist()
        rejected = int(self.counts[4].item()) if self._calls else 0
        return {"calls": self._calls, "rows": int(s[0]), "mean_fill": (s[0] / (self._calls * self.batch_size)) if self._calls else 0.0, "rejected": rejected}


def low_dim_observation(polys):
    """generate_observation_low_dim (box_delivery_env.py:1025-1037, area_clearing.py:908-919): |centroid| of each polygon, flattened."""
    out = np.zeros(len(polys) * 2)
    for i, p in enumerate(polys):
        out[2 * i: 2 * i + 2] = poly_centroid(p)
    return out


class BoxDeliveryEnv(_AdapterBase):
    """Reference-shaped single environment (E = 1): reset()/step() returns and info keys of box_delivery_env.py:578-830."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}

    def __init__(self, cfg=None, trials=None, device="cuda:0", num_trials=32):
        super().__init__()
        self._b = BatchedBoxDeliveryEnv(1, cfg=cfg, trials=trials, device=device, num_trials=num_trials)
        self.cfg = self._b.cfg
        from ..obs_log import refuse_render_log_obs
        refuse_render_log_obs(self.cfg, "box-delivery-v0")
        self.num_boxes = self._b.nbox
        lp = self._b.obs_shape[0]
        if self.cfg.agent.action_type == "velocity":     # box_delivery_env.py:157-162
            self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype=np.float32)
        elif self.cfg.agent.action_type == "heading":
            self.action_space = spaces.Box(low=-1, high=1, shape=(1,), dtype=np.float32)
        else:
            self.action_space = spaces.Box(low=0, high=lp * lp, dtype=np.float32)
        self.observation_shape = self._b.obs_shape
        self.low_dim_state = self.cfg.low_dim_state
        if self.low_dim_state:                            # box_delivery_env.py:166-169
            self.fixed_trial_idx = self.cfg.fixed_trial_idx
            self.observation_space = spaces.Box(low=-10, high=30, shape=(self.num_boxes * 2,), dtype=np.float32)
        else:
            self.observation_space = spaces.Box(low=0, high=255, shape=self.observation_shape, dtype=np.uint8)
        self.episode_idx = None
        self.t = 0
        self.box_clearance_statuses = [False] * self.num_boxes
        self.receptacle_position = (self._b.bd_params["recept_x"], self._b.bd_params["recept_y"])
        self.goal_points = [self.receptacle_position]

    def _boxes(self):
        verts, cnt = self._b.world_polys()
        alive, _, _ = self._b.box_state()
        verts, cnt = verts[0].cpu().numpy(), cnt[0].cpu().numpy()
        return [verts[6 + k, : cnt[6 + k]].copy() for k in range(self.num_boxes) if alive[0, k]], alive[0, : self.num_boxes]

    def _info(self, it, boxes, alive):
        self.box_clearance_statuses = [not bool(a) for a in alive]
        return {"state": self._state3(it), "cumulative_distance": float(it[3]),
                "cumulative_boxes": int(it[4]), "cumulative_reward": float(it[5]), "total_work": float(it[6]), "obs": boxes,
                "box_completed_statuses": self.box_clearance_statuses, "goal_positions": self.goal_points, "ministeps": float(it[7]),
                "inactivity": int(it[8])}

    def reset(self, seed=None, options=None):
        self._begin_episode()
        boxes, alive = self._boxes()
        # low_dim_state: reset() returns <|centroid| of every box> (box_delivery_env.py:606-607,1025-1037); step() always returns the
        # image observation (box_delivery_env.py:807)
        obs = low_dim_observation(boxes) if self.low_dim_state else self._b.obs[0].cpu().numpy()
        return obs, self._info(self._b.info[0].cpu().numpy(), boxes, alive)

    def step(self, action):
        self.t += 1
        a = torch.tensor(np.asarray(action, dtype=np.float64).reshape(-1)[: self._b.action_dim], dtype=torch.float64)
        self._b.step(a)
        boxes, alive = self._boxes()
        info = self._info(self._b.info[0].cpu().numpy(), boxes, alive)
        return (self._b.obs[0].cpu().numpy(), float(self._b.reward[0].item()), bool(self._b.terminated[0].item()),
                bool(self._b.truncated[0].item()), info)

    _STATE_FIELDS = ("t", "episode_idx", "box_clearance_statuses")

    def render(self, mode="human", close=False):
        """rgb_array: the frame of this env with the controller's current waypoints as the path (numpy [H, W, 3]; benchpush_amd/render.py).
        human: no window and no snapshot (the reference's save branch is disabled, box_delivery_env.py:1275): warns once, returns None."""
        from ..render import adapter_render
        _, wp, nwp = self._b.box_state()
        return adapter_render(self, mode, wp[0, : int(nwp[0]), :2], None)
