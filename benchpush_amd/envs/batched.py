"""What every environment of this package shares: ``_BatchedBase``, the tensor-in / tensor-out wrapper of one bp_handle that the four batched
environments derive from; ``need``, the check of a tensor argument; ``_AdapterBase``, the common part of the reference-shaped single-env classes.

PyTorch is used only for device memory and streams; all compute is in libbenchpush_hip.so (C ABI).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..gym_shim import Env


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def need(fn, t, name, dtypes, shapes, device):
    """Raises ValueError unless `t` is a contiguous tensor on `device` of one of `dtypes` (a dtype or a tuple of them) whose shape matches `shapes`: one
    shape or a list of alternatives, None standing for any size."""
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    shapes = shapes if isinstance(shapes, list) else [shapes]
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != device or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor on %s" % (fn, name, " / ".join(map(str, dtypes)), device))
    if not any(len(sh) == t.dim() and all(a is None or a == b for a, b in zip(sh, t.shape)) for sh in shapes):
        raise ValueError("%s: %s has shape %s, expected %s" % (fn, name, tuple(t.shape), " or ".join(str(list(sh)) for sh in shapes)))


class _BatchedBase:
    """Tensor-in / tensor-out wrapper of one bp_handle (shared by all four environments)."""

    # -- the handle ----------------------------------------------------------------------------------------
    def _open(self, num_envs, device, env_id_offset=0):
        """First thing in a constructor, before anything is generated: no GPU or no library is an error of its own."""
        if not torch.cuda.is_available():
            raise _lib.BpError("%s needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback" % type(self).__name__)
        self.L = _lib.load()
        self.num_envs = int(num_envs)
        self.env_id_offset = int(env_id_offset)
        self.device = torch.device(device)

    def _create(self, create, bcfg):
        """The handle, from `create` (bp_create or bp_bd_create) and its config struct."""
        self.h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.L, None, create(C.byref(bcfg), self.num_envs, self.env_id_offset, dev_index, C.byref(self.h)), create.__name__)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "h", None):
            self.L.bp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _alloc_io(self, obs_shape=None, action_dim=1):
        self.nb_cap = self.L.bp_nb_cap(self.h)
        self.obs_shape = obs_shape or (4, self.L.bp_obs_height(self.h), self.L.bp_obs_width(self.h))
        E, dv = self.num_envs, self.device
        self.obs = torch.zeros((E,) + self.obs_shape, dtype=torch.uint8, device=dv)
        self.reward = torch.zeros(E, dtype=torch.float64, device=dv)
        self.terminated = torch.zeros(E, dtype=torch.uint8, device=dv)
        self.truncated = torch.zeros(E, dtype=torch.uint8, device=dv)
        self.info = torch.zeros((E, _lib.INFO_COUNT), dtype=torch.float64, device=dv)
        self._actions = torch.zeros(E * action_dim, dtype=torch.float64, device=dv)

    def _need(self, fn):
        """``need`` for the arguments of the method `fn` of this env: need(t, name, dtypes, shapes)."""
        return lambda t, name, dtypes, shapes: need(fn, t, name, dtypes, shapes, self.device)

    def _mask(self, mask):
        return None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()

    def _env_ids(self, env_ids):
        if env_ids is None:
            return torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        return torch.as_tensor(env_ids).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()

    # -- API -----------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        """Reset the envs selected by ``mask`` (uint8/bool tensor [E]; None = all). Returns (obs, info) views."""
        _lib.check(self.L, self.h, self.L.bp_reset(self.h, _ptr(self._mask(mask)), _ptr(self.obs), _ptr(self.info), self._stream()), "bp_reset")
        return self.obs, self.info

    def step(self, actions):
        """actions: tensor [E] in [-1, 1] (any float dtype).  Returns (obs, reward, terminated, truncated, info)."""
        self._actions.copy_(actions.reshape(-1).to(self.device), non_blocking=True)
        _lib.check(self.L, self.h, self.L.bp_step(self.h, _ptr(self._actions), _ptr(self.obs), _ptr(self.reward),
                                                 _ptr(self.terminated), _ptr(self.truncated), _ptr(self.info),
                                                 self._stream()), "bp_step")
        return self.obs, self.reward, self.terminated, self.truncated, self.info

    def step_physics(self, actions):
        self._actions.copy_(actions.reshape(-1).to(self.device), non_blocking=True)
        _lib.check(self.L, self.h, self.L.bp_step_physics(self.h, _ptr(self._actions), _ptr(self.reward), _ptr(self.terminated),
                                                         _ptr(self.truncated), _ptr(self.info), self._stream()), "bp_step_physics")
        return self.reward, self.terminated, self.truncated, self.info

    def observe(self, mask=None):
        _lib.check(self.L, self.h, self.L.bp_observe(self.h, _ptr(self._mask(mask)), _ptr(self.obs), self._stream()), "bp_observe")
        return self.obs

    def world_polys(self):
        """info['obs'] for every env: (verts [E, nb_cap, 20, 2] f64, counts [E, nb_cap] i32); index 0 is the ship.  (Box-delivery / area-clearing with an
        asynchronous slice open: a busy env is shown in the middle of its env step.)"""
        out = torch.zeros((self.num_envs, self.nb_cap, _lib.MAXV, 2), dtype=torch.float64, device=self.device)
        cnt = torch.zeros((self.num_envs, self.nb_cap), dtype=torch.int32, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_get_world_polys(self.h, _ptr(out), _ptr(cnt), self._stream()), "bp_get_world_polys")
        return out, cnt

    def body_state(self):
        out = torch.zeros((self.num_envs, self.nb_cap, 9), dtype=torch.float64, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_get_body_state(self.h, _ptr(out), self._stream()), "bp_get_body_state")
        return out

    def low_dim_obs(self):
        out = torch.zeros((self.num_envs, self.nb_cap - 1, 2), dtype=torch.float64, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_get_low_dim_obs(self.h, _ptr(out), self._stream()), "bp_get_low_dim_obs")
        return out

    # -- saving, restoring and forking (include/benchpush_amd.h: state records) ---------------------------
    _OUT_ROWS = ("obs", "reward", "terminated", "truncated", "info")

    def state_bytes(self):
        """Bytes of one state record of this handle."""
        n = int(self.L.bp_state_bytes(self.h))
        _lib.check(self.L, self.h, min(n, 0), "bp_state_bytes")
        return n

    def state_layout_id(self):
        """The handle's layout id: records are exchanged between handles with equal ids (same configuration, same trials; any number of envs)."""
        return int(self.L.bp_state_layout_id(self.h))

    def save_state(self, env_ids=None):
        """The complete state of the envs `env_ids` (None: all) between two steps as an ``EnvState`` on the device: one record per env, written by one
        kernel launch, plus the envs' rows of obs / reward / terminated / truncated / info.  Raises BpError before the first reset or for an id outside
        the batch.  Synchronises the stream once (the ids are checked on the host)."""
        from ..state import EnvState
        ids = self._env_ids(env_ids)
        k = int(ids.numel())
        rec = torch.empty((k, self.state_bytes()), dtype=torch.uint8, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_save_state(self.h, _ptr(ids), k, _ptr(rec), self._stream()), "bp_save_state")
        idx = ids.long()   # (indexed only after the library has accepted the ids)
        return EnvState(rec, *[getattr(self, n)[idx] for n in self._OUT_ROWS], self.state_layout_id(), ids.clone())

    def restore_state(self, state, env_ids=None, trusted=False):
        """Put the saved envs of `state` into the envs `env_ids` (None: the envs they were saved from) -- of this handle or of any handle created with the
        same configuration and trials.  The envs continue bit for bit as the saved ones would have; their rows of obs / reward / terminated / truncated /
        info are put back as well.  Raises BpError, with no env touched, for an id outside the batch, a repeated id or records of another layout.
        trusted=True skips those checks and the host synchronisation they need."""
        ids = self._env_ids(state.env_ids if env_ids is None else env_ids)
        k = int(ids.numel())
        if k != len(state):
            raise ValueError("restore_state: %d env ids for %d saved envs" % (k, len(state)))
        if state.device != self.device:
            state = state.to(self.device)
        rec = state.records.contiguous()
        if rec.dtype != torch.uint8 or rec.dim() != 2 or rec.shape[1] != self.state_bytes():
            raise _lib.BpError("restore_state failed: BP_EINVAL (-1) records of %s bytes, this handle's are %d" % (tuple(rec.shape[1:]), self.state_bytes()))
        _lib.check(self.L, self.h, self.L.bp_load_state(self.h, _ptr(ids), k, _ptr(rec), _lib.STATE_TRUSTED if trusted else 0, self._stream()),
                   "bp_load_state")
        idx = ids.long()
        for n in self._OUT_ROWS:
            getattr(self, n)[idx] = getattr(state, n)

    def clone_envs(self, src_ids, dst_ids, trusted=False):
        """Fork: env dst_ids[i] becomes a bit-exact copy of env src_ids[i] (one kernel launch, no staging buffer); a source may be repeated (fan-out).
        The output rows follow.  Raises BpError, with no env touched, for an id outside the batch, a repeated destination or a destination that is also a
        source; trusted=True skips those checks and the host synchronisation they need."""
        src, dst = self._env_ids(src_ids), self._env_ids(dst_ids)
        if src.numel() != dst.numel():
            raise ValueError("clone_envs: %d sources for %d destinations" % (src.numel(), dst.numel()))
        _lib.check(self.L, self.h, self.L.bp_clone_state(self.h, _ptr(src), _ptr(dst), int(src.numel()), _lib.STATE_TRUSTED if trusted else 0,
                                                         self._stream()), "bp_clone_state")
        s, d = src.long(), dst.long()
        for n in self._OUT_ROWS:
            t = getattr(self, n)
            t[d] = t[s]

    # -- rgb_array frames (benchpush_amd/render.py states the frame) --------------------------------------
    def render_table(self):
        """The per-slot draw table (render.render_table) and the primitives (render.overlay_prims) this handle renders with."""
        from .. import render as R
        if getattr(self, "_rtable", None) is None:
            task = R.task_of(self)
            self._rtable = dict(R.render_table(task, self), prims=R.overlay_prims(task, self))
        return self._rtable

    def _upload_render_table(self):
        if getattr(self, "_rtable_loaded", False):
            return
        from .. import render as R
        t = self.render_table()
        order = np.ascontiguousarray(t["order"], np.int32)
        rgb = np.ascontiguousarray(t["rgb"][..., 0].astype(np.uint32) | (t["rgb"][..., 1].astype(np.uint32) << 8) | (t["rgb"][..., 2].astype(np.uint32) << 16))
        prims = R.prim_array(t["prims"])
        _lib.check(self.L, self.h, self.L.bp_set_render_table(self.h, order.shape[0], order.shape[1], order.ctypes.data_as(C.c_void_p),
                                                             rgb.ctypes.data_as(C.c_void_p), len(t["prims"]), C.cast(prims, C.c_void_p)),
                   "bp_set_render_table")
        self._rtable_loaded = True

    def frame_size(self, scale=None):
        """(H, W) of this task's frames at `scale` (cfg.render_scale if None)."""
        from .. import render as R
        return R.frame_size(R.task_of(self), self.cfg, scale)

    def render_frames(self, env_ids=None, scale=None, paths=None, out=None):
        """rgb_array frames of the envs `env_ids` (None: all): device uint8 [k, H, W, 3] (render.py states the frame).  paths: None or a list of k
        polylines (arrays [n, >= 2] of world points, or None), drawn as the planned path.  `out` may be a preallocated [k, H, W, 3] uint8 tensor.  (Box-delivery /
        area-clearing with an asynchronous slice open: a busy env is drawn in the middle of its env step.)"""
        from .. import render as R
        self._upload_render_table()
        task = R.task_of(self)
        ids = self._env_ids(env_ids)
        k = int(ids.numel())
        pt = pl = None
        max_path = 0
        if paths is not None:
            if len(paths) != k:
                raise ValueError("paths must hold one polyline (or None) per env id")
            pts = [np.zeros((0, 2)) if p is None or len(p) == 0 else np.asarray(p, np.float64).reshape(len(p), -1)[:, :2] for p in paths]
            max_path = max(1, max(len(p) for p in pts))
            host = np.zeros((k, max_path, 2), np.float64)
            for i, p in enumerate(pts):
                host[i, : len(p)] = p
            pt = torch.from_numpy(host).to(self.device)
            pl = torch.tensor([len(p) for p in pts], dtype=torch.int32, device=self.device)
        args = R.render_args(task, self.cfg, scale, max_path)
        if out is None:
            out = torch.empty((max(k, 0), args.height, args.width, 3), dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != (k, args.height, args.width, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("out must be a contiguous uint8 tensor [%d, %d, %d, 3]" % (k, args.height, args.width))
        _lib.check(self.L, self.h, self.L.bp_render(self.h, C.byref(args), _ptr(ids) if k else None, k, _ptr(pt), _ptr(pl), _ptr(out), self._stream()),
                   "bp_render")
        return out

    # -- episode metrics -----------------------------------------------------------------------------------
    def episode_metrics(self):
        """On-device ShipIceMetric (maze: MazeNamoMetric; box-delivery / area-clearing: TaskDrivenMetric, where success is the rate of completed boxes and
        0 / 0, x / 0 give NaN / inf like the host class): (rows [E, 6] float64 = efficiency, effort, episode reward, success, episode length, total_work of
        each env's most recently finished episode; counts [E] int32 = episodes finished so far).  Device tensors; rows of envs with
        count 0 are zero.  This is the block benchpush_amd.parallel.allgather_episode_metrics carries between GPUs."""
        rows = torch.zeros((self.num_envs, 6), dtype=torch.float64, device=self.device)
        cnt = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_get_episode_metrics(self.h, _ptr(rows), _ptr(cnt), self._stream()), "bp_get_episode_metrics")
        return rows, cnt

    def episode_history(self):
        """The episode lists of BaseMetric (base_metric.py:12-16) kept on the device: (ring [E, 8, 6] float64: the last 8 finished episodes of each
        env, episode n in slot n % 8; sums [E, 6] float64: the six row fields summed over all finished episodes; counts [E] int32).  No host
        round trip per step is needed to follow the episodes: see episode_lists() and benchpush_amd.parallel.gather_episode_sums."""
        ring = torch.zeros((self.num_envs, _lib.EPM_RING, _lib.EPM_COUNT), dtype=torch.float64, device=self.device)
        sums = torch.zeros((self.num_envs, _lib.EPM_COUNT), dtype=torch.float64, device=self.device)
        cnt = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_get_episode_history(self.h, _ptr(ring), _ptr(sums), _ptr(cnt), self._stream()), "bp_get_episode_history")
        return ring, sums, cnt

    def episode_lists(self):
        """Per env, the rows of its finished episodes in order (the last 8 at most): a list of E float64 arrays [n_e, 6] (host)."""
        ring, _, cnt = self.episode_history()
        ring, cnt = ring.cpu().numpy(), cnt.cpu().numpy()
        out = []
        for e in range(self.num_envs):
            n = int(cnt[e])
            out.append(np.stack([ring[e, k % _lib.EPM_RING] for k in range(max(0, n - _lib.EPM_RING), n)]) if n else np.zeros((0, _lib.EPM_COUNT)))
        return out

    # -- capacity flags and settings -------------------------------------------------------------------------
    def num_bodies(self):
        out = np.zeros(self.num_envs, np.int32)
        _lib.check(self.L, self.h, self.L.bp_get_num_bodies(self.h, out.ctypes.data_as(C.c_void_p)), "bp_get_num_bodies")
        return out

    def error_flags(self):
        """The in-kernel capacity flags of every env (BP_ERR_* bits, numpy int32 [E]; sticky since load) without raising: what check_errors() tests."""
        out = np.zeros(self.num_envs, np.int32)
        self.L.bp_check_errors(self.h, out.ctypes.data_as(C.c_void_p))
        return out

    def check_errors(self):
        out = np.zeros(self.num_envs, np.int32)
        rc = self.L.bp_check_errors(self.h, out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise _lib.BpError("capacity overflow in envs %s: %s" % (np.nonzero(out)[0][:8].tolist(),
                                                                     self.L.bp_last_error(self.h).decode()))

    def set_resettle(self, on=True):
        """Re-run the 1000 settle sub-steps on every reset instead of copying the settled per-trial template."""
        self.L.bp_set_resettle(self.h, int(on))

    # -- timing and clocks -----------------------------------------------------------------------------------
    def step_cycles(self):
        """Shader cycles each env's wavefront spent in the last step (numpy uint64 [E])."""
        out = np.zeros(self.num_envs, np.uint32)
        _lib.check(self.L, self.h, self.L.bp_get_step_cycles(self.h, out.ctypes.data_as(C.c_void_p)), "bp_get_step_cycles")
        return out.astype(np.uint64) << 8

    def clock_stamps(self):
        """uint64 [8, 2], row 0 used (the others stay zero): running sums of (shader-clock cycles, 100 MHz reference ticks) that one thread spent in the
        small kernel that follows every physics launch, each stay timed by that thread with both counters.  `clock_hz_between` turns two readings into the
        clock the chip held during the stays in between."""
        out = np.zeros((8, 2), np.uint64)
        _lib.check(self.L, self.h, self.L.bp_get_clock_stamps(self.h, out.ctypes.data_as(C.c_void_p)), "bp_get_clock_stamps")
        return out

    @staticmethod
    def clock_hz_between(c0, c1, with_span=False):
        """Shader clock between two `clock_stamps()` readings: cycles over reference time of the stays summed in between (sampled right after each physics
        launch; a stay is a few microseconds, so a handful of launches resolve the clock to about a percent).  The rows are scanned as before; only row 0
        is filled.  Returns (hz, row) or (None, None) if nothing was summed before both readings; with_span=True appends the summed reference time in seconds."""
        best = None
        for x in range(8):
            if c0[x, 1] == 0 or c1[x, 1] <= c0[x, 1]:
                continue
            if best is None or int(c0[x, 1]) > int(c0[best, 1]):
                best = x
        if best is None:
            return (None, None, None) if with_span else (None, None)
        span = int(c1[best, 1]) - int(c0[best, 1])
        hz = (int(c1[best, 0]) - int(c0[best, 0])) / span * 1e8
        return (hz, best, span / 1e8) if with_span else (hz, best)

    @staticmethod
    def clock_per_xcd(c0, c1):
        """Every row that was summed before both readings: [{xcd, mhz, span_ms}] -- what `clock_hz_between` chose from (a short span reads noisier)."""
        out = []
        for x in range(8):
            if c0[x, 1] == 0 or c1[x, 1] <= c0[x, 1]:
                continue
            span = int(c1[x, 1]) - int(c0[x, 1])
            out.append({"xcd": x, "mhz": (int(c1[x, 0]) - int(c0[x, 0])) / span * 1e2, "span_ms": span / 1e5})
        return out

    def cost_stats(self, max_launches=1024):
        """(sum, max) over the envs of the wave cycles each bp_step launch took since `enable_timing(True)`: uint64 [launches, 2], in shader cycles."""
        out = np.zeros((max_launches, 2), np.uint64)
        n = C.c_int32()
        _lib.check(self.L, self.h, self.L.bp_get_cost_stats(self.h, out.ctypes.data_as(C.c_void_p), int(max_launches), C.byref(n)), "bp_get_cost_stats")
        return out[: n.value] << np.uint64(8)

    def enable_timing(self, on=True):
        self.L.bp_enable_timing(self.h, int(on))

    def kernel_time_ms(self):
        p, r, n = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(self.L, self.h, self.L.bp_kernel_time_ms(self.h, C.byref(p), C.byref(r), C.byref(n)), "bp_kernel_time_ms")
        return p.value, r.value, n.value

    def debug_trace(self, buf, env=0):
        """Per-sub-step pose trace of one env into `buf`; only the -DBP_DEBUG_PATHS twin of the library records it (the product library returns BP_ESTATE
        for a non-null buffer, which surfaces here instead of leaving an all-zero trace behind)."""
        self._dbg = buf
        _lib.check(self.L, self.h, self.L.bp_debug_trace(self.h, _ptr(buf) if buf is not None else None, int(env)), "bp_debug_trace")


class _AdapterBase(Env):
    """What the four reference-shaped single-env classes (E = 1, the batched env in ``_b``) share; ``_STATE_FIELDS`` names the adapter's own fields
    that a state record carries."""

    _STATE_FIELDS = ()

    def _begin_episode(self):
        self.episode_idx = 0 if self.episode_idx is None else self.episode_idx + 1
        if self.episode_idx:
            self._b.check_errors()   # capacity flags of the episode that just ended (raises BpError)
        self._b.reset()
        self.t = 0

    @staticmethod
    def _state3(it):
        """info['state']: the rounded (x, y, theta) of an info row."""
        return (round(float(it[0]), 2), round(float(it[1]), 2), round(float(it[2]), 2))

    def save_state(self):
        """The whole env between two steps as an ``EnvState`` (benchpush_amd/state.py): the device state record plus this adapter's own fields."""
        from ..state import adapter_save
        return adapter_save(self, self._STATE_FIELDS)

    def restore_state(self, state):
        """Back to a state of save_state(): the following steps repeat bit for bit what followed the save."""
        from ..state import adapter_restore
        adapter_restore(self, state, self._STATE_FIELDS)

    def close(self):
        self._b.close()
