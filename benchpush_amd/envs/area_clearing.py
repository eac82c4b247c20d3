"""area-clearing-v0 on MI355X: batched tensor environment + the reference-shaped single-env adapter.

Reference: benchpush/environments/area_clearing/area_clearing.py (AreaClearingEnv).  Same engine and kernels as box-delivery-v0
with ``bp_bd_config.task = 1``: waypoints from the PositionController, execute_robot_path under the DP controller (look-ahead
Lfc 0.5, velocity x5, omega / 2), then ``sim.steps`` more sim steps; a box is cleared when its polygon no longer intersects the
clearance boundary; rewards from the change of each box's distance to the nearest boundary goal point.

Layouts: trial t = ``random.Random(base_seed + t)`` with the reference's draw order (it uses the unseeded global ``random``).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..area_clearing_scenario import area_clearing_params, area_clearing_physics_params, env_layout, generate_trials, goal_points
from ..config import default_cfg, merge_user_cfg
from ..gym_shim import spaces
from .batched import _AdapterBase
from .box_delivery import BatchedBoxDeliveryEnv, low_dim_observation
from .ship_ice import _ptr

__all__ = ["BatchedAreaClearingEnv", "AreaClearingEnv", "AC_INFO_KEYS"]
AC_INFO_KEYS = ["x", "y", "theta", "total_work", "collision_reward", "diff_reward", "box_completed_reward", "box_count", "ministeps",
                "robot_hit_obstacle", "substeps", "robot_distance", "t", "num_waypoints", "work", "pushing_reward"]


def _ac_cfg(cfg):
    c = merge_user_cfg(default_cfg("area_clearing"), cfg)
    if c.env not in c.envs:
        raise FileNotFoundError(f"Environment config {c.env} not found")   # area_clearing.py:105-108
    if c.agent.action_type not in ("heading", "position", "velocity"):
        raise ValueError("agent.action_type must be heading, position or velocity")
    return c


class BatchedAreaClearingEnv(BatchedBoxDeliveryEnv):
    """E independent area-clearing environments on one GPU: reset(mask) / step(actions) with device tensors; step_async(actions, budget) / drain() /
    async_open / slices, the asynchronous step, are BatchedBoxDeliveryEnv's (the two tasks share the step kernels)."""

    render_task = "area_clearing"
    _task_cfg = staticmethod(_ac_cfg)
    _physics_params = staticmethod(area_clearing_physics_params)
    _task_params = staticmethod(area_clearing_params)
    _generate_trials = staticmethod(generate_trials)
    _same_box_count = False

    def __init__(self, num_envs, cfg=None, trials=None, device="cuda:0", env_id_offset=0, num_trials=32, base_seed=0, bd_overrides=None):
        super().__init__(num_envs, cfg, trials, device, env_id_offset, num_trials, base_seed, bd_overrides)
        self.target_speed = float(self.cfg.controller.target_speed)     # area_clearing.py:196-209: what a 'velocity' action is scaled by
        self.max_yaw_rate_step = (np.pi / 2) / 15

    def _bd_config(self):
        lay = env_layout(self.cfg)
        self.goal_points = goal_points(self.cfg)
        bcfg = super()._bd_config()
        _lib.fill_area_geometry(bcfg, lay.boundary, lay.outer_boundary, self.cfg.agent.footprint_vertices, self.goal_points)
        bcfg.distance_scale_max = self.bd_params["distance_scale_max"]
        return bcfg

    ASYNC_BUDGET = 3000   # the best of the measured sweep for this task (profiles/async/README.md: its env steps have no stragglers, so slicing only adds launches)

    def step_async(self, actions, budget=ASYNC_BUDGET):
        """BatchedBoxDeliveryEnv.step_async with this task's default budget."""
        return super().step_async(actions, budget)

    # -- the planning baseline's device calls (DESIGN.md "GTSP") --------------------------------------------
    def push_box_polys(self):
        """The box rows of ``world_polys()``: (verts [E, nbox, 20, 2] f64, counts [E, nbox] i32), contiguous."""
        verts, cnt = self.world_polys()
        return verts[:, 6:6 + self.nbox].contiguous(), cnt[:, 6:6 + self.nbox].contiguous()

    def boundary_goals(self):
        """``planning.boundary_goals`` of this handle's layout, computed once: (numpy [G, 2, 2], device tensor [G, 4])."""
        if getattr(self, "_gtsp_goals", None) is None:
            from ..planning import boundary_goals
            lay = env_layout(self.cfg)
            g = boundary_goals(lay.boundary, lay.walls if "walls" in lay else [])
            self._gtsp_goals = (g, torch.from_numpy(np.ascontiguousarray(g.reshape(-1, 4))).to(self.device))
        return self._gtsp_goals

    def _gtsp_struct(self, config, goals=None):
        from ..planning import GTSPConfig
        config = config or GTSPConfig()
        G = config.num_goals
        if G is None:
            G = int(goals.shape[0]) if goals is not None else len(self.boundary_goals()[0])
        return config.as_struct(self, num_goals=G)

    def gtsp_workspace_bytes(self, config=None):
        """Bytes of workspace that ``gtsp_plan`` needs with `config`: per env 2^max_boxes * max_boxes * num_goals int32 (160 KB at 10 boxes, 4 goals)."""
        cfg = self._gtsp_struct(config)
        n = self.L.bp_gtsp_workspace_bytes(C.byref(cfg), self.num_envs)
        if n < 0:
            raise _lib.BpError("bp_gtsp_workspace_bytes refuses the config (max_boxes outside 1 .. 12, num_goals outside 1 .. 8, ...)")
        return int(n)

    def gtsp_plan(self, poses=None, boxes=None, counts=None, goals=None, active=None, config=None, workspace=None, out=None, return_weights=False):
        """The reference's GTSP push plan for every env in one launch (bp_gtsp_plan), solved exactly, no host synchronisation.  DESIGN.md "GTSP"
        states the semantics.  All tensors are contiguous and on the env's device:

        poses      float64 [E, 3] or None: info[:, :3]
        boxes      float64 [E, B, V, 2] with counts int32 [E, B], or both None: ``push_box_polys()``.  Convex, 3 .. V vertices, either winding; a count
                   of 0 skips the slot.  A box is pushed iff it intersects the handle's clearance boundary
        goals      float64 [G, 4] = (ax, ay, bx, by) or None: ``boundary_goals()`` of the handle's layout
        active     bool / uint8 [E] or None: envs with False get status GTSP_SKIPPED and nothing else written
        config     ``planning.GTSPConfig`` or None (the reference's values)
        workspace  uint8 [>= gtsp_workspace_bytes(config)] or None (allocated, and kept for the next call)
        out        None or an earlier result to be overwritten
        return_weights  also the integer weight matrix, int32 [E, N_max, N_max] with N_max = max_boxes * G + 1

        Returns ``planning.GTSPPlan``.  Raises ValueError, before any launch, for a wrong dtype, device, shape or a non-contiguous tensor; BpError for
        what the library refuses.  Touches no environment state."""
        from ..planning import GTSPPlan
        E, dev, need = self.num_envs, self.device, self._need("gtsp_plan")
        if poses is None:
            poses = self.info[:, :3].contiguous()
        if (boxes is None) != (counts is None):
            raise ValueError("gtsp_plan: boxes and counts go together")
        if boxes is None:
            boxes, counts = self.push_box_polys()
        if goals is None:
            goals = self.boundary_goals()[1]
        need(goals, "goals", torch.float64, (None, 4))
        cfg = self._gtsp_struct(config, goals)
        if goals.shape[0] != cfg.num_goals:
            raise ValueError("gtsp_plan: goals has %d rows, config.num_goals is %d" % (goals.shape[0], cfg.num_goals))
        need(poses, "poses", torch.float64, (E, 3))
        need(boxes, "boxes", torch.float64, (E, None, None, 2))
        need(counts, "counts", torch.int32, (E, boxes.shape[1]))
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), (E,))
        nm, G = max(int(cfg.max_boxes), 0), int(cfg.num_goals)
        Nm = nm * G + 1
        if out is not None:
            need(out.status, "out.status", torch.int32, (E,))
            need(out.n_push, "out.n_push", torch.int32, (E,))
            need(out.tour, "out.tour", torch.int32, (E, nm))
            need(out.cost, "out.cost", torch.int32, (E,))
            need(out.paths, "out.paths", torch.float64, (E, 2 * nm + 1, 3))
            need(out.lengths, "out.lengths", torch.int32, (E,))
            need(out.track_id, "out.track_id", torch.int32, (E,))
            need(out.track_setpoint, "out.track_setpoint", torch.float64, (E, 2))
            if return_weights:
                if out.weights is None:
                    raise ValueError("gtsp_plan: return_weights needs out.weights")
                need(out.weights, "out.weights", torch.int32, (E, Nm, Nm))
        else:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
            big = nm > _lib.GTSP_MAX_BOXES or G > _lib.GTSP_MAX_GOALS        # a config that the library is about to refuse: allocate nothing large
            out = GTSPPlan(z(E, torch.int32), z(E, torch.int32), z((E, nm), torch.int32), z(E, torch.int32), z((E, 2 * nm + 1, 3), torch.float64),
                           z(E, torch.int32), z(E, torch.int32), z((E, 2), torch.float64),
                           z((E, Nm, Nm), torch.int32) if return_weights and not big else None)
        if workspace is None:
            nbytes = self.L.bp_gtsp_workspace_bytes(C.byref(cfg), E)
            workspace = getattr(self, "_gtsp_ws", None)
            if nbytes > 0 and (workspace is None or workspace.numel() < nbytes):
                workspace = self._gtsp_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            elif workspace is None:
                workspace = torch.empty(16, dtype=torch.uint8, device=dev)     # a config that the library is about to refuse
        need(workspace, "workspace", torch.uint8, (None,))
        _lib.check(self.L, self.h, self.L.bp_gtsp_plan(
            self.h, C.byref(cfg), _ptr(poses), _ptr(boxes) if boxes.numel() else None, _ptr(counts) if boxes.numel() else None,
            int(boxes.shape[1]) if boxes.numel() else 0, int(boxes.shape[2]), _ptr(goals), _ptr(active), _ptr(workspace), int(workspace.numel()),
            _ptr(out.status), _ptr(out.n_push), _ptr(out.tour), _ptr(out.cost), _ptr(out.paths), _ptr(out.lengths), _ptr(out.track_id),
            _ptr(out.track_setpoint), _ptr(out.weights) if return_weights else None, self._stream()), "bp_gtsp_plan")
        return out

    def track_pushes(self, plan, tracker, poses=None, active=None, config=None, out=None):
        """One call of the reference's ``PlanningBasedPolicy.act`` after planning, for every env in one launch (bp_gtsp_track), no host
        synchronisation.  plan: a ``GTSPPlan`` (its paths and lengths are read); tracker: a ``planning.GTSPTrackerState``, updated in place; poses
        float64 [E, 3] or None (info[:, :3]); active bool / uint8 [E] or None; config: the ``GTSPConfig`` the plan was made with (None: the
        reference's values); out None or (actions, diag) to be overwritten.  Returns (actions float64 [E, 2] -- what ``step`` takes with
        action_type 'velocity' --, diag int32 [E] = current_point_id).  An env that is not active, has a length below 2, or a non-finite pose or
        counted waypoint gets NaN and -1, and its state is left as it is."""
        E, dev, need = self.num_envs, self.device, self._need("track_pushes")
        cfg = self._gtsp_struct(config)
        P = 2 * int(cfg.max_boxes) + 1
        need(plan.paths, "plan.paths", torch.float64, (E, P, 3))
        need(plan.lengths, "plan.lengths", torch.int32, (E,))
        need(tracker.ids, "tracker.ids", torch.int32, (E,))
        need(tracker.setpoint, "tracker.setpoint", torch.float64, (E, 2))
        if poses is None:
            poses = self.info[:, :3].contiguous()
        need(poses, "poses", torch.float64, (E, 3))
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), (E,))
        if out is not None:
            actions, diag = out
            need(actions, "out[0]", torch.float64, (E, 2))
            need(diag, "out[1]", torch.int32, (E,))
        else:
            actions, diag = torch.zeros((E, 2), dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
        _lib.check(self.L, self.h, self.L.bp_gtsp_track(self.h, C.byref(cfg), _ptr(plan.paths), _ptr(plan.lengths), _ptr(poses), _ptr(active),
                                                        _ptr(tracker.ids), _ptr(tracker.setpoint), _ptr(actions), _ptr(diag), self._stream()),
                   "bp_gtsp_track")
        return actions, diag


class AreaClearingEnv(_AdapterBase):
    """Reference-shaped single environment (E = 1): reset()/step() returns and info keys of area_clearing.py:563-778."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}

    def __init__(self, cfg=None, trials=None, device="cuda:0", num_trials=32, **kwargs):
        super().__init__()
        self._b = BatchedAreaClearingEnv(1, cfg=cfg, trials=trials, device=device, num_trials=num_trials)
        self.cfg = self._b.cfg
        from ..obs_log import refuse_render_log_obs
        refuse_render_log_obs(self.cfg, "area-clearing-v0")
        lay = env_layout(self.cfg)
        self.boundary_vertices, self.outer_boundary_vertices = lay.boundary, lay.outer_boundary
        self.walls = lay.walls if "walls" in lay else []
        self.static_obstacles = lay.static_obstacles if "static_obstacles" in lay else []
        self.goal_points = [tuple(g) for g in self._b.goal_points]
        self.num_box = self._b.nbox
        self.max_yaw_rate_step = (np.pi / 2) / 15
        lp = self._b.obs_shape[0]
        if self.cfg.agent.action_type == "velocity":      # area_clearing.py:200-205
            self.action_space = spaces.Box(low=-1, high=1, shape=(2,), dtype=np.float32)
        elif self.cfg.agent.action_type == "position":
            self.action_space = spaces.Box(low=0, high=lp * lp, shape=(1,), dtype=np.int32)
        else:
            self.action_space = spaces.Box(low=-1, high=1, shape=(1,), dtype=np.float32)
        self.observation_shape = self._b.obs_shape
        self.low_dim_state = self.cfg.low_dim_state
        if self.low_dim_state:                            # area_clearing.py:212-215
            self.fixed_trial_idx = self.cfg.fixed_trial_idx
            self.observation_space = spaces.Box(low=-10, high=30, shape=(self.cfg.num_obstacles * 2,), dtype=np.float32)
        else:
            self.observation_space = spaces.Box(low=0, high=255, shape=self.observation_shape, dtype=np.uint8)
        self.episode_idx = None
        self.t = 0
        self.box_clearance_statuses = [False] * self.num_box

    def _boxes(self):
        verts, cnt = self._b.world_polys()
        verts, cnt = verts[0].cpu().numpy(), cnt[0].cpu().numpy()
        return [verts[6 + k, : cnt[6 + k]].copy() for k in range(self.num_box)]

    def _statuses(self, boxes):
        """box_clearance_statuses: the box polygon no longer intersects the (convex) clearance boundary (area_clearing.py:1122-1140)."""
        bd = np.asarray(self.boundary_vertices, np.float64)

        def sep(a, b):
            o = 1.0 if np.sum(a[:, 0] * np.roll(a[:, 1], -1) - np.roll(a[:, 0], -1) * a[:, 1]) > 0 else -1.0
            for i in range(len(a)):
                e = a[(i + 1) % len(a)] - a[i]
                cr = e[0] * (b[:, 1] - a[i, 1]) - e[1] * (b[:, 0] - a[i, 0])
                if np.all(cr * o < 0):
                    return True
            return False
        return [bool(sep(bd, np.asarray(b)) or sep(np.asarray(b), bd)) for b in boxes]

    def _low_dim(self, boxes):
        return low_dim_observation(boxes)

    def _result(self, info):
        """low_dim_state: the vector is the observation; otherwise it rides along in info (area_clearing.py:599-606,766-772)."""
        if self.low_dim_state:
            return info.pop("low_level_observation")
        return self._b.obs[0].cpu().numpy()

    def reset(self, seed=None, options=None):
        self._begin_episode()
        it = self._b.info[0].cpu().numpy()
        boxes = self._boxes()
        self.box_clearance_statuses = [False] * self.num_box
        info = {"state": self._state3(it), "total_work": 0, "obs": boxes, "box_count": 0,
                "boundary": self.boundary_vertices, "walls": self.walls, "static_obstacles": self.static_obstacles,
                "goal_positions": self.goal_points, "low_level_observation": self._low_dim(boxes)}
        return self._result(info), info

    def step(self, action):
        self.t += 1
        a = torch.tensor(np.asarray(action, dtype=np.float64).reshape(-1)[: self._b.action_dim], dtype=torch.float64)
        self._b.step(a)
        it = self._b.info[0].cpu().numpy()
        boxes = self._boxes()
        self.box_clearance_statuses = self._statuses(boxes)
        info = {"state": self._state3(it), "total_work": float(it[3]),
                "collision reward": float(it[4]), "diff_reward": float(it[5]), "box_completed_reward": float(it[6]), "obs": boxes,
                "box_completed_statuses": self.box_clearance_statuses, "box_count": int(it[7]), "ministeps": float(it[8]),
                "low_level_observation": self._low_dim(boxes)}
        return (self._result(info), float(self._b.reward[0].item()), bool(self._b.terminated[0].item()),
                bool(self._b.truncated[0].item()), info)

    _STATE_FIELDS = ("t", "episode_idx", "box_clearance_statuses")

    def render(self, mode="human", close=False):
        """rgb_array: the frame of this env with the controller's current waypoints as the path (numpy [H, W, 3]; benchpush_amd/render.py).
        human: no window; with render.show set, every anim.plot_steps-th step writes <output_dir>/t<episode_idx>/<t>.png (area_clearing.py:1145-1149),
        otherwise warns once.  Returns None."""
        from ..render import adapter_render, snapshot_path
        r, anim = self.cfg.get("render", None), self.cfg.get("anim", None)
        show = bool(r is not None and r.get("show", False))
        every = int(anim.get("plot_steps", 0)) if anim is not None else 0
        snap = None
        if mode == "human" and show and every > 0 and self.t % every == 0:
            snap = snapshot_path(self.cfg, self.episode_idx, self.t)
        _, wp, nwp = self._b.box_state()
        return adapter_render(self, mode, wp[0, : int(nwp[0]), :2], snap)
