"""maze-NAMO-v0 on MI355X: batched tensor environment + the reference-shaped single-env adapter.

Reference: benchpush/environments/maze_NAMO/maze_NAMO_env.py (MazeNAMO).  Same engine as ship-ice: the robot is a
kinematic body of five shapes (outline + four wheels, robot.py:77-118), boxes are dynamic squares, walls are static
Segment(radius 0.5) shapes; 400 sub-steps per step, reward from the work term and the BFS goal map, observation
uint8 [4, 192, 192] = rotated ego views of [footprint, boxes, walls, goal map].

The reference draws a new random box layout from the unseeded global ``random`` at every reset; here layout t comes
from ``random.Random(base_seed + t)`` and env e plays layout (global_env_id + episode) % T.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from ..config import default_cfg, maze_physics_params, maze_walls, merge_user_cfg
from ..gym_shim import spaces
from ..maze_scenario import generate_layout
from ..scenario import poly_centroid
from .batched import _AdapterBase
from .ship_ice import BatchedShipIceEnv, _ptr

__all__ = ["BatchedMazeEnv", "MazeNAMO", "default_layouts"]

MAZE_INFO_KEYS = ["x", "y", "theta", "total_work", "work", "collision_reward", "scaled_collision_reward", "dist_increment_reward",
                  "trial_success", "boundary_violated", "wall_collision", "total_ke", "total_impulse", "n_post_solve",
                  "n_contact_pts", "n_first_contact"]


def _maze_cfg(cfg):
    c = merge_user_cfg(default_cfg("maze_namo"), cfg)
    if c.maze_version == 1:      # maze_NAMO_env.py:68-73
        c.env = c.env1
    elif c.maze_version == 2:
        c.env = c.env2
    else:
        raise Exception("Invalid Maze Version!")
    return c


def default_layouts(cfg, num_layouts, base_seed=0):
    c = _maze_cfg(cfg) if "env" not in cfg else cfg
    walls = maze_walls(c)
    return [generate_layout(c, walls, base_seed + t) for t in range(num_layouts)]


class BatchedMazeEnv(BatchedShipIceEnv):
    """E independent maze-NAMO environments on one GPU (reset / step / world_polys / ... as BatchedShipIceEnv)."""

    render_task = "maze"

    def __init__(self, num_envs, cfg=None, layouts=None, device="cuda:0", env_id_offset=0, num_layouts=64, base_seed=0):
        self._open(num_envs, device, env_id_offset)
        self.cfg = _maze_cfg(cfg)
        self.params = maze_physics_params(self.cfg)
        self.goal = (self.cfg.env.goal_x, self.cfg.env.goal_y)
        self.max_yaw_rate_step = (math.pi / 2) / 15
        self.walls = maze_walls(self.cfg)
        if layouts is None:
            layouts = [generate_layout(self.cfg, self.walls, base_seed + t) for t in range(num_layouts)]
        self.layouts = layouts
        self.trials = layouts
        rv = self.cfg.robot.vertices
        head = ((rv[0][0] + rv[3][0]) / 2, (rv[0][1] + rv[3][1]) / 2)   # maze_NAMO_env.py:94-95
        tail = ((rv[1][0] + rv[2][0]) / 2, (rv[1][1] + rv[2][1]) / 2)
        bcfg = _lib.make_config(self.params, rv, head, tail, env_kind=_lib.ENV_MAZE, wheel_vertices=self.cfg.robot.wheel_vertices,
                                obstacle_size=self.cfg.obstacle_size)
        self._create(self.L.bp_create, bcfg)
        nbox = len(layouts[0]["centres"])
        if any(len(l["centres"]) != nbox for l in layouts):
            raise ValueError("all layouts must hold the same number of boxes")
        centres = np.ascontiguousarray(np.stack([np.asarray(l["centres"], np.float64).reshape(nbox, 2) for l in layouts]))
        walls = np.ascontiguousarray(self.walls, np.float64)
        # one start pose per layout: the fixed pose, or the layout's draw of cfg.random_start (the reference re-draws per episode from
        # python's unseeded global generator; here episode k plays layout (env + k) % T, whose start was drawn from Random(base_seed + t))
        start = np.ascontiguousarray(np.stack([np.asarray(l["start"], np.float64).reshape(3) for l in layouts]))
        _lib.check(self.L, self.h, self.L.bp_load_maze(self.h, len(layouts), nbox, centres.ctypes.data_as(C.c_void_p), len(walls),
                                                       walls.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p)), "bp_load_maze")
        self._alloc_io()

    def goal_map(self):
        """info['goal_dt'] of the reference: un-normalised wavefront distances, numpy [grid_h, grid_w]."""
        gh, gw = C.c_int32(), C.c_int32()
        _lib.check(self.L, self.h, self.L.bp_get_goal_map(self.h, None, C.byref(gh), C.byref(gw)), "bp_get_goal_map")
        out = np.zeros((gh.value, gw.value), np.float64)
        _lib.check(self.L, self.h, self.L.bp_get_goal_map(self.h, out.ctypes.data_as(C.c_void_p), None, None), "bp_get_goal_map")
        return out

    # -- the planning baseline's device calls (DESIGN.md "RRT") ---------------------------------------------
    def box_polys(self):
        """The box rows of ``world_polys()``: (verts [E, nbox, 20, 2] f64, counts [E, nbox] i32), contiguous."""
        verts, cnt = self.world_polys()
        n0 = 1 + len(self.cfg.robot.wheel_vertices)
        nbox = len(self.layouts[0]["centres"])
        return verts[:, n0:n0 + nbox].contiguous(), cnt[:, n0:n0 + nbox].contiguous()

    def rrt_workspace_bytes(self, config=None):
        """Bytes of workspace that ``rrt_plan`` needs with `config`: per env (max_nodes + 2) * 20 bytes, 520 KB at the reference's 26000."""
        from ..planning import RRTConfig
        cfg = (config or RRTConfig()).as_struct(self)
        n = self.L.bp_rrt_workspace_bytes(C.byref(cfg), self.num_envs)
        if n < 0:
            raise _lib.BpError("bp_rrt_workspace_bytes refuses the config (step <= 0, max_nodes < 1, max_waypoints < 2, ...)")
        return int(n)

    def rrt_plan(self, starts=None, goals=None, walls=None, boxes=None, counts=None, streams=None, active=None, config=None, workspace=None, out=None):
        """The reference's two-pass RRT, ``_densify`` and ``prune_by_distance`` for every env in one launch (bp_rrt_plan), no host synchronisation.
        DESIGN.md "RRT" states the semantics.  All tensors are contiguous and on the env's device:

        starts     float64 [E, 2] or None: info[:, :2]
        goals      float64 [E, 2] or None: cfg.env.goal_x / goal_y for every env
        walls      float64 [W, 4] or None: the handle's own walls
        boxes      float64 [E, B, V, 2] with counts int32 [E, B], or both None: the box rows of ``world_polys()``.  Convex, 3 .. V vertices, either
                   winding; a count of 0 skips the polygon
        streams    int64 [E] or None: env_id_offset + arange(E).  A plan depends on the env's own inputs and its stream only
        active     bool / uint8 [E] or None: envs with False get status RRT_SKIPPED and nothing else written
        config     ``planning.RRTConfig`` or None (the reference's values; inflate_radius None: 2.25 * cfg.robot.min_r)
        workspace  uint8 [>= rrt_workspace_bytes(config)] or None (allocated, and kept for the next call).  520 KB per env at the reference's max_nodes:
                   a caller short of memory plans with a smaller env, or in groups through `active`
        out        None or an earlier result to be overwritten

        Returns ``planning.RRTPlan``: status int32 [E] (_lib.RRT_*), n_nodes and iterations int32 [E, 2] (per pass), paths float64
        [E, max_waypoints, 2], lengths int32 [E].  Raises ValueError, before any launch, for a wrong dtype, device, shape or a non-contiguous tensor;
        BpError for what the library refuses.  Touches no environment state."""
        from ..planning import RRTConfig, RRTPlan
        E, dev, need = self.num_envs, self.device, self._need("rrt_plan")
        config = config or RRTConfig()
        cfg = config.as_struct(self)
        if starts is None:
            starts = self.info[:, :2].contiguous()
        if goals is None:
            if getattr(self, "_rrt_goals", None) is None:
                self._rrt_goals = torch.tensor([float(self.cfg.env.goal_x), float(self.cfg.env.goal_y)], dtype=torch.float64).to(dev)[None, :].expand(E, 2).contiguous()
            goals = self._rrt_goals
        if walls is None:
            if getattr(self, "_rrt_walls", None) is None:
                self._rrt_walls = torch.tensor(self.walls, dtype=torch.float64).reshape(-1, 4).to(dev)
            walls = self._rrt_walls
        if (boxes is None) != (counts is None):
            raise ValueError("rrt_plan: boxes and counts go together")
        if boxes is None:
            boxes, counts = self.box_polys()
        if streams is None:
            streams = self.env_id_offset + torch.arange(E, dtype=torch.int64, device=dev)
        need(starts, "starts", torch.float64, (E, 2))
        need(goals, "goals", torch.float64, (E, 2))
        need(walls, "walls", torch.float64, (None, 4))
        need(boxes, "boxes", torch.float64, (E, None, None, 2))
        need(counts, "counts", torch.int32, (E, boxes.shape[1]))
        need(streams, "streams", torch.int64, (E,))
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), (E,))
        P = int(cfg.max_waypoints)
        if out is not None:
            need(out.status, "out.status", torch.int32, (E,))
            need(out.n_nodes, "out.n_nodes", torch.int32, (E, 2))
            need(out.iterations, "out.iterations", torch.int32, (E, 2))
            need(out.paths, "out.paths", torch.float64, (E, P, 2))
            need(out.lengths, "out.lengths", torch.int32, (E,))
        else:
            out = RRTPlan(torch.zeros(E, dtype=torch.int32, device=dev), torch.zeros((E, 2), dtype=torch.int32, device=dev),
                          torch.zeros((E, 2), dtype=torch.int32, device=dev), torch.zeros((E, max(P, 0), 2), dtype=torch.float64, device=dev),
                          torch.zeros(E, dtype=torch.int32, device=dev))
        if workspace is None:
            nbytes = self.L.bp_rrt_workspace_bytes(C.byref(cfg), E)
            workspace = getattr(self, "_rrt_ws", None)
            if nbytes > 0 and (workspace is None or workspace.numel() < nbytes):
                workspace = self._rrt_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            elif workspace is None:
                workspace = torch.empty(16, dtype=torch.uint8, device=dev)     # a config that the library is about to refuse
        need(workspace, "workspace", torch.uint8, (None,))
        _lib.check(self.L, self.h, self.L.bp_rrt_plan(
            self.h, C.byref(cfg), _ptr(starts), _ptr(goals), _ptr(walls) if walls.shape[0] else None, int(walls.shape[0]),
            _ptr(boxes) if boxes.numel() else None, _ptr(counts) if boxes.numel() else None, int(boxes.shape[1]) if boxes.numel() else 0,
            int(boxes.shape[2]), _ptr(streams), _ptr(active), _ptr(workspace), int(workspace.numel()), _ptr(out.status), _ptr(out.n_nodes),
            _ptr(out.iterations), _ptr(out.paths), _ptr(out.lengths), self._stream()), "bp_rrt_plan")
        return out

    def track_waypoints(self, paths, lengths=None, poses=None, active=None, Lfc=0.5, dt=0.8, action_scale=None, out=None):
        """The reference's maze controller -- ``DP.ideal_control`` of a fresh ``DP`` on the path, as ``PlanningBasedPolicy.act`` calls it -- for every env
        in one launch (bp_track_waypoints), no host synchronisation.  paths float64 [E, P, 2]; lengths int32 [E] or None (all P); poses float64 [E, 3]
        or None (info[:, :3]); active bool / uint8 [E] or None; Lfc and dt as in rrt_config.yaml; action_scale None: max_yaw_rate_step; out None or
        (actions, diag) to be overwritten.  Returns (actions float64 [E] -- what ``step`` takes --, diag int32 [E, 2] = nearest and target index).  An
        env that is not active, has a length below 1, or a non-finite pose or counted waypoint gets NaN and (-1, -1)."""
        E, dev, need = self.num_envs, self.device, self._need("track_waypoints")
        need(paths, "paths", torch.float64, (E, None, 2))
        if lengths is not None:
            need(lengths, "lengths", torch.int32, (E,))
        if poses is None:
            poses = self.info[:, :3].contiguous()
        need(poses, "poses", torch.float64, (E, 3))
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), (E,))
        if out is not None:
            actions, diag = out
            need(actions, "out[0]", torch.float64, (E,))
            need(diag, "out[1]", torch.int32, (E, 2))
        else:
            actions, diag = torch.zeros(E, dtype=torch.float64, device=dev), torch.zeros((E, 2), dtype=torch.int32, device=dev)
        cfg = _lib.BpTrackWpConfig(P=int(paths.shape[1]), pad_=0, Lfc=float(Lfc), dt=float(dt),
                                   action_scale=float(self.max_yaw_rate_step if action_scale is None else action_scale))
        _lib.check(self.L, self.h, self.L.bp_track_waypoints(self.h, C.byref(cfg), _ptr(paths), _ptr(lengths), _ptr(poses), _ptr(active), _ptr(actions),
                                                             _ptr(diag), self._stream()), "bp_track_waypoints")
        return actions, diag


class MazeNAMO(_AdapterBase):
    """Reference-shaped single environment (E = 1): reset()/step() returns and info keys of maze_NAMO_env.py:325-485."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}

    def __init__(self, cfg=None, layouts=None, device="cuda:0", num_layouts=64, base_seed=0):
        super().__init__()
        self._b = BatchedMazeEnv(1, cfg=cfg, layouts=layouts, device=device, num_layouts=num_layouts, base_seed=base_seed)
        self.cfg = self._b.cfg
        self.beta = 1.5
        self.k = 2
        self.k_increment = 150
        self.episode_idx = None
        self.path = None
        self.low_dim_state = self.cfg.low_dim_state
        self.env_max_trial = 4000
        self.max_linear_speed = 1.0
        self.min_linear_speed = 0.0
        self.max_yaw_rate_step = (np.pi / 2) / 15
        self.action_space = spaces.Box(low=-1, high=1, dtype=np.float64)
        self.observation_shape = self._b.obs_shape
        if self.low_dim_state:  # maze_NAMO_env.py:106-112
            self.fixed_trial_idx = self.cfg.fixed_trial_idx
            n = (self.cfg.num_obstacles + 1) * 2 if self.cfg.randomize_obstacles else 8
            self.observation_space = spaces.Box(low=-10, high=30, shape=(n,), dtype=np.float64)
        else:
            self.observation_space = spaces.Box(low=0, high=255, shape=self.observation_shape, dtype=np.uint8)
        self.goal = self._b.goal
        self.total_work = [0, []]
        self.wall_collision = False
        self.t = 0
        self._goal_dt = self._b.goal_map()

    def _polys(self):
        verts, cnt = self._b.world_polys()
        verts, cnt = verts[0].cpu().numpy(), cnt[0].cpu().numpy()
        n0 = 1 + len(self.cfg.robot.wheel_vertices)
        nbox = len(self._b.layouts[0]["centres"])
        return [verts[i, : cnt[i]].copy() for i in range(n0, n0 + nbox)]

    def _low_dim(self, obstacles, it):
        """generate_observation_low_dim (maze_NAMO_env.py:488-504): <robot x, y, |centroid| of obstacles 1..n-1 at pairs 1..n-1>; like
        the reference's loop, obstacle 0 is never written and the last pair stays zero."""
        out = np.zeros((len(obstacles) + 1) * 2)
        out[0], out[1] = float(it[0]), float(it[1])
        for i in range(1, len(obstacles)):
            out[2 * i: 2 * i + 2] = poly_centroid(obstacles[i])
        return out

    def _observation(self, obstacles, it):
        return self._low_dim(obstacles, it) if self.low_dim_state else self._b.obs[0].cpu().numpy()

    def reset(self, seed=None, options=None):
        self._begin_episode()
        self.total_work = [0, []]
        self.wall_collision = False
        it = self._b.info[0].cpu().numpy()
        obstacles = self._polys()
        self.obstacles = obstacles
        info = {"state": self._state3(it), "total_work": self.total_work[0], "obs": obstacles, "box_count": 0, "goal_dt": self._goal_dt, "m_to_pix_scale": self.cfg.occ.m_to_pix_scale}
        return self._observation(obstacles, it), info

    def step(self, action):
        self.t += 1
        a = torch.tensor([float(np.asarray(action, dtype=np.float64).reshape(-1)[0])], dtype=torch.float64)
        self._b.step(a)
        it = self._b.info[0].cpu().numpy()
        reward = float(self._b.reward[0].item())
        terminated = bool(self._b.terminated[0].item())
        obstacles = self._polys()
        self.obstacles = obstacles
        self.total_work[0] = float(it[3])
        self.total_work[1].append(float(it[4]))
        self.wall_collision = bool(it[10])
        info = {"state": self._state3(it), "total_work": self.total_work[0],
                "collision reward": float(it[5]), "scaled collision reward": float(it[6]), "dist increment reward": float(it[7]),
                "trial_success": bool(it[8]), "obs": obstacles}
        if self.cfg.log_obs:
            self.log_observation()
        return self._observation(obstacles, it), reward, terminated, False, info

    def log_observation(self):
        """`cfg.log_obs` (maze_NAMO_env.py:482-483, 539-595): <cfg.output_dir>/t<episode_idx>/<t>_footprint, _movable_obs, _fixed_obs, _local_distance_map (the four
        observation channels) and _distance_map (the global goal-distance map: wavefront distances over their maximum, walls and unreached cells 1.0)."""
        from ..obs_log import dump_channels
        o = self._b.obs[0].cpu().numpy()               # [footprint, boxes, walls, distance] (occupancy_map.py:142-202)
        g = np.asarray(self._goal_dt, np.float64)
        gn = g / g.max() if g.max() > 0 else g.copy()
        gn[g == 0] = 1.0
        return dump_channels(self.cfg.output_dir, self.episode_idx, self.t,
                             {"footprint": o[0], "movable_obs": o[1], "fixed_obs": o[2], "distance_map": gn, "local_distance_map": o[3]})

    _STATE_FIELDS = ("t", "total_work", "episode_idx", "path", "obstacles", "wall_collision")

    def update_path(self, new_path, scatter=False):
        self.path = new_path

    def render(self, mode="human", close=False):
        """rgb_array: the frame of this env with the path of update_path (numpy [H, W, 3]; benchpush_amd/render.py).  human: no window; with
        cfg.render_snapshot every call writes <output_dir>/t<episode_idx>/<t>.png (maze_NAMO_env.py:604-606), otherwise warns once.  Returns None."""
        from ..render import adapter_render, snapshot_path
        snap = snapshot_path(self.cfg, self.episode_idx, self.t) if mode == "human" and self.cfg.get("render_snapshot", False) else None
        return adapter_render(self, mode, self.path, snap)
