"""PlanningBasedPolicy: the reference's planning-based maze-NAMO baseline (benchpush/baselines/maze_NAMO/planning_based/policy.py) on the batched env.
Every env gets a path from the batched RRT (``BatchedMazeEnv.rrt_plan``: two passes, ``_densify``, ``prune_by_distance``) at the start of its episode,
and the reference's controller -- ``DP.ideal_control`` of a fresh ``DP`` at every step -- follows it, one launch per step for all envs
(``BatchedMazeEnv.track_waypoints``).  DESIGN.md "RRT" lists where this deviates from the reference.  How well the baseline solves the maze has not been
measured.
"""
from typing import List, Tuple

import numpy as np

from ...base_class import BasePolicy


class PlanningBasedPolicy(BasePolicy):
    """planner_type   'RRT' (anything else raises, like the reference)
    cfg            the env's configuration (dict / DotDict / None), as for ``BatchedMazeEnv``
    planner_config ``planning.RRTConfig``, a dict of its keyword arguments, or None (the reference's rrt_config.yaml)
    num_envs       envs that ``evaluate`` runs side by side
    env_kwargs     further keyword arguments of ``BatchedMazeEnv`` (layouts, num_layouts, base_seed, device, env_id_offset)"""

    def __init__(self, planner_type, cfg=None, planner_config=None, num_envs=1, max_episode_steps=400, **env_kwargs) -> None:
        super().__init__()
        if planner_type not in ['RRT']:   # only RRT is implemented, in the reference too
            raise Exception("Invalid planner type")
        self.planner_type = planner_type
        self.cfg, self.planner_config = cfg, planner_config
        self.num_envs, self.max_episode_steps, self.env_kwargs = int(num_envs), int(max_episode_steps), env_kwargs
        self.env = None
        self._first_episode = 0
        self._wipe()

    def _config(self):
        from ....planning import RRTConfig
        pc = self.planner_config
        return pc if isinstance(pc, RRTConfig) else RRTConfig(**dict(pc or {}))

    def _ensure_env(self):
        if self.env is None:
            from ....envs.maze_namo import BatchedMazeEnv
            self.env = BatchedMazeEnv(self.num_envs, cfg=self.cfg, **self.env_kwargs)
            self.env.reset()
        return self.env

    # -- the batched surface -------------------------------------------------------------------------------
    def act_batch(self, env=None, fresh=None):
        """Yaw actions [E] (device, float64) for all envs of `env` (None: the policy's own).  fresh: bool / uint8 [E] of the envs that have just started
        an episode -- they get a new plan, from RNG stream (global env id) * 2**32 + (episodes this policy has planned for the env); None on the first
        call means all, later none.  Paths, lengths and statuses stay on the device (``paths``, ``lengths``, ``status``); no host synchronisation."""
        import torch
        env = env or self._ensure_env()
        if self._bound is not env:                      # the paths belong to one env object
            self._wipe()
            self._bound, fresh = env, None
            self.episodes = torch.zeros(env.num_envs, dtype=torch.int64, device=env.device)
        first = self._plan is None
        if first or fresh is not None:
            cfg = self._config()
            mask = torch.ones(env.num_envs, dtype=torch.bool, device=env.device) if first else fresh.to(device=env.device, dtype=torch.bool)
            gid = env.env_id_offset + torch.arange(env.num_envs, dtype=torch.int64, device=env.device)
            self._plan = env.rrt_plan(streams=gid * (1 << 32) + self.episodes, active=mask.to(torch.uint8), config=cfg, out=self._plan)
            self.status = self._plan.status.clone() if first else torch.where(mask, self._plan.status, self.status)   # the others read SKIPPED
            self.paths, self.lengths = self._plan.paths, self._plan.lengths       # rows of envs that were not planned are as they were
            self.episodes = self.episodes + mask.to(torch.int64)
        cfg = self._config()
        self._out = env.track_waypoints(self.paths, self.lengths, Lfc=cfg.Lfc, dt=cfg.dt, out=self._out)
        actions = self._out[0]
        return torch.where(self.lengths > 0, actions, torch.zeros_like(actions))      # an env without a path (CAP, BAD_INPUT) goes straight on

    def evaluate(self, num_eps: int, model_eps: str = "latest") -> Tuple[List[float], List[float], List[float], List[float], str]:
        """Run `num_envs` envs side by side, every finished env starting its next episode at once, until `num_eps` episodes have finished.  Returns
        the reference's (success rates, efficiency scores, effort scores, rewards, 'RRT') of the finished episodes, from the on-device episode
        metrics.  An episode ends when the env terminates or truncates, or after `max_episode_steps` steps."""
        import torch
        env = self._ensure_env()
        env.reset()
        self._wipe()
        age = torch.zeros(env.num_envs, dtype=torch.int64, device=env.device)
        success, eff, effort, rewards = [], [], [], []
        fresh = None
        while len(eff) < num_eps:
            _, _, term, trunc, _ = env.step(self.act_batch(env, fresh))
            age += 1
            done = term.bool() | trunc.bool() | (age >= self.max_episode_steps)
            fresh = None
            if bool(done.any()):
                env.reset(done)                       # a reset of a running episode closes it as truncated
                rows, _ = env.episode_metrics()
                for r in rows[done].cpu().numpy():
                    eff.append(float(r[0])), effort.append(float(r[1])), rewards.append(float(r[2])), success.append(float(r[3]))
                age = torch.where(done, torch.zeros_like(age), age)
                fresh = done
        env.check_errors()
        return success, eff, effort, rewards, self.planner_type

    # -- the reference's single-env surface ------------------------------------------------------------------
    def _single_inputs(self, env, walls, obstacles):
        import torch
        from .... import _lib
        E, dev = env.num_envs, env.device
        w = np.asarray(walls if walls is not None else env.walls, np.float64).reshape(-1, 4)       # [[ax, ay, bx, by]] or [[(ax, ay), (bx, by)]]
        if obstacles is None:
            boxes, counts = env.box_polys()
        else:
            polys = [np.asarray(p, np.float64).reshape(-1, 2) for p in obstacles]
            boxes = np.zeros((E, max(1, len(polys)), _lib.MAXV, 2))
            counts = np.zeros((E, max(1, len(polys))), np.int32)
            for b, p in enumerate(polys):
                boxes[0, b, :len(p)], counts[0, b] = p, len(p)
            boxes, counts = torch.from_numpy(boxes).to(dev), torch.from_numpy(counts).to(dev)
        active = torch.zeros(E, dtype=torch.uint8, device=dev)
        active[0] = 1
        return torch.from_numpy(w).to(dev), boxes, counts, active

    def plan_path(self, start, goal, observation, maze_vertices, obstacles=None, robot_radius=None):
        """Sets ``path`` (numpy [n, 2]): the plan of env 0's RNG stream for (start, goal) among the walls `maze_vertices` (None: the env's) and the box
        polygons `obstacles` (None: env 0's own boxes), on the device.  robot_radius, if given, inflates the walls by 1.5 * (1.5 * robot_radius) like the
        reference; otherwise the planner config decides.  `observation` is not read."""
        import torch
        from ....planning import RRTConfig
        env = self._ensure_env()
        E, dev = env.num_envs, env.device
        cfg = self._config()
        if robot_radius is not None:
            cfg = RRTConfig(**dict({k: getattr(cfg, k) for k in RRTConfig.FIELDS + ("max_nodes", "seed", "max_waypoints", "passes", "Lfc", "dt")},
                                   inflate_radius=1.5 * (1.5 * float(robot_radius))))
        walls, boxes, counts, active = self._single_inputs(env, maze_vertices, obstacles)
        pts = torch.tensor([[float(start[0]), float(start[1])], [float(goal[0]), float(goal[1])]], dtype=torch.float64).to(dev)
        streams = torch.full((E,), env.env_id_offset * (1 << 32) + self._first_episode, dtype=torch.int64, device=dev)
        plan = env.rrt_plan(pts[0][None].expand(E, 2).contiguous(), pts[1][None].expand(E, 2).contiguous(), walls, boxes, counts, streams, active,
                            config=cfg)
        self._first_episode += 1
        self.path_status = int(plan.status[0])
        self.path = plan.paths[0, :int(plan.lengths[0])].cpu().numpy()

    def act(self, observation, **kwargs):
        """The reference's call: ``act(observation, robot_pos=(x, y, yaw), robot_radius=..., goal=(gx, gy), maze_vertices=..., obstacles=...,
        action_scale=...)`` returns ``omega / action_scale`` as a float.  Planner and controller run on the device (env 0 of the policy's env)."""
        import torch
        robot_pos, action_scale = kwargs.get('robot_pos', None), kwargs.get('action_scale', 1.0)
        env = self._ensure_env()
        if self.path is None:
            self.plan_path(start=robot_pos[0:2], goal=kwargs.get('goal', None), observation=observation, maze_vertices=kwargs.get('maze_vertices', None),
                           obstacles=kwargs.get('obstacles', None), robot_radius=kwargs.get('robot_radius', None))
        if len(self.path) == 0:
            raise ValueError("PlanningBasedPolicy.act: the planner gave no path (status %d)" % self.path_status)
        E, dev = env.num_envs, env.device
        cfg = self._config()
        pose = torch.tensor([float(v) for v in robot_pos[:3]], dtype=torch.float64).to(dev)[None, :].expand(E, 3).contiguous()
        paths = torch.from_numpy(np.ascontiguousarray(self.path, np.float64)).to(dev)[None].expand(E, len(self.path), 2).contiguous()
        active = torch.zeros(E, dtype=torch.uint8, device=dev)
        active[0] = 1
        actions, _ = env.track_waypoints(paths, poses=pose, active=active, Lfc=cfg.Lfc, dt=cfg.dt, action_scale=action_scale)
        return float(actions[0])

    def _wipe(self):
        self.path = self.path_status = None                                  # single-env surface: numpy [n, 2]
        self.paths = self.lengths = self.status = self.episodes = None      # batched surface, device tensors
        self._plan = self._out = self._bound = None

    def reset(self):
        """The next ``act`` plans a new path (the reference's reset)."""
        self.path = self.path_status = None

    def close(self):
        if self.env is not None:
            self.env.close()
            self.env = None
