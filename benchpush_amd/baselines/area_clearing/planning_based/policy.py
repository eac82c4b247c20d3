"""PlanningBasedPolicy: the reference's planning-based area-clearing baseline ("GTSP", benchpush/baselines/area_clearing/planning_based/policy.py) on the
batched env.  Every env gets a push plan at the start of its episode -- one push path per box and boundary goal, the integer transition costs of the
reference's GTSP instance, and the optimal tour by an exact set DP where the reference calls the GLNS heuristic (``BatchedAreaClearingEnv.gtsp_plan``) --
and the reference's controller follows it, one launch per step for all envs (``BatchedAreaClearingEnv.track_pushes``).  DESIGN.md "GTSP" lists where
this deviates from the reference.  ``evaluate`` with num_envs > 1 scores the envs side by side from the on-device episode metrics
(examples/eval_task_metrics.py prints the means).
"""
from typing import List, Tuple

import numpy as np

from ...base_class import BasePolicy


class PlanningBasedPolicy(BasePolicy):
    """glns_executable_path  accepted for the reference's signature and ignored: the tour is solved exactly on the device
    cfg             the env's configuration (dict / DotDict / None), as for ``BatchedAreaClearingEnv``; ``evaluate`` sets action_type 'velocity'
    num_envs        envs of the policy's own env (``act_batch`` without an env, and the single-env surface, which uses env 0)
    planner_config  ``planning.GTSPConfig``, a dict of its keyword arguments, or None (the reference's values)
    t_max           sim.t_max of ``evaluate`` (the reference: 2000)
    env_kwargs      further keyword arguments of the env (trials, num_trials, base_seed, device)"""

    def __init__(self, glns_executable_path=None, cfg=None, num_envs=1, planner_config=None, t_max=2000, **env_kwargs) -> None:
        super().__init__()
        self.glns_executable_path = glns_executable_path
        self.cfg, self.planner_config = cfg, planner_config
        self.num_envs, self.t_max, self.env_kwargs = int(num_envs), int(t_max), env_kwargs
        self.boundary_vertices = self.walls = self.static_obstacles = self.boundary_goals = None
        self.current_point_id = 0
        self.env = None
        self._wipe()

    def _config(self, **over):
        from ....planning import GTSPConfig
        pc = self.planner_config
        kw = dict(pc.as_dict(), v_scale=pc.v_scale, w_scale=pc.w_scale) if isinstance(pc, GTSPConfig) else dict(pc or {})
        return GTSPConfig(**dict(kw, **over))

    def _velocity_cfg(self):
        from ....config import default_cfg, merge_user_cfg
        c = merge_user_cfg(default_cfg("area_clearing"), self.cfg)
        c.agent.action_type = 'velocity'          # the reference's evaluate sets both on the env it made
        c.sim.t_max = self.t_max
        return c

    def _ensure_env(self):
        if self.env is None:
            from ....envs.area_clearing import BatchedAreaClearingEnv
            self.env = BatchedAreaClearingEnv(self.num_envs, cfg=self._velocity_cfg(), **self.env_kwargs)
            self.env.reset()
        return self.env

    # -- the batched surface -------------------------------------------------------------------------------
    def act_batch(self, env=None, fresh=None):
        """Velocity actions [E, 2] (device, float64) for all envs of `env` (None: the policy's own).  fresh: bool / uint8 [E] of the envs that have just
        started an episode -- they get a new plan; None on the first call means all, later none.  Plans and controller states stay on the device
        (``plan``, ``tracker``, ``status``); no host synchronisation."""
        import torch
        from ....planning import GTSPTrackerState
        env = env or self._ensure_env()
        if self._bound is not env:                      # the plans belong to one env object
            self._wipe()
            self._bound, fresh = env, None
        cfg = self._config()
        first = self.plan is None
        if first or fresh is not None:
            mask = torch.ones(env.num_envs, dtype=torch.bool, device=env.device) if first else fresh.to(device=env.device, dtype=torch.bool)
            self.plan = env.gtsp_plan(active=mask.to(torch.uint8), config=cfg, out=self.plan)
            self.status = self.plan.status.clone() if first else torch.where(mask, self.plan.status, self.status)   # the others read SKIPPED
            if first:
                self.tracker = GTSPTrackerState(env.num_envs, env.device)
            self.tracker.take(self.plan, mask)
        self._out = env.track_pushes(self.plan, self.tracker, config=cfg, out=self._out)
        return torch.nan_to_num(self._out[0], nan=0.0)      # an env without a path to follow (nothing to push, CAP, INVALID) stands still

    def evaluate(self, num_eps: int, model_eps: str = "latest", max_episode_steps=None) -> Tuple[List[float], List[float], List[float], List[float], str]:
        """Returns (success rates, efficiency scores, effort scores, rewards, 'GTSP') of `num_eps` finished episodes, with action_type 'velocity' and
        sim.t_max = `t_max`.
        num_envs == 1: the reference's loop on the reference-shaped single env -- plan where an episode begins, steer, step, and feed the host
        ``TaskDrivenMetric``, one episode after another (`max_episode_steps` is not used).
        num_envs > 1: the policy's `num_envs` envs side by side, every finished env starting its next episode at once, until at least `num_eps` episodes
        have finished; the four lists come from the on-device episode metrics (``episode_metrics()``, the same TaskDrivenMetric), in the order the
        episodes finished (env order within a step).  An episode ends when the env terminates or truncates, or after `max_episode_steps` steps
        (None: no limit beside sim.t_max); the reset that follows closes it as truncated.
        Planner, controller and simulation run on the device either way."""
        if self.num_envs > 1:
            return self._evaluate_batched(num_eps, max_episode_steps)
        from ....envs.area_clearing import AreaClearingEnv
        from ....metrics.task_driven_metric import TaskDrivenMetric
        env = AreaClearingEnv(cfg=self._velocity_cfg(), **self.env_kwargs)
        metric = TaskDrivenMetric(alg_name="GTSP", robot_mass=env.cfg.agent.mass)
        try:
            for _ in range(num_eps):
                _, info = env.reset()
                metric.reset(info)
                self._wipe()
                while True:
                    action = self.act_batch(env._b)
                    _, reward, done, truncated, info = env.step(action[0].cpu().numpy())
                    metric.update(info=info, reward=reward, eps_complete=(done or truncated))
                    if done or truncated:
                        break
            env._b.check_errors()
        finally:
            env.close()
            self._wipe()
        return metric.success_rates, metric.efficiency_scores, metric.effort_scores, metric.rewards, "GTSP"

    def _evaluate_batched(self, num_eps, max_episode_steps):
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
            done = term.bool() | trunc.bool()
            if max_episode_steps is not None:
                done = done | (age >= int(max_episode_steps))
            fresh = None
            if bool(done.any()):
                env.reset(done)                       # a reset of a running episode closes it as truncated
                rows, _ = env.episode_metrics()
                for r in rows[done].cpu().numpy():
                    eff.append(float(r[0])), effort.append(float(r[1])), rewards.append(float(r[2])), success.append(float(r[3]))
                age = torch.where(done, torch.zeros_like(age), age)
                fresh = done
        env.check_errors()
        return success, eff, effort, rewards, "GTSP"

    # -- the reference's single-env surface ------------------------------------------------------------------
    def update_boundary_and_obstacles(self, boundary, walls, static_obstacles):
        """Keeps the three and computes ``boundary_goals`` (numpy [G, 2, 2]) from `boundary` and `walls`; needs no GPU.  Whether a box is to be pushed
        is decided against the clearance boundary of the policy's env, which `boundary` is expected to be."""
        from ....planning import boundary_goals
        self.boundary_vertices, self.walls, self.static_obstacles = boundary, walls, static_obstacles
        self.boundary_goals = boundary_goals(boundary, walls)

    def plan_path(self, agent_pos, observation, obstacles=None):
        """Sets ``path`` (numpy [2 n + 1, 3]): the pose, then per pushed box the start and the end of its push path with the heading between them.
        `obstacles`: the box polygons (None: env 0's own boxes).  Planned on the device as env 0 of the policy's env; `observation` is not read."""
        import torch
        from .... import _lib
        env = self._ensure_env()
        E, dev = env.num_envs, env.device
        if obstacles is None:
            boxes, counts = env.push_box_polys()
        else:
            polys = [np.asarray(p, np.float64).reshape(-1, 2) for p in obstacles]
            boxes = np.zeros((E, max(1, len(polys)), _lib.MAXV, 2))
            counts = np.zeros((E, max(1, len(polys))), np.int32)
            for b, p in enumerate(polys):
                boxes[0, b, :len(p)], counts[0, b] = p, len(p)
            boxes, counts = torch.from_numpy(boxes).to(dev), torch.from_numpy(counts).to(dev)
        goals = None
        if self.boundary_goals is not None:
            goals = torch.from_numpy(np.ascontiguousarray(np.asarray(self.boundary_goals, np.float64).reshape(-1, 4))).to(dev)
        active = torch.zeros(E, dtype=torch.uint8, device=dev)
        active[0] = 1
        pose = torch.tensor([float(v) for v in agent_pos[:3]], dtype=torch.float64).to(dev)[None, :].expand(E, 3).contiguous()
        self._single_cfg = self._config(v_scale=1.0, w_scale=1.0, num_goals=None if goals is None else int(goals.shape[0]))
        self._single_plan = env.gtsp_plan(pose, boxes, counts, goals, active, config=self._single_cfg)
        self._single_tracker = self._single_plan.tracker()
        self.path_status = int(self._single_plan.status[0])
        self.path = self._single_plan.paths[0, :int(self._single_plan.lengths[0])].cpu().numpy()
        self.current_point_id = 1

    def act(self, observation, **kwargs):
        """The reference's call: ``act(observation, agent_pos=(x, y, yaw), obstacles=...)`` returns (speed, omega) as floats, unscaled; (0, 0) once
        the path is done or where there is nothing to push.  Planner and controller run on the device (env 0 of the policy's env)."""
        import torch
        agent_pos = kwargs.get('agent_pos', [0, 0, np.pi / 2])
        if self.path is None:
            self.plan_path(agent_pos, observation, kwargs.get('obstacles', None))
        if len(self.path) == 0:
            raise ValueError("PlanningBasedPolicy.act: the planner gave no path (status %d)" % self.path_status)
        if len(self.path) < 2:
            return 0.0, 0.0
        env = self.env
        E, dev = env.num_envs, env.device
        pose = torch.tensor([float(v) for v in agent_pos[:3]], dtype=torch.float64).to(dev)[None, :].expand(E, 3).contiguous()
        active = torch.zeros(E, dtype=torch.uint8, device=dev)
        active[0] = 1
        actions, diag = env.track_pushes(self._single_plan, self._single_tracker, poses=pose, active=active, config=self._single_cfg)
        self.current_point_id = int(diag[0])
        return float(actions[0, 0]), float(actions[0, 1])

    def _wipe(self):
        self.path = self.path_status = None                                  # single-env surface: numpy [n, 3]
        self._single_plan = self._single_tracker = self._single_cfg = None
        self.plan = self.tracker = self.status = None                        # batched surface, device tensors
        self._out = self._bound = None

    def reset(self):
        """The next ``act`` plans a new path (the reference's reset)."""
        self.path = self.path_status = None

    def close(self):
        if self.env is not None:
            self.env.close()
            self.env = None
