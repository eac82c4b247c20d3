"""PlanningBasedPolicy: the reference's planning-based ship-ice baseline (benchpush/baselines/ship_ice_nav/planning_based/policy.py:11-208) on the
batched env.  A planner gives every env a path -- 'straight': ``planning.straight_paths``; 'lattice': ``planning.BatchedLatticePlanner`` -- and the
reference's tracking controller follows it, one kernel launch per step for all envs (``BatchedShipIceEnv.track_paths``).  DESIGN.md "Path tracking" lists
where this deviates from the reference: the yaw element of the (yaw, surge) pair is what the env is given; paths are planned at every episode start and
the controller's integrators are cleared there.  How well this steers has not been measured.
"""
from typing import List, Tuple

import numpy as np

from ...base_class import BasePolicy

ALG_NAMES = {"lattice": "Lattice Planning", "straight": "Straight Planning", "predictive": "Predictive Planning"}


class PlanningBasedPolicy(BasePolicy):
    """planner_type   'straight' or 'lattice' ('predictive' raises NotImplementedError: its network weights are not in the reference tree)
    cfg            the env's configuration (dict / DotDict / None), as for ``BatchedShipIceEnv``
    planner_config 'lattice': a dict with the control set as data -- ``edges`` and ``turning_radius`` (in lattice units) as
                   ``planning.LatticePrimitives`` takes them, or a ready ``prims`` -- and optionally ``scale`` (5), ``padding`` (0.25), ``horizon`` (30),
                   ``step_size`` (0.1), ``search`` (keyword arguments of ``lattice_search``); 'straight': optionally ``dy`` (10)
    num_envs       envs that ``evaluate`` runs side by side
    tracker_config ``planning.TrackerConfig`` or None (the reference's values)
    replan_every   'lattice': every n-th step of ``act_batch`` plans again and keeps the new path where ``Path.update``'s comparison prefers it (0: never)
    env_kwargs     further keyword arguments of ``BatchedShipIceEnv`` (trials, num_trials, base_seed, device)"""

    def __init__(self, planner_type, cfg=None, planner_config=None, num_envs=1, tracker_config=None, replan_every=0, max_episode_steps=300,
                 **env_kwargs) -> None:
        super().__init__()
        if planner_type not in ALG_NAMES:
            raise ValueError("PlanningBasedPolicy: no planner called %r ('straight' and 'lattice' are available)" % (planner_type,))
        if planner_type == "predictive":
            raise NotImplementedError("the predictive planner needs network weights that the reference tree does not hold")
        self.planner_type = planner_type
        self.cfg, self.planner_config = cfg, dict(planner_config or {})
        self.num_envs, self.tracker_config, self.replan_every = int(num_envs), tracker_config, int(replan_every)
        self.max_episode_steps, self.env_kwargs = int(max_episode_steps), env_kwargs
        self.env = self._prims = None
        self.reset()

    # -- the env and the planner ---------------------------------------------------------------------------
    def _ensure_env(self):
        if self.env is None:
            from ....envs.ship_ice import BatchedShipIceEnv
            self.env = BatchedShipIceEnv(self.num_envs, cfg=self.cfg, **self.env_kwargs)
            self.env.reset()
        return self.env

    def _lattice(self, env):
        if self.planner is None or self.planner.env is not env:
            from ....planning import BatchedLatticePlanner, LatticePrimitives
            pc = self.planner_config
            prims = pc.get("prims") or self._prims
            scale = pc.get("scale", 5)
            if prims is None:
                if "edges" not in pc or "turning_radius" not in pc:
                    raise ValueError("PlanningBasedPolicy('lattice'): planner_config must hold the control set (edges, turning_radius) or prims")
                prims = self._prims = LatticePrimitives(pc["edges"], 4 * len(pc["edges"]), scale, pc["turning_radius"], pc.get("step_size", 0.1))
            self.planner = BatchedLatticePlanner(env, prims, scale, pc.get("padding", 0.25), pc.get("horizon", 30), search_kwargs=pc.get("search"))
        return self.planner

    def _plan_batch(self, env, fresh, update=False):
        """Paths in metres for the envs of `fresh` (bool [E] or None: all); with `update` the others compare as ``Path.update`` does ('lattice')."""
        import torch
        if self.planner_type == "lattice":
            pl = self._lattice(env)
            pl.plan(fresh=fresh, update=update)
            self.paths, self.lengths = pl.paths_metres(), pl.lengths.contiguous()
            return
        from ....planning import straight_paths
        dy = self.planner_config.get("dy", 10)
        goal_y = float(env.cfg.goal_y)
        max_len = int(np.ceil((goal_y + dy * 0.5) / dy)) + 1      # a start at y >= -dy needs no more samples
        new, new_len = straight_paths(env.info[:, :3], goal_y, dy, max_len=max_len)
        if self.paths is None or fresh is None:
            self.paths, self.lengths = new, new_len
        else:
            self.paths = torch.where(fresh[:, None, None], new, self.paths)
            self.lengths = torch.where(fresh, new_len, self.lengths)

    # -- the batched surface -------------------------------------------------------------------------------
    def act_batch(self, env=None, fresh=None):
        """Yaw actions [E] (device, float64) for all envs of `env` (None: the policy's own).  fresh: bool / uint8 [E] of the envs that have just started
        an episode -- they get a new path and a cleared controller; None on the first call means all, later none.  No host synchronisation."""
        import torch
        from ....planning import TrackerState
        env = env or self._ensure_env()
        if self.tracker is None or self._bound is not env:      # the paths and integrators belong to one env object
            self.reset()
            self.tracker, self._bound, fresh = TrackerState(env.num_envs, env.device), env, None
        first = self.paths is None
        if fresh is not None:
            fresh = fresh.to(device=env.device, dtype=torch.bool)
            self.tracker.reset(fresh)
        replan = self.planner_type == "lattice" and self.replan_every > 0 and self._calls > 0 and self._calls % self.replan_every == 0
        if first or fresh is not None or replan:
            self._plan_batch(env, None if first else fresh, update=replan)
        self._calls += 1
        self._out = env.track_paths(self.paths, self.tracker, lengths=self.lengths, config=self.tracker_config, out=self._out)
        actions = self._out[0]
        return torch.where(self.lengths > 0, actions[:, 0], torch.zeros_like(actions[:, 0]))   # an env without a path goes straight on

    def evaluate(self, num_eps: int, model_eps: str = "latest") -> Tuple[List[float], List[float], List[float], str]:
        """Run `num_envs` envs side by side, every finished env starting its next episode at once, until `num_eps` episodes have finished.  Returns
        (efficiency scores, effort scores, rewards, algorithm name) of the finished episodes, from the on-device episode metrics."""
        import torch
        alg_name = ALG_NAMES[self.planner_type]
        env = self._ensure_env()
        env.reset()
        self.reset()
        E = env.num_envs
        age = torch.zeros(E, dtype=torch.int64, device=env.device)
        eff, effort, rewards = [], [], []
        fresh = None
        while len(eff) < num_eps:
            _, _, term, trunc, _ = env.step(self.act_batch(env, fresh))
            age += 1
            done = term.bool() | trunc.bool() | (age >= self.max_episode_steps)     # TimeLimit of the registered id
            fresh = None
            if bool(done.any()):
                env.reset(done)                       # a reset of a running episode closes it as truncated
                rows, _ = env.episode_metrics()
                for r in rows[done].cpu().numpy():
                    eff.append(float(r[0])), effort.append(float(r[1])), rewards.append(float(r[2]))
                age = torch.where(done, torch.zeros_like(age), age)
                fresh = done
        env.check_errors()
        return eff, effort, rewards, alg_name

    # -- the reference's single-env surface ------------------------------------------------------------------
    def straight_planner(self, ship_pose, goal, dy=10):
        """``planning.straight_paths`` for one pose: numpy [n, 3], the samples (x, y + i * dy, theta) up to goal[1]."""
        from ....planning import straight_paths
        paths, lengths = straight_paths([[float(v) for v in ship_pose]], float(goal[1]), dy)
        return paths[0, :int(lengths[0])].numpy()

    def plan_path(self, ship_pos, goal, observation, conc, obstacles=None):
        """Sets ``path`` (numpy [n, 3] in metres).  'lattice' plans on the device from the state of env 0 of the policy's env, whose floes it knows:
        `obstacles` and `observation` are not read, and a `ship_pos` that is not that env's pose (to the 0.01 that ``info['state']`` is rounded to) is
        refused with ValueError -- the path would belong to another ship."""
        if self.planner_type == "straight":
            self.path = self.straight_planner(ship_pos, goal, self.planner_config.get("dy", 10))
            return
        env = self._ensure_env()
        here = env.info[0, :3].cpu().numpy()
        if not np.allclose(np.asarray([float(v) for v in ship_pos]), here, rtol=0.0, atol=0.006):
            raise ValueError("PlanningBasedPolicy.plan_path('lattice'): ship_pos %s is not the pose %s of env 0 of the policy's env, from whose state "
                             "the path is planned" % (tuple(ship_pos), tuple(here.tolist())))
        pl = self._lattice(env)
        pl.plan(fresh=None if pl.path is None else _ones(env), update=False)
        n = int(pl.lengths[0])
        self.path = pl.paths_metres()[0, :n].cpu().numpy()

    def act(self, observation, **kwargs):
        """The reference's call: ``act(observation, ship_pos=(x, y, yaw), goal=(gx, gy), action_scale=..., dt=0.005, conc=..., obstacles=...)`` returns
        the pair (yaw action, surge command) as floats.  The controller runs on the device (env 0 of the policy's env)."""
        import torch
        from ....planning import TrackerConfig, TrackerState
        env = self._ensure_env()
        if self.path is None:
            self.plan_path(kwargs["ship_pos"], kwargs["goal"], observation, kwargs.get("conc"), kwargs.get("obstacles"))
        if len(self.path) == 0:
            raise ValueError("PlanningBasedPolicy.act: the planner found no path")
        if self._single is None:
            self._single = TrackerState(env.num_envs, env.device)
        base = self.tracker_config or TrackerConfig()
        cfg = TrackerConfig(**dict(base.as_dict(), dt=kwargs.get("dt", base.dt)), action_scale=kwargs["action_scale"])
        E, dev = env.num_envs, env.device
        pose = torch.tensor([float(v) for v in kwargs["ship_pos"]], dtype=torch.float64).to(dev)[None, :].expand(E, 3).contiguous()
        active = torch.zeros(E, dtype=torch.uint8, device=dev)
        active[0] = 1
        path = torch.from_numpy(np.ascontiguousarray(self.path, np.float64)).to(dev)
        actions, _, _ = env.track_paths(path, self._single, poses=pose, active=active, config=cfg)
        yaw, surge = actions[0].cpu().tolist()
        return yaw, surge

    def reset(self):
        """A new path is planned at the next call and the controllers start afresh."""
        self.path = None                     # single-env surface: numpy [n, 3] in metres
        self._single = None                  # single-env surface: TrackerState
        self.paths = self.lengths = self.tracker = None   # batched surface: device paths in metres [E, P, 3], lengths [E], TrackerState
        self.planner = self._bound = None    # the lattice planner (it keeps paths of its own) and the env that the batched members belong to
        self._out, self._calls = None, 0

    def close(self):
        if self.env is not None:
            self.env.close()
            self.env = None


def _ones(env):
    import torch
    return torch.ones(env.num_envs, dtype=torch.bool, device=env.device)
