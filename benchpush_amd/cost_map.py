"""Planner cost map with the reference's CostMap surface (benchpush/common/cost_map.py:18-126), computed on the GPU from the
environment's current obstacles.

The reference planners build ``CostMap(horizon=..., ship_mass=..., **cfg.costmap)`` and call ``update(info['obs'], ship_pos_y, vs)``
every planning step (planners/lattice.py:37-38,78-79), then read ``cost_map``.  Here the map is produced by ``bp_costmap_update`` from
the device state of a ``ShipIceEnv`` / ``BatchedShipIceEnv`` -- ``info['obs']`` *is* that state -- so the polygons never visit the host.
"""
import numpy as np

MAX_COST = 1e10


class CostMap:
    def __init__(self, scale, m, n, alpha=10, ship_mass=1, horizon=None, margin=1, env=None):
        if env is None:
            raise ValueError("CostMap needs the environment whose obstacles it rasterises: CostMap(..., env=env)")
        self._b = getattr(getattr(env, "unwrapped", env), "_b", env)   # gym adapter -> its batched env
        self.scale, self.m, self.n = scale, m, n
        self.alpha, self.ship_mass, self.margin = alpha, ship_mass, margin
        self.horizon = horizon * scale if horizon else None            # cost_map.py:42
        self._horizon_m = horizon
        self.cost_maps = None
        self.cost_map = np.zeros((int(m * scale), int(n * scale)))
        self.boundary_cost()

    @property
    def shape(self):
        return self.cost_map.shape

    def boundary_cost(self):
        if not self.margin:
            return
        self.cost_map[:, :self.margin] = MAX_COST
        self.cost_map[:, -self.margin:] = MAX_COST

    def update(self, obstacles=None, ship_pos_y=0, vs=1):
        """``obstacles`` is accepted for signature compatibility; the environment's device state is what gets rasterised."""
        E = self._b.num_envs
        spy = np.broadcast_to(np.asarray(ship_pos_y, np.float64), (E,)).copy()
        self.cost_maps = self._b.cost_maps(self.scale, self.m, self.n, self.alpha, self.ship_mass, self._horizon_m, self.margin, spy, vs)
        self.cost_map = self.cost_maps[0].cpu().numpy()

    def swath_cost(self, path, ship_vertices):
        """``compute_swath_cost(cost_map, path, ship_vertices)`` of the reference (common/swath.py:114-163) for environment 0 over the map of the last
        ``update()``, computed on the device (``BatchedShipIceEnv.swath_costs``): path [n, 3] = (x, y, theta) in cells, ship_vertices [nv, 2] in cells
        (``Ship.vertices``).  Returns (swath: bool [H, W], cost: float)."""
        import torch
        if self.cost_maps is None:
            raise ValueError("CostMap.swath_cost needs a cost map: call update() first")
        b = self._b
        p = np.ascontiguousarray(np.asarray(path, np.float64).reshape(-1, 3))
        paths = torch.from_numpy(p).to(b.device)[None, None].expand(b.num_envs, 1, len(p), 3).contiguous()
        fp = torch.from_numpy(np.ascontiguousarray(np.asarray(ship_vertices, np.float64).reshape(-1, 2))).to(b.device)
        costs, swaths = b.swath_costs(paths, fp, self.cost_maps, return_swaths=True)
        return swaths[0, 0].cpu().numpy().astype(bool), float(costs[0, 0].item())
