"""ship-ice-v0 on MI355X: batched tensor environment + the reference-shaped single-env adapter.

Reference: benchpush/environments/ship_ice_nav/ship_ice_env.py (ShipIceEnv).  ``BatchedShipIceEnv`` is the native
surface (device tensors in / out, all envs stepped by one kernel launch pair); ``ShipIceEnv`` mirrors the reference
class for drop-in use by BasePolicy / BaseMetric code (same constructor, reset()/step() returns, info keys,
attributes ``cfg``, ``goal``, ``max_yaw_rate_step``, ``action_space``, ``observation_space``, ``unwrapped``).

PyTorch is used only for device memory and streams; all compute is in libbenchpush_hip.so (C ABI).
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from .. import _lib
from ..config import DotDict, default_cfg, merge_user_cfg, ship_ice_physics_params
from ..gym_shim import spaces
from ..scenario import generate_ice_field, load_experiment, pack_trials
from .batched import _AdapterBase, _BatchedBase, _ptr   # (_ptr: the other env modules and replay.py import it from here)

__all__ = ["BatchedShipIceEnv", "ShipIceEnv", "default_trials"]

_CONC_GEN = {  # synthetic generator radii per concentration (floe count ~ BASELINE.json configs)
    0.1: dict(min_r=0.40, max_r=0.58), 0.2: dict(min_r=0.40, max_r=0.58), 0.3: dict(min_r=0.40, max_r=0.58),
    0.4: dict(min_r=0.40, max_r=0.58), 0.5: dict(min_r=0.40, max_r=0.58),
}


def default_trials(concentration, num_trials, base_seed=0, goal_y=9.0):
    """Synthetic stand-in for experiments_<conc>_100_r06_d40x12.pk (missing blobs): trial i <- seed base_seed+i."""
    kw = _CONC_GEN.get(round(float(concentration), 2), dict(min_r=0.40, max_r=0.58))
    return [generate_ice_field(float(concentration), base_seed + i, goal_y=goal_y, **kw) for i in range(num_trials)]


def experiment_file(concentration, directory):
    """The reference's file name for a concentration (ship_ice_env.py:76): ice_environments/experiments_<c*100>_100_r06_d40x12.pk."""
    return os.path.join(directory, "experiments_" + str(int(concentration * 100)) + "_100_r06_d40x12.pk")


def resolve_trials(cfg, num_trials=100, base_seed=0):
    """Trials of an environment, like the reference's constructor (ship_ice_env.py:74-80): the pickled experiment file of the configured
    concentration when one is available -- looked up in ``cfg.ice_environments_dir``, ``$BENCHPUSH_ICE_DIR`` and
    ``benchpush_amd/ice_environments`` -- else the synthetic stand-in (the reference checkout ships the files as missing LFS blobs)."""
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ice_environments")
    for d in (cfg.get("ice_environments_dir", None) if hasattr(cfg, "get") else None, os.environ.get("BENCHPUSH_ICE_DIR"), here):
        if d and os.path.isfile(experiment_file(cfg.concentration, d)):
            exp = load_experiment(experiment_file(cfg.concentration, d), cfg.concentration)
            return [exp[k] for k in sorted(exp)]
    return default_trials(cfg.concentration, num_trials, base_seed, goal_y=cfg.goal_y)


class LatticeResult:
    """Device tensors of ``BatchedShipIceEnv.lattice_search``: status, g, expanded, n_nodes [E]; nodes [E, N, 3]; edges [E, N]."""
    __slots__ = ("status", "g", "expanded", "n_nodes", "nodes", "edges")

    def __init__(self, status, g, expanded, n_nodes, nodes, edges):
        self.status, self.g, self.expanded, self.n_nodes, self.nodes, self.edges = status, g, expanded, n_nodes, nodes, edges


class BatchedShipIceEnv(_BatchedBase):
    """E independent ship-ice environments on one GPU.

    reset(mask) / step(actions) follow ShipIceEnv.reset / .step (ship_ice_env.py:223-355) for every env at once.
    Trial selection generalises ``episode_idx % len(experiment)`` (:188) to ``(global_env_id + episode_idx) % T``.
    """

    render_task = "ship_ice"

    def __init__(self, num_envs, cfg=None, trials=None, device="cuda:0", env_id_offset=0, num_trials=100, base_seed=0):
        self._open(num_envs, device, env_id_offset)
        self.cfg = merge_user_cfg(default_cfg("ship_ice"), cfg)
        assert self.cfg.concentration in [0.1, 0.2, 0.3, 0.4, 0.5]  # ship_ice_env.py:75
        self.params = ship_ice_physics_params(self.cfg)
        self.goal = (0, self.cfg.goal_y)
        self.max_yaw_rate_step = (math.pi / 2) / 7
        if trials is None:
            trials = resolve_trials(self.cfg, num_trials, base_seed)
        if self.cfg.low_dim_state:  # ship_ice_env.py:190-191 pins one trial
            trials = [trials[self.cfg.fixed_trial_idx]]
        self.trials = trials
        self._create(self.L.bp_create, _lib.make_config(self.params, self.cfg.ship.vertices, self.cfg.ship.head, self.cfg.ship.tail))
        pk = pack_trials(trials, max_verts=_lib.MAXV)
        T, F, V = pk["verts"].shape[:3]
        _lib.check(self.L, self.h, self.L.bp_load_scenarios(
            self.h, T, F, V, pk["verts"].ctypes.data_as(C.c_void_p), pk["counts"].ctypes.data_as(C.c_void_p),
            pk["centres"].ctypes.data_as(C.c_void_p), pk["starts"].ctypes.data_as(C.c_void_p),
            pk["nfloes"].ctypes.data_as(C.c_void_p)), "bp_load_scenarios")
        self._alloc_io()

    def observe_global(self, mask=None):
        """Planner observation (cfg.egocentric_obs: false): uint8 [E, 2, map_h/0.2, map_w/0.2]."""
        gh, gw = int(self.cfg.occ.map_height / 0.2), int(self.cfg.occ.map_width / 0.2)
        if getattr(self, "_gobs", None) is None:
            self._gobs = torch.zeros((self.num_envs, 2, gh, gw), dtype=torch.uint8, device=self.device)
        _lib.check(self.L, self.h, self.L.bp_observe_global(self.h, _ptr(self._mask(mask)), _ptr(self._gobs), self._stream()), "bp_observe_global")
        return self._gobs

    def cost_maps(self, scale, m, n, alpha=10.0, ship_mass=1.0, horizon=None, margin=1, ship_pos_y=None, vs=1.0, out=None):
        """Planner cost maps of every env (CostMap(...).update(info['obs'], ship_pos_y, vs).cost_map, common/cost_map.py:27-126):
        float64 [E, int(m*scale), int(n*scale)] on the device.  ship_pos_y: [E] tensor in cost-map units, or None for 0."""
        H, W = int(m * scale), int(n * scale)
        if out is None:
            out = torch.empty((self.num_envs, H, W), dtype=torch.float64, device=self.device)
        cfg = _lib.BpCostmapConfig(scale=float(scale), m=int(m), n=int(n), alpha=float(alpha), ship_mass=float(ship_mass),
                                   horizon=float(horizon or 0.0), margin=int(margin), pad_=0)
        spy = None
        if ship_pos_y is not None:
            spy = torch.as_tensor(ship_pos_y, dtype=torch.float64).to(self.device).reshape(self.num_envs).contiguous()
        _lib.check(self.L, self.h, self.L.bp_costmap_update(self.h, C.byref(cfg), _ptr(spy) if spy is not None else None, float(vs),
                                                            _ptr(out), self._stream()), "bp_costmap_update")
        return out

    def swath_costs(self, paths, footprint, cost_maps, lengths=None, rows=None, outside="clip", return_swaths=False, out=None):
        """Cost of K candidate paths per env over the cost maps, on the device (bp_swath_cost): the sum of `cost_maps` over the cells that the ship
        footprint sweeps along each path -- the reference's ``compute_swath_cost`` (common/swath.py:114-163), the sum inside ``AStar.get_swath_cost``
        and the two sums of ``Path.update`` -- with no copy to the host.  All arguments are contiguous device tensors:

        paths      float64 [E, K, P, 3]: samples (x, y, theta) in cost-map cells / radians
        footprint  float64 [nv, 2] in cells, 3 <= nv <= 20, any simple polygon (``planning.ship_footprint``)
        cost_maps  float64 [E, H, W] (``cost_maps()``), or one [H, W] map shared by all envs; H * ceil(W / 64) <= 4096
        lengths    int32 [E, K] or None: the samples of each candidate that count (clamped to [0, P])
        rows       int32 [E, 2] or [E, K, 2] or None: the swath is restricted to rows lo <= r < hi (each clamped to [0, H])
        outside    "clip": cells off the map are ignored, like compute_swath_cost.  "reject": +inf for a candidate with any footprint vertex of a counted
                   sample outside [0, W-1] x [0, H-1] -- what A*'s ``return np.inf`` is for, stated on the vertices so that it is exact; it is stricter than
                   the reference's pixel rule by less than one cell.
        out        None, a float64 [E, K] tensor for the costs, or (costs, swaths) with swaths uint8 [E, K, H, W]

        Returns costs [E, K], or (costs, swaths) with return_swaths (0 / 1 masks, row window applied).  A candidate with a non-finite counted sample costs
        NaN and has an empty mask; a finite sample beyond 1e15 lies off the map.  The sum runs over a row's columns, then over the rows, in ascending
        order: equal inputs give equal bits.  Raises ValueError, before any launch, for a wrong dtype, device, shape or a non-contiguous tensor; BpError
        for what the library refuses (footprint size, grid above the LDS limit, not a ship-ice env).  Touches no environment state."""
        E = self.num_envs

        need = self._need("swath_costs")
        if outside not in ("clip", "reject"):
            raise ValueError("swath_costs: outside must be 'clip' or 'reject'")
        need(paths, "paths", torch.float64, [(E, None, None, 3)])
        K, P = int(paths.shape[1]), int(paths.shape[2])
        need(footprint, "footprint", torch.float64, [(None, 2)])
        need(cost_maps, "cost_maps", torch.float64, [(E, None, None), (None, None)])
        H, W = int(cost_maps.shape[-2]), int(cost_maps.shape[-1])
        if lengths is not None:
            need(lengths, "lengths", torch.int32, [(E, K)])
        if rows is not None:
            need(rows, "rows", torch.int32, [(E, 2), (E, K, 2)])
            if rows.dim() == 2:
                rows = rows[:, None, :].expand(E, K, 2).contiguous()
        costs, swaths = out if isinstance(out, (tuple, list)) else (out, None)
        if costs is not None:
            need(costs, "out", torch.float64, [(E, K)])
        if swaths is not None:
            need(swaths, "out[1]", torch.uint8, [(E, K, H, W)])
        if min(K, P, H, W) <= 0:
            raise ValueError("swath_costs: empty paths or cost maps")
        if costs is None:
            costs = torch.empty((E, K), dtype=torch.float64, device=self.device)
        if return_swaths and swaths is None:
            swaths = torch.empty((E, K, H, W), dtype=torch.uint8, device=self.device)
        cfg = _lib.BpSwathConfig(H=H, W=W, K=K, P=P, nv=int(footprint.shape[0]), outside=_lib.SWATH_REJECT if outside == "reject" else _lib.SWATH_CLIP,
                                 map_stride=H * W if cost_maps.dim() == 3 else 0)
        _lib.check(self.L, self.h, self.L.bp_swath_cost(self.h, C.byref(cfg), _ptr(cost_maps), _ptr(paths), _ptr(lengths), _ptr(rows), _ptr(footprint),
                                                        _ptr(costs), _ptr(swaths) if return_swaths else None, self._stream()), "bp_swath_cost")
        return (costs, swaths) if return_swaths else costs

    def lattice_search(self, cost_maps, starts, goal_y, prims, masks, weight=1.0, h_baseline=False, margin=None, active=None, max_expansions=8192,
                       max_path_nodes=128, node_capacity=None, queue_capacity=None, out=None):
        """Lattice A* of every env over the cost maps, on the device (bp_lattice_search): ``AStar.search`` of the reference's planning baseline for the
        goal line y >= goal_y, one wavefront per env, no host synchronisation.  DESIGN.md "Lattice search" states the semantics.

        cost_maps  float64 [E, H, W] (``cost_maps()``) or one shared [H, W] map
        starts     float64 [E, 3] = (x, y, theta) in cells / radians; goal_y float64 [E] in cells
        prims      ``planning.LatticePrimitives``; masks int64 [E, nh * ne_max, S] (``planning.lattice_swath_masks``) or one shared [nh * ne_max, S]
        weight     f = g + weight * h; h_baseline: h = max(0, goal_y - y) instead of the Dubins heuristic; margin: rows below the start and above the goal
                   that the window keeps (None: int(5 * prims.scale), the reference's default)
        active     bool / uint8 [E] or None: envs with False are SKIPPED and only their status is written
        max_expansions, max_path_nodes, node_capacity (None: 2 * max_expansions), queue_capacity (None: 2 * max_expansions): the caps; exceeding one
                   gives status CAP.  profiles/lattice/README.md records what the shipped configuration needs.
        out        None or a LatticeResult of a previous call with the same shapes, to be overwritten

        Returns a LatticeResult of device tensors: status int32 [E] (LATTICE_FOUND 0, NO_PATH 1, CAP 2, SKIPPED 3), g float64 [E], expanded int32 [E],
        n_nodes int32 [E], nodes float64 [E, max_path_nodes, 3] = (X, Y, world heading) start to goal, edges int32 [E, max_path_nodes] (base * ne_max + k,
        -1 for the start).  Only rows 0 .. n_nodes-1 of found envs are written.  The workspace is cached on the env.  Raises ValueError, before any launch,
        for a wrong dtype, device, shape or a non-contiguous tensor; BpError for what the library refuses.  Touches no environment state."""
        E = self.num_envs

        need = self._need("lattice_search")
        nh, nb, nem = int(prims.num_headings), int(prims.num_base_h), int(prims.ne_max)
        need(cost_maps, "cost_maps", torch.float64, [(E, None, None), (None, None)])
        H, W = int(cost_maps.shape[-2]), int(cost_maps.shape[-1])
        need(starts, "starts", torch.float64, [(E, 3)])
        need(goal_y, "goal_y", torch.float64, [(E,)])
        need(masks, "masks", torch.int64, [(E, nh * nem, None), (nh * nem, None)])
        S = int(masks.shape[-1])
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), [(E,)])
        if min(H, W, S) <= 0:
            raise ValueError("lattice_search: empty cost maps or masks")
        node_capacity = 2 * int(max_expansions) if node_capacity is None else int(node_capacity)
        queue_capacity = 2 * int(max_expansions) if queue_capacity is None else int(queue_capacity)
        N = int(max_path_nodes)
        if out is None:
            if N <= 0:
                raise ValueError("lattice_search: max_path_nodes must be positive")
            out = LatticeResult(torch.empty(E, dtype=torch.int32, device=self.device), torch.empty(E, dtype=torch.float64, device=self.device),
                                torch.empty(E, dtype=torch.int32, device=self.device), torch.empty(E, dtype=torch.int32, device=self.device),
                                torch.zeros((E, N, 3), dtype=torch.float64, device=self.device),
                                torch.full((E, N), -1, dtype=torch.int32, device=self.device))
        else:
            need(out.status, "out.status", torch.int32, [(E,)])
            need(out.g, "out.g", torch.float64, [(E,)])
            need(out.expanded, "out.expanded", torch.int32, [(E,)])
            need(out.n_nodes, "out.n_nodes", torch.int32, [(E,)])
            need(out.nodes, "out.nodes", torch.float64, [(E, N, 3)])
            need(out.edges, "out.edges", torch.int32, [(E, N)])
        cfg = _lib.BpLatticeConfig(H=H, W=W, S=S, nh=nh, nb=nb, ne_max=nem, den=int(prims.den), margin=int(5 * prims.scale) if margin is None else int(margin),
                                   h_baseline=int(bool(h_baseline)), max_expansions=int(max_expansions), node_capacity=node_capacity,
                                   queue_capacity=queue_capacity, max_path_nodes=N, pad_=0, map_stride=H * W if cost_maps.dim() == 3 else 0,
                                   mask_stride=nh * nem * S if masks.dim() == 3 else 0, unit=float(prims.scale), weight=float(weight),
                                   turning_radius=float(prims.turning_radius))
        nbytes = int(self.L.bp_lattice_workspace_bytes(C.byref(cfg), E))
        ws = getattr(self, "_lattice_ws", None)
        if nbytes > 0 and (ws is None or ws.numel() < nbytes):
            ws = self._lattice_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        e, hd, ln, cnt = prims.tables()
        e, hd, ln, cnt = (np.ascontiguousarray(e, np.float64), np.ascontiguousarray(hd, np.int32), np.ascontiguousarray(ln, np.float64),
                          np.ascontiguousarray(cnt, np.int32))
        hp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        _lib.check(self.L, self.h, self.L.bp_lattice_search(
            self.h, C.byref(cfg), _ptr(cost_maps), _ptr(starts), _ptr(goal_y), _ptr(active) if active is not None else None, hp(e), hp(hd), hp(ln), hp(cnt),
            _ptr(masks), _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0, _ptr(out.status), _ptr(out.g), _ptr(out.expanded),
            _ptr(out.n_nodes), _ptr(out.nodes), _ptr(out.edges), self._stream()), "bp_lattice_search")
        return out

    def track_paths(self, paths, state, lengths=None, poses=None, active=None, config=None, out=None):
        """The tracking controller of the reference's planning-based policy (``PlanningBasedPolicy.act``, policy.py:61-172) for every env in one launch
        (bp_track_path), no host synchronisation.  DESIGN.md "Path tracking" states the semantics.  All tensors are contiguous and on the env's device:

        paths    float64 [E, P, 3] = (x, y, theta), or one [P, 3] path shared by all envs, in the units of the poses (the reference: metres)
        state    ``planning.TrackerState`` or its float64 [E, 4] tensor: the integrators, read and written
        lengths  int32 [E] or None (all P): the samples that count
        poses    float64 [E, 3] or None: the ships' (x, y, yaw); None takes info[:, :3]
        active   bool / uint8 [E] or None: envs with False have nothing written
        config   ``planning.TrackerConfig`` or None (the reference's values); its action_scale defaults to max_yaw_rate_step
        out      None or (actions float64 [E, 2], ct_err float64 [E], diag int32 [E, 4]) to be overwritten

        Returns (actions, ct_err, diag): actions[:, 0] is the yaw action that ``step`` takes, actions[:, 1] the surge command (which ship-ice-v0 has no
        use for); diag = (i_near, branch, forward index, backward index) with branch 0 none, 1 gentle fixed-rate turn, 2 PID, 3 near.  An env that is not
        active or whose length is below 1 has nothing written (fresh outputs are zero), its state row included; a non-finite pose or counted sample
        gives NaN actions, branch 0 and an untouched state row.  Raises ValueError, before any launch, for a wrong dtype, device, shape or a
        non-contiguous tensor; BpError for what the library refuses.  Touches no environment state."""
        from ..planning import TrackerConfig
        E = self.num_envs

        need = self._need("track_paths")
        need(paths, "paths", torch.float64, [(E, None, 3), (None, 3)])
        P = int(paths.shape[-2])
        st = getattr(state, "state", state)
        need(st, "state", torch.float64, [(E, 4)])
        if lengths is not None:
            need(lengths, "lengths", torch.int32, [(E,)])
        if poses is None:
            poses = self.info[:, :3].contiguous()
        need(poses, "poses", torch.float64, [(E, 3)])
        if active is not None:
            need(active, "active", (torch.bool, torch.uint8), [(E,)])
        actions, ct_err, diag = out if out is not None else (None, None, None)
        if out is not None:
            need(actions, "out[0]", torch.float64, [(E, 2)])
            need(ct_err, "out[1]", torch.float64, [(E,)])
            need(diag, "out[2]", torch.int32, [(E, 4)])
        else:
            actions = torch.zeros((E, 2), dtype=torch.float64, device=self.device)
            ct_err = torch.zeros(E, dtype=torch.float64, device=self.device)
            diag = torch.zeros((E, 4), dtype=torch.int32, device=self.device)
        config = config or TrackerConfig()
        cfg = _lib.BpTrackConfig(P=P, pad_=0, action_scale=self.max_yaw_rate_step if config.action_scale is None else config.action_scale,
                                 **config.as_dict())
        _lib.check(self.L, self.h, self.L.bp_track_path(self.h, C.byref(cfg), _ptr(paths), 3 * P if paths.dim() == 3 else 0, _ptr(lengths), _ptr(poses),
                                                        _ptr(active), _ptr(st), _ptr(actions), _ptr(ct_err), _ptr(diag), self._stream()),
                   "bp_track_path")
        return actions, ct_err, diag

    def start_uniform(self, env, episode):
        """The uniform of the counter RNG that places env's ship in `episode` when cfg.random_start is set (bp_start_uniform)."""
        return float(self.L.bp_start_uniform(int(self.params["start_seed"]), int(self.env_id_offset) + int(env), int(episode)))

    def sched_warnings(self):
        """(watchdog events, envs finished by the completion launch) of the step scheduler since load: (0, 0) unless a scheduler fault occurred."""
        out = np.zeros(2, np.int32)
        _lib.check(self.L, self.h, self.L.bp_sched_warnings(self.h, out.ctypes.data_as(C.c_void_p)), "bp_sched_warnings")
        return int(out[0]), int(out[1])

    def pair_stats(self):
        """Two environments per wavefront (bp_get_pair_stats): dict of the pairing mode and limits, and the cumulative counters since load."""
        out = np.zeros(16, np.int32)
        _lib.check(self.L, self.h, self.L.bp_get_pair_stats(self.h, out.ctypes.data_as(C.c_void_p)), "bp_get_pair_stats")
        keys = ["mode", "solo_first", "max_arbiter_lanes", "max_velocity_slots", "max_moving", "max_active", "max_warm_x_colours", "max_work_rate",
                "paired_first_tasks", "paired_tasks_from_queues", "envs_finished_in_a_pair", "envs_left_as_heavy", "heavy_envs_queued", "light_envs_queued"]
        return dict(zip(keys, out.tolist()))

    def sched_chunk(self):
        """Sub-steps per chunk of the preemptive step scheduler, 0 = one wavefront per env for the whole step."""
        return int(self.L.bp_sched_chunk(self.h))

    def set_cost_hint(self, costs):
        """Dispatch-order hint for the next step (uint32 per env, larger = earlier); by default the previous step's wave cycles."""
        c = np.ascontiguousarray(costs, dtype=np.uint32)
        assert c.shape == (self.num_envs,)
        _lib.check(self.L, self.h, self.L.bp_set_step_cost_hint(self.h, c.ctypes.data_as(C.c_void_p)), "bp_set_step_cost_hint")


class ShipIceEnv(_AdapterBase):
    """Reference-shaped single environment (E = 1) on the GPU path.

    Same surface as the reference ShipIceEnv (ship_ice_env.py:33-355): ``reset(seed, options) -> (obs, info)``,
    ``step(action) -> (obs, reward, terminated, False, info)`` with numpy observations and the reference's info keys.
    ``cfg.random_start`` (:201-203) re-draws the start x of every episode -- from a counter RNG keyed (start_seed, env, episode)
    instead of python's global ``random`` (``BatchedShipIceEnv.start_uniform`` reproduces the draw) -- and every reset then runs
    the 1000 settle sub-steps with the ship at that pose, like the reference.
    """

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 4}

    def __init__(self, cfg=None, trials=None, device="cuda:0", num_trials=100, base_seed=0):
        super().__init__()
        self._b = BatchedShipIceEnv(1, cfg=cfg, trials=trials, device=device, num_trials=num_trials, base_seed=base_seed)
        self.cfg = self._b.cfg
        self.local_window_v_shift = 2
        self.beta = 30
        self.directional_reward_scale = 1.0
        self.episode_idx = None
        self.goal = (0, self.cfg.goal_y)
        self.path = None
        self.low_dim_state = self.cfg.low_dim_state
        self.max_yaw_rate_step = (np.pi / 2) / 7
        self.action_space = spaces.Box(low=-1, high=1, dtype=np.float32)
        self.env_max_trial = len(self._b.trials)
        if self.low_dim_state:
            n = len(self._b.trials[0]["obstacles"])
            self.observation_space = spaces.Box(low=-10, high=30, shape=(n * 2,), dtype=np.float64)
        else:
            if self.cfg.egocentric_obs:
                obs_shape = self._b.obs_shape
            else:  # planner observation (ship_ice_env.py:96-99)
                obs_shape = (2, int(self.cfg.occ.map_height / 0.2), int(self.cfg.occ.map_width / 0.2))
            self.observation_space = spaces.Box(low=0, high=255, shape=obs_shape, dtype=np.uint8)
        self.yaw_lim = (0, np.pi)
        self.boundary_violation_limit = 0.0
        self.total_work = [0, []]
        self.t = 0

    def _polys(self):
        verts, cnt = self._b.world_polys()
        verts = verts[0].cpu().numpy()
        cnt = cnt[0].cpu().numpy()
        nb = int(self._b.num_bodies()[0])
        return [verts[i, : cnt[i]].copy() for i in range(1, nb)]

    def _observation(self, obstacles):
        if self.low_dim_state:
            nb = int(self._b.num_bodies()[0])
            return self._b.low_dim_obs()[0, : nb - 1].reshape(-1).cpu().numpy()
        if not self.cfg.egocentric_obs:
            return self._b.observe_global()[0].cpu().numpy()
        return self._b.obs[0].cpu().numpy()

    def reset(self, seed=None, options=None):
        self._begin_episode()
        self.total_work = [0, []]
        it = self._b.info[0].cpu().numpy()
        obstacles = self._polys()
        self.obstacles = obstacles
        info = {"state": self._state3(it), "total_work": self.total_work[0], "obs": obstacles}
        return self._observation(obstacles), info

    def step(self, action):
        self.t += 1
        # the action keeps the caller's precision, like `action * self.max_yaw_rate_step` in the reference (ship_ice_env.py:265)
        a = torch.tensor([float(np.asarray(action, dtype=np.float64).reshape(-1)[0])], dtype=torch.float64)
        self._b.step(a)
        it = self._b.info[0].cpu().numpy()
        reward = float(self._b.reward[0].item())
        terminated = bool(self._b.terminated[0].item())
        obstacles = self._polys()
        self.obstacles = obstacles
        work = float(it[4])
        self.total_work[0] = float(it[3])
        self.total_work[1].append(work)
        info = {"state": self._state3(it), "total_work": self.total_work[0], "collision reward": float(it[5]), "scaled collision reward": float(it[6]),
                "dist reward": float(it[7]), "trial_success": bool(it[8]), "obs": obstacles}
        if self.cfg.log_obs:
            self.log_observation()
        return self._observation(obstacles), reward, terminated, False, info

    def log_observation(self):
        """`cfg.log_obs` (ship_ice_env.py:352-353, 412-479): one PNG per observation channel under <cfg.output_dir>/t<episode_idx>/, named like the reference's
        files -- egocentric: <t>_con (occupancy), _orientation, _edt, _footprint; planner mode: <t>_con (5x5 block-mean occupancy), _footprint (obs_log.py)."""
        from ..obs_log import dump_channels
        if self.cfg.egocentric_obs:
            o = self._b.obs[0].cpu().numpy()           # channels [footprint, goal-line distance, orientation, occupancy] (ship_ice_env.py:392)
            ch = {"con": o[3], "orientation": o[2], "edt": o[1], "footprint": o[0]}
        else:
            o = self._b.observe_global()[0].cpu().numpy()   # [occupancy, footprint] (ship_ice_env.py:405)
            ch = {"con": o[0], "footprint": o[1]}
        return dump_channels(self.cfg.output_dir, self.episode_idx, self.t, ch)

    _STATE_FIELDS = ("t", "total_work", "episode_idx", "path", "obstacles")

    def update_path(self, new_path):
        self.path = new_path

    def render(self, mode="human", close=False):
        """rgb_array: the frame of this env with the path of update_path (numpy [H, W, 3]; benchpush_amd/render.py).  human: no window; with
        cfg.render_snapshot every call writes <output_dir>/t<episode_idx>/<t>.png (ship_ice_env.py:489-491), otherwise warns once.  Returns None."""
        from ..render import adapter_render, snapshot_path
        snap = snapshot_path(self.cfg, self.episode_idx, self.t) if mode == "human" and self.cfg.get("render_snapshot", False) else None
        return adapter_render(self, mode, self.path, snap)
