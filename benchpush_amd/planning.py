"""Small helpers for planners that score candidate paths on the device with ``BatchedShipIceEnv.swath_costs``.

Plain torch / numpy, not a hot path: the footprint of the reference's ``Ship`` (common/ship.py:18-20), constant-curvature candidate paths in closed
form, the replanning comparison of ``Path.update`` (common/utils/utils.py:58-89), and what the lattice A* (``BatchedShipIceEnv.lattice_search``)
takes and gives: the primitive tables (``LatticePrimitives``, common/primitives.py), the swath masks (``lattice_swath_masks``, common/swath.py:15-88) and
the sampled path of a search result (``lattice_full_paths``, ``AStar.build_path``).  ``BatchedLatticePlanner`` chains them into the planning round of
``LatticePlanner.plan``.  For ``BatchedShipIceEnv.track_paths``: the controller's tunables and integrators (``TrackerConfig``, ``TrackerState``) and the
reference's ``straight_planner`` for a batch (``straight_paths``).  For ``BatchedMazeEnv.rrt_plan``: ``RRTConfig``, ``RRTPlan``.  For
``BatchedAreaClearingEnv.gtsp_plan`` / ``track_pushes``: ``GTSPConfig``, ``GTSPPlan``, ``GTSPTrackerState`` and the boundary goal segments of the
reference's area-clearing policy (``boundary_goals``).
"""
import collections

import numpy as np
import torch

from . import dubins as _dubins

__all__ = ["ship_footprint", "arc_paths", "replan_mask", "LATTICE_SHIP_VERTICES", "LatticePrimitives", "ship_halves", "lattice_max_val",
           "lattice_swath_masks", "lattice_full_paths", "BatchedLatticePlanner", "TrackerConfig", "TrackerState", "straight_paths", "RRTConfig", "RRTPlan",
           "GTSPConfig", "GTSPPlan", "GTSPTrackerState", "boundary_goals"]

# ship.vertices of the reference's lattice planner configuration (17 vertices, some collinear); with padding 0.25 and scale 5 it is the planner's footprint
LATTICE_SHIP_VERTICES = [[1., -0.], [0.9, 0.10], [0.5, 0.25], [0.25, 0.25], [0, 0.25], [-0.25, 0.25], [-0.5, 0.25], [-0.75, 0.25], [-1., 0.25],
                         [-1., -0.25], [-0.75, -0.25], [-0.5, -0.25], [-0.25, -0.25], [0, -0.25], [0.25, -0.25], [0.5, -0.25], [0.9, -0.10]]


def ship_footprint(vertices, scale, padding=0.0):
    """``Ship(scale, vertices, padding).vertices``: every coordinate a becomes sign(a) * (|a| + padding) * scale, so a zero coordinate stays zero.
    Returns a float64 numpy array [nv, 2] in cost-map cells (ship facing +x)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 2)
    return np.sign(v) * (np.abs(v) + padding) * scale


def arc_paths(pose, curvature, length, step):
    """Constant-curvature candidate paths: pose [E, 3] = (x, y, theta) in cells / radians, curvature [K] or [E, K] in 1 / cell (positive turns left,
    towards growing theta), arc length `length` sampled every `step` cells from s = 0.  Returns [E, K, P, 3] float64 on pose's device with
    P = floor(length / step) + 1: theta = theta0 + k * s, x = x0 + (sin(theta) - sin(theta0)) / k, y = y0 - (cos(theta) - cos(theta0)) / k, and the
    straight line x0 + s * cos(theta0), y0 + s * sin(theta0) where |k| < 1e-9."""
    pose = torch.as_tensor(pose, dtype=torch.float64)
    if pose.dim() != 2 or pose.shape[1] != 3:
        raise ValueError("arc_paths: pose must be [E, 3]")
    E = pose.shape[0]
    k = torch.as_tensor(curvature, dtype=torch.float64).to(pose.device)
    if k.dim() == 1:
        k = k[None, :].expand(E, k.shape[0])
    if k.dim() != 2 or k.shape[0] != E:
        raise ValueError("arc_paths: curvature must be [K] or [E, K]")
    if not (step > 0 and length >= 0):
        raise ValueError("arc_paths: step must be positive and length non-negative")
    P = int(np.floor(length / step + 1e-9)) + 1
    s = (torch.arange(P, dtype=torch.float64, device=pose.device) * step)[None, None, :]
    x0, y0, th0 = (pose[:, i, None, None] for i in range(3))
    kk = k[:, :, None]
    straight = kk.abs() < 1e-9
    ks = torch.where(straight, torch.ones_like(kk), kk)
    th = th0 + kk * s
    x = torch.where(straight, x0 + s * torch.cos(th0), x0 + (torch.sin(th) - torch.sin(th0)) / ks)
    y = torch.where(straight, y0 + s * torch.sin(th0), y0 - (torch.cos(th) - torch.cos(th0)) / ks)
    return torch.stack([x, y, th.expand_as(x)], dim=-1).contiguous()


def replan_mask(new_cost, old_cost, threshold_cost=0.95):
    """The comparison of ``Path.update``: True where the new path's swath cost is below threshold_cost times the old path's (tensors or arrays of any
    equal shape; both costs taken over the same row window, ``swath_costs(rows=...)``)."""
    return new_cost < old_cost * threshold_cost


class LatticePrimitives:
    """The reference's ``Primitives`` (common/primitives.py) for a control set that the caller passes as data.

    edge_sets       {(0, 0, b): [(x, y, heading), ...]} or a list indexed by the base heading b, in lattice units (``Primitives.get_primitives``)
    num_headings    8 or 16; len(edge_sets) == num_headings / 4
    scale           cells per lattice unit; turning_radius in lattice units; step_size in cells between the samples of a primitive's path

    Attributes as in the reference: edge_set_dict (scaled edges), paths {((0, 0, b), edge): [3, P]}, path_lengths, num_base_h, max_prim, spacing,
    turning_radius (cells).  Beside them the tables of the C ABI: edges [nb][k] unscaled, den (sub-units per lattice unit: the smallest integer that
    makes every edge an integer), ne_max, and samples(b, k) / length(b, k)."""

    def __init__(self, edge_sets, num_headings=8, scale=1.0, turning_radius=1.0, step_size=0.25, _paths=None):
        sets = [edge_sets[(0, 0, b)] for b in range(len(edge_sets))] if isinstance(edge_sets, dict) else list(edge_sets)
        self.num_headings, self.scale, self.step_size = int(num_headings), float(scale), float(step_size)
        self.turning_radius = float(turning_radius) * self.scale
        self.num_base_h = len(sets)
        if self.num_headings not in (8, 16) or self.num_base_h * 4 != self.num_headings:
            raise ValueError("LatticePrimitives: 8 or 16 headings with num_headings / 4 edge sets")
        self.edges = [[(float(x), float(y), int(h)) for x, y, h in es] for es in sets]
        self.ne_max = max(len(es) for es in self.edges)
        self.den = next((d for d in range(1, 65) if all((x * d).is_integer() and (y * d).is_integer() for es in self.edges for x, y, _ in es)), None)
        if self.den is None:
            raise ValueError("LatticePrimitives: the edges share no sub-unit of 1/64 lattice unit or coarser")
        self.spacing = 2 * np.pi / self.num_headings
        self.edge_set_dict = {(0, 0, b): [(x * self.scale, y * self.scale, h) for x, y, h in es] for b, es in enumerate(self.edges)}
        self.paths, self.path_lengths = {}, {}
        for origin, es in self.edge_set_dict.items():
            for edge in es:
                if _paths is not None:
                    self.paths[(origin, edge)], self.path_lengths[(origin, edge)] = _paths(origin, edge)
                    continue
                # get_points_on_dubins_path(p1=origin, p2=edge, initial_heading=0, eps=1e-10)
                t0 = (origin[2] * 2 * np.pi / self.num_headings) % (2 * np.pi)
                t1 = (edge[2] * 2 * np.pi / self.num_headings) % (2 * np.pi)
                dp = _dubins.shortest_path((origin[0], origin[1], t0), (edge[0], edge[1], t1), self.turning_radius - 1e-10)
                conf, _ = dp.sample_many(self.step_size)
                self.paths[(origin, edge)] = np.asarray(conf, np.float64).T.reshape(3, -1)
                self.path_lengths[(origin, edge)] = dp.path_length()
        self.max_prim = int(round(max(self.path_lengths.values())))

    @classmethod
    def from_reference(cls, prim):
        """From any object with the reference's attributes (edge_set_dict scaled, paths, path_lengths, num_headings, scale, turning_radius scaled,
        step_size): its own paths and lengths are taken over, nothing is recomputed."""
        nb = len(prim.edge_set_dict)
        scale = float(prim.scale)
        sets = [[(x / scale, y / scale, h) for x, y, h in prim.edge_set_dict[(0, 0, b)]] for b in range(nb)]
        look = {}
        for b in range(nb):
            for k, e in enumerate(prim.edge_set_dict[(0, 0, b)]):
                look[(b, k)] = (np.asarray(prim.paths[((0, 0, b), e)], np.float64), float(prim.path_lengths[((0, 0, b), e)]))
        self = cls.__new__(cls)
        order = iter([look[(b, k)] for b in range(nb) for k in range(len(sets[b]))])
        cls.__init__(self, sets, prim.num_headings, scale, float(prim.turning_radius) / scale, prim.step_size, _paths=lambda o, e: next(order))
        return self

    def samples(self, b, k):
        return self.paths[((0, 0, b), self.edge_set_dict[(0, 0, b)][k])]

    def length(self, b, k):
        return self.path_lengths[((0, 0, b), self.edge_set_dict[(0, 0, b)][k])]

    def tables(self):
        """(edges float64 [nb, ne_max, 2] in lattice units, headings int32 [nb, ne_max], lengths float64 [nb, ne_max] in cells, counts int32 [nb])."""
        nb = self.num_base_h
        e, hd, ln, cnt = np.zeros((nb, self.ne_max, 2)), np.zeros((nb, self.ne_max), np.int32), np.zeros((nb, self.ne_max)), np.zeros(nb, np.int32)
        for b, es in enumerate(self.edges):
            cnt[b] = len(es)
            for k, (x, y, h) in enumerate(es):
                e[b, k], hd[b, k], ln[b, k] = (x, y), h, self.length(b, k)
        return e, hd, ln, cnt


def _hull(points):
    """Convex hull, counter-clockwise, collinear points dropped (monotone chain)."""
    pts = sorted(set(map(tuple, np.asarray(points, np.float64).tolist())))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])   # noqa: E731
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.asarray(lower[:-1] + upper[:-1], np.float64)


def ship_halves(footprint):
    """``Ship.split_vertices`` (common/ship.py:110-131) widened as in ``generate_swath`` (common/swath.py:33-34): the convex hulls of the footprint's
    x >= 0 and x <= 0 vertices plus (0, +-width / 2), every y grown by width / 2.  Returns (right, left) float64 [n, 2]."""
    v = np.asarray(footprint, np.float64).reshape(-1, 2)
    width = v[:, 1].max() - v[:, 1].min()
    extra = np.array([[0.0, width / 2], [0.0, -width / 2]])
    out = []
    for half in (v[v[:, 0] >= 0], v[v[:, 0] <= 0]):
        hv = _hull(np.concatenate((half, extra)))
        out.append(np.stack([hv[:, 0], np.sign(hv[:, 1]) * (np.abs(hv[:, 1]) + width / 2)], 1))
    return out[0], out[1]


def lattice_max_val(prims, footprint):
    """``AStar.max_val`` = int(max_prim + max_ship_length // 2): half the side of the swath masks, S = 2 * max_val + 1."""
    v = np.asarray(footprint, np.float64).reshape(-1, 2)
    d = np.sqrt(((v[:, None, :] - v[None, :, :]) ** 2).sum(-1)).max()
    return int(prims.max_prim + int(np.ceil(d)) // 2)


def lattice_swath_masks(env, prims, footprint, theta0):
    """The swath masks of every (heading, edge) key for every env, rasterised on the device with no host synchronisation: int64 [E, nh * ne_max, S],
    word r of key h * ne_max + k = row r of the S x S mask (bit c = column c) of edge k taken from a node of lattice heading h, the node at the centre
    cell.  The footprint is swept along the primitive's samples rotated by theta0 + q * 90 deg (q = h // nb) with ``swath_costs(return_swaths=True)``
    on a blank S x S map, then the two widened ship halves at the first sample are removed (``generate_swath``'s planning branch).  theta0: [E] tensor
    or array in radians, taken mod 2 pi.  Unlike the reference, which rotates the theta0 = 0 raster with a nearest-neighbour image rotation, the rotated
    primitive itself is rasterised (DESIGN.md "Lattice search")."""
    E, dev = env.num_envs, env.device
    nh, nb, nem = prims.num_headings, prims.num_base_h, prims.ne_max
    mv = lattice_max_val(prims, footprint)
    S = 2 * mv + 1
    if S > 64:
        raise ValueError("lattice_swath_masks: masks of %d cells per side exceed the 64 of bp_lattice_search" % S)
    K = nh * nem
    P = max(prims.samples(b, k).shape[1] for b in range(nb) for k in range(len(prims.edges[b])))
    base = np.zeros((K, P, 3))
    lens = np.zeros(K, np.int32)
    quad = np.zeros(K)
    for h in range(nh):
        b, q = h % nb, h // nb
        for k in range(len(prims.edges[b])):
            sm = prims.samples(b, k)
            base[h * nem + k, :sm.shape[1]] = sm.T
            lens[h * nem + k] = sm.shape[1]
            quad[h * nem + k] = q
    th0 = torch.remainder(torch.as_tensor(theta0, dtype=torch.float64).to(dev).reshape(E), 2 * np.pi)
    base_t = torch.from_numpy(base).to(dev)
    rot = th0[:, None] + torch.from_numpy(quad * (np.pi / 2)).to(dev)[None, :]                  # [E, K]
    c, s = torch.cos(rot)[:, :, None], torch.sin(rot)[:, :, None]
    x, y = base_t[None, :, :, 0], base_t[None, :, :, 1]
    paths = torch.stack([c * x - s * y + float(mv), s * x + c * y + float(mv),
                         torch.remainder(base_t[None, :, :, 2] + rot[:, :, None], 2 * np.pi)], dim=-1).contiguous()
    lengths = torch.from_numpy(lens).to(dev)[None, :].expand(E, K).contiguous()
    blank = torch.zeros((S, S), dtype=torch.float64, device=dev)
    fp = torch.from_numpy(np.ascontiguousarray(np.asarray(footprint, np.float64).reshape(-1, 2))).to(dev)
    _, sw = env.swath_costs(paths, fp, blank, lengths=lengths, return_swaths=True)
    first = paths[:, :, :1, :].contiguous()
    one = torch.clamp(lengths, max=1)
    for half in ship_halves(footprint):
        _, cut = env.swath_costs(first, torch.from_numpy(np.ascontiguousarray(half)).to(dev), blank, lengths=one, return_swaths=True)
        sw = sw & ~cut
    return (sw.to(torch.int64) << torch.arange(S, dtype=torch.int64, device=dev)).sum(-1)


def lattice_full_paths(prims, result, starts):
    """``AStar.build_path`` for a batch: the sampled path of every env's node path, [E, Pmax, 3] float64 plus lengths [E] int32 (0 for an env without
    a path), on the device of `result` and ready for ``swath_costs(paths[:, None], ..., lengths=lengths[:, None])``.  Primitive (b, k) that leaves node
    n is rotated by that node's world heading minus b * spacing and moved to the node; headings are taken mod 2 pi.  Pmax = (max_path_nodes - 1) *
    (samples of the longest primitive): fixed by the shapes, so nothing is read back."""
    nodes, edges, n_nodes = result.nodes, result.edges, result.n_nodes
    dev = nodes.device
    E, N = edges.shape
    nb, nem = prims.num_base_h, prims.ne_max
    Pm = max(prims.samples(b, k).shape[1] for b in range(nb) for k in range(len(prims.edges[b])))
    tab, cnt = np.zeros((nb * nem, Pm, 3)), np.zeros(nb * nem, np.int64)
    for b in range(nb):
        for k in range(len(prims.edges[b])):
            sm = prims.samples(b, k)
            tab[b * nem + k, :sm.shape[1]], cnt[b * nem + k] = sm.T, sm.shape[1]
    tab_t, cnt_t = torch.from_numpy(tab).to(dev), torch.from_numpy(cnt).to(dev)
    if N < 2:
        return torch.zeros((E, 0, 3), dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.int32, device=dev)
    seg = torch.arange(N - 1, device=dev)[None, :] < (n_nodes.to(torch.int64)[:, None] - 1)      # [E, N-1]: segment n -> n + 1 exists
    eid = torch.where(seg, edges[:, 1:].to(torch.int64), torch.zeros_like(edges[:, 1:], dtype=torch.int64)).clamp(0, nb * nem - 1)
    ns = torch.where(seg, cnt_t[eid], torch.zeros_like(eid))                                      # samples per segment
    off = torch.cumsum(ns, 1) - ns
    a = nodes[:, :-1, :]
    theta = a[:, :, 2] - (eid // nem).to(torch.float64) * prims.spacing
    c, s = torch.cos(theta)[:, :, None], torch.sin(theta)[:, :, None]
    pp = tab_t[eid]                                                                               # [E, N-1, Pm, 3]
    x = c * pp[..., 0] - s * pp[..., 1] + a[:, :, None, 0]
    y = s * pp[..., 0] + c * pp[..., 1] + a[:, :, None, 1]
    t = torch.remainder(pp[..., 2] + theta[:, :, None], 2 * np.pi)
    valid = torch.arange(Pm, device=dev)[None, None, :] < ns[:, :, None]
    Pmax = (N - 1) * Pm
    dst = torch.where(valid, off[:, :, None] + torch.arange(Pm, device=dev)[None, None, :], torch.full_like(valid, Pmax, dtype=torch.int64))
    out = torch.zeros((E, Pmax + 1, 3), dtype=torch.float64, device=dev)
    out.scatter_(1, dst.reshape(E, -1, 1).expand(E, (N - 1) * Pm, 3), torch.stack([x, y, t], -1).reshape(E, -1, 3))
    return out[:, :Pmax].contiguous(), ns.sum(1).to(torch.int32)


class BatchedLatticePlanner:
    """The planning round of the reference's ``LatticePlanner.plan`` (baselines/ship_ice_nav/planning_based/planners/lattice.py) for every env of a
    ``BatchedShipIceEnv`` at once, with no host synchronisation: cost maps -> lattice A* from each ship's pose to the horizon's goal line -> the sampled
    path of each node path -> ``Path.update``'s comparison of the new and the kept path over the same row window.

    prims    ``LatticePrimitives``: the control set is data that the caller passes
    scale, padding, horizon: cells per metre, footprint padding and receding horizon in metres (the reference's lattice_config.yaml: 5, 0.25, 30)

    ``path`` [E, Pmax, 3] and ``lengths`` [E] hold the kept paths in cost-map cells (None before the first round); ``status`` the last search's status and
    ``found`` the number of searches that found a path so far (device tensors)."""

    def __init__(self, env, prims, scale=5, padding=0.25, horizon=30, ship_vertices=None, threshold_cost=0.95, search_kwargs=None):
        self.env, self.prims = env, prims
        self.scale, self.padding, self.horizon, self.threshold_cost = scale, padding, horizon, threshold_cost
        self.fp_np = ship_footprint(LATTICE_SHIP_VERTICES if ship_vertices is None else ship_vertices, scale, padding)
        self.fp = torch.from_numpy(self.fp_np).to(env.device)
        self.search_kwargs = dict(search_kwargs or {})
        self.path = self.lengths = self.status = None
        self.found = torch.zeros((), dtype=torch.int64, device=env.device)

    def pose_cells(self):
        """The ships' poses in cost-map cells: [E, 3] float64."""
        return self.env.info[:, :3] * torch.tensor([self.scale, self.scale, 1.0], dtype=torch.float64, device=self.env.device)

    def plan(self, fresh=None, update=True):
        """One planning round; returns the kept paths [E, P, 3] and their lengths [E] (device tensors).  fresh: bool / uint8 [E] or None: envs that take
        their new path unconditionally, found or not (an episode start).  The other envs apply ``Path.update``'s comparison if `update`, else they keep
        their path and are not searched.  The first round takes every new path."""
        env, cfg, scale = self.env, self.env.cfg, self.scale
        m, n = int(cfg.occ.map_height), int(cfg.occ.map_width)
        pose = self.pose_cells()
        first = self.path is None
        if fresh is not None:
            fresh = fresh.to(device=env.device, dtype=torch.bool).contiguous()
        half = float(self.fp_np[:, 0].max() - self.fp_np[:, 0].min()) / 2
        maps = env.cost_maps(scale, m, n, horizon=self.horizon, ship_pos_y=pose[:, 1] - half, vs=float(cfg.target_speed) * scale + 1e-8)
        goal_y = torch.clamp(pose[:, 1] + self.horizon * scale, max=float(cfg.goal_y) * scale).contiguous()
        masks = lattice_swath_masks(env, self.prims, self.fp_np, pose[:, 2])
        active = fresh if (fresh is not None and not update and not first) else None
        res = env.lattice_search(maps, pose.contiguous(), goal_y, self.prims, masks, active=active, **self.search_kwargs)
        res.n_nodes = torch.where(res.status == 0, res.n_nodes, torch.zeros_like(res.n_nodes))   # only found envs have their rows written
        new, new_len = lattice_full_paths(self.prims, res, pose)
        self.status = res.status
        self.found += (res.status == 0).sum()
        if first:
            self.path, self.lengths = new, new_len
            return self.path, self.lengths
        if update:
            # Path.update: both swath costs over the rows from the ship to the goal line
            rows = torch.stack([pose[:, 1].to(torch.int32), goal_y.to(torch.int32)], 1).contiguous()
            both = torch.stack([new, self.path], 1).contiguous()
            cost = env.swath_costs(both, self.fp, maps, lengths=torch.stack([new_len, self.lengths], 1).contiguous(), rows=rows)
            take = (new_len > 0) & (replan_mask(cost[:, 0], cost[:, 1], self.threshold_cost) | (self.lengths == 0))
            if fresh is not None:
                take = take | fresh
        else:
            take = fresh if fresh is not None else torch.zeros_like(new_len, dtype=torch.bool)
        self.path = torch.where(take[:, None, None], new, self.path)
        self.lengths = torch.where(take, new_len, self.lengths)
        return self.path, self.lengths

    def paths_metres(self):
        """The kept paths in metres, [E, P, 3] contiguous: what ``track_paths`` takes next to the env's own poses."""
        return (self.path / torch.tensor([self.scale, self.scale, 1.0], dtype=torch.float64, device=self.env.device)).contiguous()

    def pursuit_actions(self, lookahead=15.0):
        """A plain pure-pursuit rule over the kept path (`lookahead` cells ahead of the ship): yaw actions [E] in [-1, 1].  Not the reference's
        controller: that is ``BatchedShipIceEnv.track_paths``."""
        dev = self.env.device
        pose = self.pose_cells()
        P = self.path.shape[1]
        valid = torch.arange(P, device=dev)[None, :] < self.lengths[:, None]
        d = torch.hypot(self.path[:, :, 0] - pose[:, None, 0], self.path[:, :, 1] - pose[:, None, 1])
        ahead = valid & (d >= lookahead) & (self.path[:, :, 1] > pose[:, None, 1])
        idx = torch.where(ahead.any(1), ahead.to(torch.int64).argmax(1), (self.lengths.to(torch.int64) - 1).clamp_min(0))
        tgt = self.path[torch.arange(self.path.shape[0], device=dev), idx]
        bearing = torch.atan2(tgt[:, 1] - pose[:, 1], tgt[:, 0] - pose[:, 0])
        err = torch.remainder(bearing - pose[:, 2] + torch.pi, 2 * torch.pi) - torch.pi
        return torch.where(self.lengths > 0, (2.0 * err).clamp(-1.0, 1.0), torch.zeros_like(err))


class RRTPlan(collections.namedtuple("RRTPlan", "status n_nodes iterations paths lengths")):
    """What ``BatchedMazeEnv.rrt_plan`` returns, device tensors: status int32 [E] (``_lib.RRT_*``), n_nodes and iterations int32 [E, 2] (one column
    per pass), paths float64 [E, max_waypoints, 2] (the pruned waypoints) and lengths int32 [E]."""
    __slots__ = ()


class RRTConfig:
    """The reference's RRT as data: rrt_config.yaml (step, goal_radius, goal_bias, max_nodes, densify_ds, seed), the ``min_dist`` that its policy
    prunes with, and this port's own: inflate_radius (None: 2.25 * cfg.robot.min_r, the reference's 1.5 * (1.5 * min_r)), max_waypoints (rows of the
    returned paths) and passes (2; 1: boxes always block).  Lfc and dt are the controller's (``track_waypoints``)."""
    FIELDS = ("step", "goal_radius", "goal_bias", "densify_ds", "prune_min_dist")

    def __init__(self, step=0.05, goal_radius=0.01, goal_bias=0.01, max_nodes=26000, densify_ds=0.08, prune_min_dist=0.3, inflate_radius=None, seed=42,
                 max_waypoints=256, passes=2, Lfc=0.5, dt=0.8):
        for k in self.FIELDS + ("Lfc", "dt"):
            setattr(self, k, float(locals()[k]))
        self.inflate_radius = None if inflate_radius is None else float(inflate_radius)
        self.max_nodes, self.seed, self.max_waypoints, self.passes = int(max_nodes), int(seed), int(max_waypoints), int(passes)

    def as_struct(self, env=None):
        from . import _lib
        r = self.inflate_radius if self.inflate_radius is not None else 1.5 * (1.5 * float(env.cfg.robot.min_r))   # policy.py, rrt.py: two factors of 1.5
        return _lib.BpRrtConfig(inflate_radius=r, seed=self.seed & 0xFFFFFFFFFFFFFFFF, max_nodes=self.max_nodes, max_waypoints=self.max_waypoints,
                                passes=self.passes, pad_=0, **{k: getattr(self, k) for k in self.FIELDS})


class GTSPPlan(collections.namedtuple("GTSPPlan", "status n_push tour cost paths lengths track_id track_setpoint weights")):
    """What ``BatchedAreaClearingEnv.gtsp_plan`` returns, device tensors: status int32 [E] (``_lib.GTSP_*`` in the low byte, ``GTSP_FLAG_*`` above),
    n_push int32 [E], tour int32 [E, max_boxes] (node c * G + g: cluster c to goal g), cost int32 [E], paths float64 [E, 2 * max_boxes + 1, 3],
    lengths int32 [E], the tracker's first state track_id int32 [E] / track_setpoint float64 [E, 2], and weights int32 [E, N_max, N_max] or None."""
    __slots__ = ()

    def tracker(self):
        """A fresh ``GTSPTrackerState`` at the plan's first state (copies)."""
        return GTSPTrackerState(ids=self.track_id.clone(), setpoint=self.track_setpoint.clone())


class GTSPConfig:
    """The reference's GTSP baseline as data: policy.py (the box is shrunk by 0.4, the push path extended by 2 behind the box and rounded to 7 decimals,
    the controller switches waypoints within 0.4), transition_graph_lookup.py (cost = 0.5 * length + pi / 4 * angle) and gtsp_config.yaml's controller
    (Lfc 0.5, dt 0.8, target_speed 0.2).  This port's own: max_boxes (boxes to push at most, <= 12: the DP table has 2^max_boxes rows) and num_goals
    (None: as many as the env's boundary goals, <= 8).  v_scale / w_scale None: the env's target_speed and max_yaw_rate_step."""
    FIELDS = ("shrink", "extend", "lin_vel", "ang_vel", "Lfc", "dt", "target_speed", "switch_dist")

    def __init__(self, shrink=0.4, extend=2.0, lin_vel=0.5, ang_vel=np.pi / 4, round_decimals=7, max_boxes=10, num_goals=None, Lfc=0.5, dt=0.8,
                 target_speed=0.2, switch_dist=0.4, v_scale=None, w_scale=None):
        for k in self.FIELDS:
            v = float(locals()[k])
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError("GTSPConfig: %s must be finite and not negative" % k)
            setattr(self, k, v)
        if not self.dt > 0.0:
            raise ValueError("GTSPConfig: dt must be positive")
        self.round_decimals, self.max_boxes = int(round_decimals), int(max_boxes)
        self.num_goals = None if num_goals is None else int(num_goals)
        if not 0 <= self.round_decimals <= 15:
            raise ValueError("GTSPConfig: round_decimals must be 0 .. 15")
        if self.max_boxes < 1 or (self.num_goals is not None and self.num_goals < 1):
            raise ValueError("GTSPConfig: max_boxes and num_goals must be positive")    # the upper caps are the library's to refuse
        self.v_scale = None if v_scale is None else float(v_scale)
        self.w_scale = None if w_scale is None else float(w_scale)
        for k in ("v_scale", "w_scale"):
            v = getattr(self, k)
            if v is not None and not (np.isfinite(v) and v > 0.0):
                raise ValueError("GTSPConfig: %s must be positive and finite" % k)

    def as_dict(self):
        return dict({k: getattr(self, k) for k in self.FIELDS}, round_decimals=self.round_decimals, max_boxes=self.max_boxes, num_goals=self.num_goals)

    def as_struct(self, env=None, num_goals=None):
        from . import _lib
        G = self.num_goals if self.num_goals is not None else num_goals
        v = self.v_scale if self.v_scale is not None else float(env.target_speed)
        w = self.w_scale if self.w_scale is not None else float(env.max_yaw_rate_step)
        return _lib.BpGtspConfig(v_scale=v, w_scale=w, round_decimals=self.round_decimals, max_boxes=self.max_boxes, num_goals=int(G), pad_=0,
                                 **{k: getattr(self, k) for k in self.FIELDS})


class GTSPTrackerState:
    """What the GTSP controller keeps between calls, on the device: ``ids`` int32 [E] (``current_point_id``) and ``setpoint`` float64 [E, 2]."""

    def __init__(self, num_envs=None, device="cuda:0", ids=None, setpoint=None):
        self.ids = torch.ones(int(num_envs), dtype=torch.int32, device=device) if ids is None else ids
        self.setpoint = torch.zeros((self.ids.shape[0], 2), dtype=torch.float64, device=self.ids.device) if setpoint is None else setpoint

    def take(self, plan, mask=None):
        """The first state of `plan` for the envs of `mask` (bool / uint8 [E]; None: all).  No host synchronisation."""
        if mask is None:
            self.ids.copy_(plan.track_id)
            self.setpoint.copy_(plan.track_setpoint)
        else:
            m = mask.to(device=self.ids.device, dtype=torch.bool)
            self.ids.copy_(torch.where(m, plan.track_id, self.ids))
            self.setpoint.copy_(torch.where(m[:, None], plan.track_setpoint, self.setpoint))
        return self

    def clone(self):
        return GTSPTrackerState(ids=self.ids.clone(), setpoint=self.setpoint.clone())


def boundary_goals(boundary, walls, buffer=0.1, min_len=0.1):
    """``PlanningBasedPolicy._compute_boundary_goals`` (policy.py:88-117) in numpy: every edge of the boundary polygon minus the `buffer`-capsule of
    every wall segment, pieces no longer than `min_len` dropped.  Returns float64 [G, 2, 2] in edge order, the pieces of an edge from its start.  The
    capsule is exact (a stadium), where shapely's ``buffer`` is a polygon with 16 segments per quarter circle."""
    bd = np.asarray(boundary, np.float64).reshape(-1, 2)
    out = []
    for i in range(len(bd)):
        a, b = bd[i], bd[(i + 1) % len(bd)]
        d = b - a
        L = float(np.hypot(d[0], d[1]))
        if L == 0.0:
            continue
        cut = []                                         # parameter intervals of the edge inside some capsule
        for w in ([] if walls is None else walls):
            w = np.asarray(w, np.float64).reshape(-1, 2)
            for k in range(len(w) - 1):
                iv = _capsule_interval(a, d, L, w[k], w[k + 1], float(buffer))
                if iv is not None:
                    cut.append(iv)
        t0 = 0.0
        for lo, hi in sorted(cut):
            if lo > t0 and (lo - t0) * L > min_len:
                out.append([a + t0 * d, a + lo * d])
            t0 = max(t0, hi)
        if t0 < 1.0 and (1.0 - t0) * L > min_len:
            out.append([a + t0 * d, b])
    return np.asarray(out, np.float64).reshape(-1, 2, 2)


def _capsule_interval(a, d, L, p, q, r):
    """The parameters t in [0, 1] of a + t * d whose distance to the segment (p, q) is below r: one interval (the distance is convex in t), or None."""
    def dist(t):
        x = a + t * d
        e = q - p
        l2 = float(e @ e)
        s = 0.0 if l2 == 0.0 else min(1.0, max(0.0, float((x - p) @ e) / l2))
        return float(np.hypot(*(x - (p + s * e))))
    lo, hi = 0.0, 1.0                                    # ternary search for the minimum of a convex function, then bisection for the two crossings
    for _ in range(200):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if dist(m1) <= dist(m2):
            hi = m2
        else:
            lo = m1
    tm = (lo + hi) / 2
    if not dist(tm) < r:
        return None
    ends = []
    for end in (0.0, 1.0):
        if dist(end) < r:
            ends.append(end)
            continue
        inside, outside = tm, end
        for _ in range(200):
            mid = (inside + outside) / 2
            if dist(mid) < r:
                inside = mid
            else:
                outside = mid
        ends.append(inside)
    return ends[0], ends[1]


class TrackerConfig:
    """The tunables of the reference's tracking controller (``PlanningBasedPolicy.act``, policy.py:63-82) as data; the defaults are the reference's values.
    They are in the units of the paths and poses that ``track_paths`` is given (the reference: metres).  action_scale None: the env's max_yaw_rate_step."""
    FIELDS = ("thresh", "look_car", "d_back", "d_ahead", "kp", "ki", "kd", "i_cap", "dead", "straight_ang", "yaw_big", "omega_small", "kp_v", "ki_v",
              "v_max", "omega_max", "dt")

    def __init__(self, thresh=10.0, look_car=50.0, d_back=15.0, d_ahead=25.0, kp=0.10, ki=0.15, kd=2.0, i_cap=10.0, dead=0.02, straight_ang=0.100,
                 yaw_big=0.50, omega_small=0.002, kp_v=0.50, ki_v=0.05, v_max=2.5, omega_max=0.02, dt=0.005, action_scale=None):
        for k, v in list(locals().items()):
            if k in self.FIELDS:
                setattr(self, k, float(v))
        self.action_scale = None if action_scale is None else float(action_scale)

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}


class TrackerState:
    """The integrators that the controller keeps between calls: ``state`` float64 [E, 4] = (int_yaw, prev_yaw, int_v, has_yaw) on the device.  A zero row
    is a fresh controller."""

    def __init__(self, num_envs=None, device="cuda:0", state=None):
        self.state = torch.zeros((int(num_envs), 4), dtype=torch.float64, device=device) if state is None else state

    def reset(self, mask=None):
        """Fresh controllers for the envs of `mask` (bool / uint8 [E]; None: all).  No host synchronisation."""
        if mask is None:
            self.state.zero_()
        else:
            self.state.masked_fill_(mask.to(device=self.state.device, dtype=torch.bool)[:, None], 0.0)
        return self

    def clone(self):
        return TrackerState(state=self.state.clone())

    def to(self, device):
        return TrackerState(state=self.state.to(device))


def straight_paths(pose, goal_y, dy=10, max_len=None):
    """The reference's ``straight_planner`` (policy.py:44-59) for a batch: from every pose [E, 3] = (x, y, theta) the samples (x, y + i * dy, theta) up to
    goal_y (a number or [E]), goal_y itself included where it lands on the grid -- ``np.arange(y, goal_y + dy * 0.5, dy)`` value for value.  Returns
    (paths [E, P, 3] float64, lengths [E] int32) on pose's device; rows beyond an env's length repeat nothing meaningful (zeros).  max_len None: P is
    the longest length, which is read back from the device once; with max_len given nothing is read back and longer paths are cut to it."""
    pose = torch.as_tensor(pose, dtype=torch.float64)
    if pose.dim() != 2 or pose.shape[1] != 3:
        raise ValueError("straight_paths: pose must be [E, 3]")
    if not dy > 0:
        raise ValueError("straight_paths: dy must be positive")
    E, dev = pose.shape[0], pose.device
    gy = torch.as_tensor(goal_y, dtype=torch.float64).to(dev).expand(E)
    x, y, th = pose[:, 0], pose[:, 1], pose[:, 2]
    n = torch.ceil(((gy + dy * 0.5) - y) / dy).clamp(min=0)
    n = torch.where(torch.isfinite(n), n, torch.zeros_like(n)).to(torch.int64)
    P = max(1, int(n.max()) if E else 1) if max_len is None else int(max_len)
    if P <= 0:
        raise ValueError("straight_paths: max_len must be positive")
    n = n.clamp(max=P)
    i = torch.arange(P, dtype=torch.float64, device=dev)[None, :]
    nxt = y + dy
    yv = y[:, None] + i * (nxt - y)[:, None]           # numpy fills a float arange as start + i * ((start + step) - start)
    if P > 1:
        yv[:, 1] = nxt
    valid = (torch.arange(P, device=dev)[None, :] < n[:, None])[:, :, None]
    out = torch.stack([x[:, None].expand(E, P), yv, th[:, None].expand(E, P)], dim=-1)
    return torch.where(valid, out, torch.zeros_like(out)).contiguous(), n.to(torch.int32)
