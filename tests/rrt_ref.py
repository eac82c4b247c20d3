"""Scalar restatement of the batched RRT and of the waypoint controller (DESIGN.md "RRT"; include/benchpush_amd.h: bp_rrt_plan, bp_track_waypoints)
in Python floats.  Helper of test_rrt_cpu.py, test_gpu_rrt.py and test_gpu_track_waypoints.py; tests/golden/make_golden_rrt.py runs the reference's own
``_run_rrt`` / ``prune_by_distance`` / ``DP.ideal_control`` next to it.

Every float operation below is one IEEE binary64 +, -, *, / or sqrt, in the order the kernel performs them, so the kernel is held to ``==``.  The
reference calls ``math.hypot`` where the kernel takes ``sqrt(dx * dx + dy * dy)``: ``rrt_plan(..., hypot=math.hypot)`` restates the reference itself
(steer, goal test and densify through hypot), which is what the goldens are compared with."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FOUND, FOUND_IGNORING_BOXES, FALLBACK, BLOCKED, CAP, BAD_INPUT, SKIPPED = range(7)
MASK = (1 << 64) - 1

# rrt_config.yaml of the reference, policy.py's prune_by_distance(min_dist=0.3)
DEFAULTS = dict(step=0.05, goal_radius=0.01, goal_bias=0.01, max_nodes=26000, densify_ds=0.08, prune_min_dist=0.3, inflate_radius=0.0, seed=42,
                max_waypoints=256, passes=2)
TRACK_DEFAULTS = dict(Lfc=0.5, dt=0.8)
# The controller's trig (atan2, sin / cos, atan2) is libm's in the reference and the oracle's deterministic functions here and on the device: each
# result is within an ulp or two of its own, all of magnitude pi at most, so theta_e agrees to a few ulp of pi -- 8 are allowed.  The action is
# theta_e / (dt * action_scale).
THETA_TOL = 8 * 4.440892098500626e-16


# ---- counter RNG ------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def rrt_uniform(seed, stream, p, k, j):
    """U(p, k, j) of env stream `stream`: a function of (seed, stream, pass, iteration, draw) only, in [0, 1)."""
    key = splitmix64((seed & MASK) ^ splitmix64(stream & MASK))
    z = splitmix64(key ^ (((p & 3) << 62) | ((k & 0xFFFFFFFF) << 2) | (j & 3)))
    return (z >> 11) * (1.0 / 9007199254740992.0)


# ---- predicates ---------------------------------------------------------------------------------------------------------
def orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _on(ax, ay, bx, by, cx, cy):
    """c inside the bounding box of (a, b), closed; with orient == 0: c on the segment."""
    return min(ax, bx) <= cx <= max(ax, bx) and min(ay, by) <= cy <= max(ay, by)


def seg_meet(a, b, c, d):
    """Do the closed segments (a, b) and (c, d) share a point?  Orientation signs only; a degenerate segment is a point."""
    o1 = orient(a[0], a[1], b[0], b[1], c[0], c[1])
    o2 = orient(a[0], a[1], b[0], b[1], d[0], d[1])
    o3 = orient(c[0], c[1], d[0], d[1], a[0], a[1])
    o4 = orient(c[0], c[1], d[0], d[1], b[0], b[1])
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    if o1 == 0 and _on(a[0], a[1], b[0], b[1], c[0], c[1]):
        return True
    if o2 == 0 and _on(a[0], a[1], b[0], b[1], d[0], d[1]):
        return True
    if o3 == 0 and _on(c[0], c[1], d[0], d[1], a[0], a[1]):
        return True
    if o4 == 0 and _on(c[0], c[1], d[0], d[1], b[0], b[1]):
        return True
    return False


def point_seg_d2(p, a, b):
    abx, aby = b[0] - a[0], b[1] - a[1]
    apx, apy = p[0] - a[0], p[1] - a[1]
    l2 = abx * abx + aby * aby
    if l2 == 0.0:
        return apx * apx + apy * apy
    t = (apx * abx + apy * aby) / l2
    t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
    ex, ey = p[0] - (a[0] + t * abx), p[1] - (a[1] + t * aby)
    return ex * ex + ey * ey


def seg_seg_d2(a, b, c, d):
    """Exact squared distance of two segments: 0 where they meet, else the smallest of the four point-segment distances."""
    if seg_meet(a, b, c, d):
        return 0.0
    return min(point_seg_d2(a, c, d), point_seg_d2(b, c, d), point_seg_d2(c, a, b), point_seg_d2(d, a, b))


def point_in_poly(p, poly):
    """p in or on the convex polygon, either winding: no two orientation signs oppose."""
    pos = neg = False
    n = len(poly)
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        o = orient(a[0], a[1], b[0], b[1], p[0], p[1])
        pos, neg = pos or o > 0, neg or o < 0
    return not (pos and neg)


class Scene:
    """Walls [W][4] and the counted box polygons of one env; ``seg_hit`` as the kernel decides it ('static' before 'movable')."""

    def __init__(self, walls, boxes, inflate_radius):
        self.walls = [tuple(float(v) for v in w) for w in walls]
        self.boxes = [[(float(x), float(y)) for x, y in poly] for poly in boxes if len(poly) > 0]
        self.r2 = inflate_radius * inflate_radius
        self.walls_infl = None     # the reference's _run_rrt reads it (its early return is the BLOCKED test here)
        xs = [w[0] for w in self.walls] + [w[2] for w in self.walls] + [q[0] for poly in self.boxes for q in poly]
        ys = [w[1] for w in self.walls] + [w[3] for w in self.walls] + [q[1] for poly in self.boxes for q in poly]
        self.bounds = (min(xs), max(xs), min(ys), max(ys)) if xs else (-3.0, 3.0, -3.0, 3.0)

    def static_hit(self, a, b):
        return any(seg_seg_d2(a, b, (w[0], w[1]), (w[2], w[3])) <= self.r2 for w in self.walls)

    def movable_hit(self, a, b):
        for poly in self.boxes:
            if point_in_poly(a, poly) or point_in_poly(b, poly):
                return True
            if any(seg_meet(a, b, poly[i], poly[(i + 1) % len(poly)]) for i in range(len(poly))):
                return True
        return False

    def seg_hit(self, a, b, boxes_blocking):
        if self.static_hit(a, b):
            return "static"
        if boxes_blocking and self.movable_hit(a, b):
            return "movable"
        return "none"

    def blocked(self, p):
        return any(point_seg_d2(p, (w[0], w[1]), (w[2], w[3])) <= self.r2 for w in self.walls)


# ---- the search --------------------------------------------------------------------------------------------------------
def _sqrt_hypot(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def rrt_pass(start, goal, scene, cfg, boxes_blocking, draw, hypot=None, audit=None):
    """One ``_run_rrt``.  draw(k, j) -> U(p, k, j).  Returns (nodes, parents, iterations, found).  With hypot None the distances that are compared are
    squared and the one that is divided by is their sqrt (the kernel); with ``math.hypot`` the steer, the goal test (and _densify) take the reference's
    distances.  The nearest node is the first minimum of d2 either way (numpy, elementwise IEEE); with an `audit` dict every iteration also finds the
    reference's own ``min(range(n), key=hypot)``, counts in audit['argmin_diff'] where the two differ, and goes on with the reference's."""
    xmin, xmax, ymin, ymax = scene.bounds
    step, gr = cfg["step"], cfg["goal_radius"]
    cap = cfg["max_nodes"] + 2
    nx, ny = np.zeros(cap), np.zeros(cap)
    nx[0], ny[0] = start
    nodes, parents = [tuple(start)], [-1]
    its = 0
    for k in range(cfg["max_nodes"]):
        its = k + 1
        if draw(k, 0) < cfg["goal_bias"]:
            q = tuple(goal)
        else:
            q = (xmin + (xmax - xmin) * draw(k, 1), ymin + (ymax - ymin) * draw(k, 2))
        n = len(nodes)
        ddx, ddy = nx[:n] - q[0], ny[:n] - q[1]
        d2 = ddx * ddx + ddy * ddy
        near = int(np.argmin(d2))
        if audit is not None:
            near_h = min(range(n), key=lambda i: math.hypot(nodes[i][0] - q[0], nodes[i][1] - q[1]))
            audit["argmin_diff"] = audit.get("argmin_diff", 0) + (near_h != near)
            near = near_h
        a = nodes[near]
        dx, dy = q[0] - a[0], q[1] - a[1]
        L = math.sqrt(float(d2[near])) if hypot is None else hypot(dx, dy)
        if L <= step or L == 0.0:
            new = q
        else:
            s = step / L
            new = (a[0] + s * dx, a[1] + s * dy)
        if scene.seg_hit(a, new, boxes_blocking) != "none":
            continue
        nx[n], ny[n] = new
        nodes.append(new)
        parents.append(near)
        gx, gy = new[0] - goal[0], new[1] - goal[1]
        if (gx * gx + gy * gy <= gr * gr) if hypot is None else (hypot(gx, gy) <= gr):
            nodes.append(tuple(goal))
            parents.append(len(nodes) - 2)
            return nodes, parents, its, True
    return nodes, parents, its, False


def backtrack(nodes, parents):
    path, idx = [], len(nodes) - 1
    while idx != -1:
        path.append(nodes[idx])
        idx = parents[idx]
    return path[::-1]


def densify(path, ds, hypot=None):
    hypot = hypot or _sqrt_hypot
    if len(path) <= 1:
        return list(path)
    ds = max(1e-3, ds)
    dense = [path[0]]
    for i in range(1, len(path)):
        a, b = dense[-1], path[i]
        n = max(1, int(hypot(b[0] - a[0], b[1] - a[1]) / ds))
        for k in range(1, n + 1):
            t = k / n
            dense.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    return dense


def prune(path, min_dist):
    """prune_by_distance of the reference's policy; np.linalg.norm of a pair is sqrt(dx * dx + dy * dy)."""
    out, prev, final = [path[0]], path[0], path[-1]
    for q in path[1:-1]:
        if _sqrt_hypot(q[0] - prev[0], q[1] - prev[1]) >= min_dist and _sqrt_hypot(q[0] - final[0], q[1] - final[1]) >= min_dist:
            out.append(q)
            prev = q
    out.append(path[-1])
    return out


def rrt_plan(start, goal, walls, boxes, stream, cfg=None, sampler=None, hypot=None, audit=None):
    """One env.  boxes: a list of vertex lists (an empty one is skipped).  sampler(p, k, j), if given, replaces the counter RNG.  Returns a dict with
    status, n_nodes [2], iterations [2], path (the pruned waypoints, a list of pairs), and for the tests nodes / parents / raw (the densified path) of
    the pass that ended the search."""
    c = dict(DEFAULTS, **(cfg or {}))
    start, goal = (float(start[0]), float(start[1])), (float(goal[0]), float(goal[1]))
    out = dict(status=BAD_INPUT, n_nodes=[0, 0], iterations=[0, 0], path=[], nodes=[], parents=[], raw=[])
    flat = list(start) + list(goal) + [float(v) for w in walls for v in w] + [float(v) for poly in boxes for q in poly for v in q]
    if not all(math.isfinite(v) for v in flat) or any(0 < len(poly) < 3 for poly in boxes):
        return out
    scene = Scene(walls, boxes, c["inflate_radius"])
    if scene.blocked(start) or scene.blocked(goal):
        return dict(out, status=BLOCKED, path=[start, goal])
    for p in range(c["passes"]):
        draw = (lambda k, j, p=p: sampler(p, k, j)) if sampler else (lambda k, j, p=p: rrt_uniform(c["seed"], stream, p, k, j))
        nodes, parents, its, found = rrt_pass(start, goal, scene, c, p == 0, draw, hypot, audit)
        out["n_nodes"][p], out["iterations"][p] = len(nodes), its
        out["nodes"], out["parents"] = nodes, parents
        if found:
            raw = densify(backtrack(nodes, parents), c["densify_ds"], hypot)
            pr = prune(raw, c["prune_min_dist"])
            if len(pr) > c["max_waypoints"]:
                return dict(out, status=CAP, raw=raw, cap_prefix=pr[:c["max_waypoints"]])
            return dict(out, status=FOUND if p == 0 else FOUND_IGNORING_BOXES, raw=raw, path=pr)
    return dict(out, status=FALLBACK, path=[start, goal])


def rrt_plan_batch(starts, goals, walls, boxes, counts, streams, cfg=None, active=None):
    """The restatement over a batch, as arrays shaped like the kernel's outputs: (status [E], n_nodes [E, 2], iterations [E, 2], paths [E, P, 2],
    lengths [E]) with zeros where the device writes nothing, plus the list of per-env dicts."""
    c = dict(DEFAULTS, **(cfg or {}))
    E, P = len(starts), c["max_waypoints"]
    status, nn, it = np.zeros(E, np.int32), np.zeros((E, 2), np.int32), np.zeros((E, 2), np.int32)
    paths, lengths, plans = np.zeros((E, P, 2)), np.zeros(E, np.int32), []
    for e in range(E):
        if active is not None and not active[e]:
            status[e] = SKIPPED
            plans.append(None)
            continue
        polys = [np.asarray(boxes[e][b][:max(int(counts[e][b]), 0)]).tolist() for b in range(len(counts[e]))]
        if any(int(n) < 0 or int(n) > np.asarray(boxes).shape[2] for n in counts[e]):
            polys = [[(0.0, 0.0)]]      # a count outside 0, 3 .. V is a bad input
        r = rrt_plan(starts[e], goals[e], walls, polys, int(streams[e]), c)
        plans.append(r)
        status[e], nn[e], it[e], lengths[e] = r["status"], r["n_nodes"], r["iterations"], len(r["path"])
        wp = r["path"] or r.get("cap_prefix")       # CAP: length 0, the first max_waypoints waypoints are written
        if wp:
            paths[e, :len(wp)] = wp
    return status, nn, it, paths, lengths, plans


# ---- the waypoint controller ---------------------------------------------------------------------------------------------
def _oracle_fns():
    from oracle import oracle as orc
    from oracle import oracle_bd
    return orc.sincos, oracle_bd.atan2


LIBM = (lambda x: (math.sin(x), math.cos(x)), math.atan2)


def track_waypoints_ref(path, pose, action_scale, length=None, cfg=None, fns=None):
    """``DP(x, y, yaw, cx, cy, ...).ideal_control(x, y, yaw)[0] / action_scale`` as the reference's act computes it from a fresh DP at every call.
    path [P, 2].  Returns (action, (nearest index, target index)); (nan, (-1, -1)) for a length below 1 or a non-finite pose or counted waypoint."""
    c = dict(TRACK_DEFAULTS, **(cfg or {}))
    sincos, atan2 = fns or _oracle_fns()
    path = np.asarray(path, np.float64).reshape(-1, 2)
    n = len(path) if length is None else min(int(length), len(path))
    x, y, yaw = (float(v) for v in pose)
    if n < 1 or not (np.isfinite(path[:n]).all() and math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
        return math.nan, (-1, -1)
    px, py = path[:n, 0].tolist(), path[:n, 1].tolist()
    best, near = None, 0
    for i in range(n):
        dx, dy = x - px[i], y - py[i]
        d2 = dx * dx + dy * dy
        if best is None or d2 < best:
            best, near = d2, i
    ind = near
    while True:
        dx, dy = x - px[ind], y - py[ind]
        if not (c["Lfc"] > math.sqrt(dx * dx + dy * dy)) or ind + 1 >= n:
            break
        ind += 1
    theta_d = atan2(py[ind] - y, px[ind] - x)
    s, co = sincos(theta_d - yaw)
    theta_e = atan2(s, co)
    return theta_e / c["dt"] / action_scale, (near, ind)


def load_golden(name="rrt_golden.json"):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)
