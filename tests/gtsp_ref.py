"""Scalar restatement of the GTSP push planner and its tracker (DESIGN.md "GTSP"; include/benchpush_amd.h: bp_gtsp_plan, bp_gtsp_track) in Python
floats and ints, built on the oracle's deterministic sin / cos and atan2.  Helper of test_gtsp_cpu.py and test_gpu_gtsp.py; the kernels are held to ==
against it.  tests/golden/make_golden_gtsp.py runs the reference's own TransitionGraphLookup, cost matrix, evaluate_tour and PlanningBasedPolicy.act on
the push paths and tours computed here.  ``brute_force`` is a second, independent solver: every cluster order times every node choice."""
import itertools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, NOTHING_TO_PUSH, SKIPPED, CAP, INVALID = 0, 1, 2, 3, 4
FLAG_VANISHED, FLAG_DEGENERATE = 0x100, 0x200
SELF_WEIGHT = 99999999
MAX_BOXES, MAX_GOALS = 12, 8

# gtsp_config.yaml's controller, policy.py's buffer(-0.4), EXTEND_BUFFER, np.round(.., 7) and the 0.4 of act, transition_graph_lookup.py's LIN_VEL, ANG_VEL
DEFAULTS = dict(shrink=0.4, extend=2.0, lin_vel=0.5, ang_vel=math.pi / 4, round_decimals=7, max_boxes=10, num_goals=4, Lfc=0.5, dt=0.8,
                target_speed=0.2, switch_dist=0.4)


def _oracle_fns():
    from oracle import oracle as orc
    from oracle import oracle_bd
    return orc.sincos, oracle_bd.atan2


LIBM = (lambda x: (math.sin(x), math.cos(x)), math.atan2)


def _area2(p):
    s = 0.0
    for i in range(len(p)):
        j = i + 1 if i + 1 < len(p) else 0
        s += p[i][0] * p[j][1] - p[j][0] * p[i][1]
    return s


def _sep(a, b):
    """An edge of `a` has all of `b` strictly on its outer side (AreaClearingEnv._statuses)."""
    o = 1.0 if _area2(a) > 0 else -1.0
    for i in range(len(a)):
        j = i + 1 if i + 1 < len(a) else 0
        ex, ey = a[j][0] - a[i][0], a[j][1] - a[i][1]
        if all((ex * (q[1] - a[i][1]) - ey * (q[0] - a[i][0])) * o < 0 for q in b):
            return True
    return False


def intersects(boundary, box):
    return not (_sep(boundary, box) or _sep(box, boundary))


def shrink(p, d):
    """The exact inward offset of the convex polygon p by d: p clipped by every edge's half-plane moved inwards by d.  None if nothing is left."""
    area = _area2(p)
    if area == 0:
        return None
    o = 1.0 if area > 0 else -1.0
    cur = [tuple(v) for v in p]
    for i in range(len(p)):
        a, b = p[i], p[i + 1 if i + 1 < len(p) else 0]
        ex, ey = b[0] - a[0], b[1] - a[1]
        L = math.sqrt(ex * ex + ey * ey)
        if L == 0:
            continue
        nx, ny = (o * -ey) / L, (o * ex) / L
        f = [((q[0] - a[0]) * nx + (q[1] - a[1]) * ny) - d for q in cur]
        nxt = []
        for k in range(len(cur)):
            k2 = k + 1 if k + 1 < len(cur) else 0
            P, Q, fp, fq = cur[k], cur[k2], f[k], f[k2]
            if fp >= 0:
                nxt.append(P)
            if (fp >= 0) != (fq >= 0):
                t = fp / (fp - fq)
                nxt.append((P[0] + t * (Q[0] - P[0]), P[1] + t * (Q[1] - P[1])))
        cur = nxt
        if len(cur) < 3:
            return None
    if not _area2(cur) * o > 0:
        return None
    return cur


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _on(a, b, c):
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _seg_meet(a, b, c, d):
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, d), _orient(c, d, a), _orient(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return (o1 == 0 and _on(a, b, c)) or (o2 == 0 and _on(a, b, d)) or (o3 == 0 and _on(c, d, a)) or (o4 == 0 and _on(c, d, b))


def _proj(p, a, b):
    """The point of the segment (a, b) nearest p, and the squared distance."""
    abx, aby, apx, apy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    l2 = abx * abx + aby * aby
    q = a
    if l2 != 0:
        t = (apx * abx + apy * aby) / l2
        t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
        q = (a[0] + t * abx, a[1] + t * aby)
    ex, ey = p[0] - q[0], p[1] - q[1]
    return (q[0], q[1]), ex * ex + ey * ey


def nearest_pair(box, poly, g0, g1):
    """(box point, goal point, degenerate) between the shrunk box `poly` and the goal segment: among equally near pairs the lowest-index vertex of
    `poly` projected onto the segment; a segment endpoint projected onto an edge only when strictly nearer.  Degenerate (the shrunk box touches or
    crosses the segment, or holds it): both are the segment's point nearest the mean of the vertices of `box`."""
    m = len(poly)
    touch, pos, neg = False, False, False
    for j in range(m):
        a, b = poly[j], poly[j + 1 if j + 1 < m else 0]
        touch = touch or _seg_meet(a, b, g0, g1)
        o = _orient(a, b, g0)
        pos, neg = pos or o > 0, neg or o < 0
    if touch or not (pos and neg):
        sx = sy = 0.0
        for v in box:
            sx += v[0]
            sy += v[1]
        q, _ = _proj((sx / len(box), sy / len(box)), g0, g1)
        return q, q, True
    best = bp = gp = None
    for v in poly:
        q, d2 = _proj(v, g0, g1)
        if best is None or d2 < best:
            best, bp, gp = d2, (v[0], v[1]), q
    for e in (g0, g1):
        for j in range(m):
            q, d2 = _proj(e, poly[j], poly[j + 1 if j + 1 < m else 0])
            if d2 < best:
                best, bp, gp = d2, q, (e[0], e[1])
    return bp, gp, False


def push_route(box, poly, g0, g1, extend, scale):
    """The route [extended start, box point, goal point] of pushing `box` (shrunk: `poly`) to the goal segment, rounded; and whether it is degenerate."""
    rnd = lambda v: float(np.rint(v * scale)) / scale   # noqa: E731
    bp, gp, deg = nearest_pair(box, poly, g0, g1)
    dx, dy = bp[0] - gp[0], bp[1] - gp[1]
    L = math.sqrt(dx * dx + dy * dy)
    ext = bp if L == 0 else (bp[0] + (dx / L) * extend, bp[1] + (dy / L) * extend)
    return [(rnd(ext[0]), rnd(ext[1])), (rnd(bp[0]), rnd(bp[1])), (rnd(gp[0]), rnd(gp[1]))], deg


def _angle(a, b, atan2):
    if math.sqrt(a[0] * a[0] + a[1] * a[1]) == 0 or math.sqrt(b[0] * b[0] + b[1] * b[1]) == 0:
        return 0.0
    return abs(atan2(a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1]))


# How far the reference's angle, arccos(clip(a . b / (|a| |b|))) in double precision, can lie from the angle |atan2(a x b, a . b)| used here.  With
# u = 2^-53: the dot product of two 2-vectors is off by at most 2 u |a| |b|, each norm (two squares, a sum, a root) by 2 u of itself, their product and
# the quotient by u each, so the quotient q is off by Q_ERR = 8 u in absolute terms.  arccos moves by at most 2 Q_ERR / sin(angle) for that, and by
# at most arccos(1 - Q_ERR) = sqrt(2 Q_ERR) = 4.2e-8 however near to parallel the directions are.  ANGLE_SLACK covers the rest: the arguments of
# atan2 are off by 2 u |a| |b| each (an angle of 4 u), arccos and atan2 round their results (an ulp of pi each), the two angles of an entry are added.
Q_ERR = 8 * 2.0 ** -53
ANGLE_SLACK = 2e-15
LENGTH_ERR = 4 * 2.0 ** -53 * 16          # sqrt(dx^2 + dy^2) against numpy's norm: 2 u of a length below 16 either way


def arccos_error(theta):
    """The bound above for one angle whose value is theta."""
    s = abs(math.sin(theta))
    return min(math.sqrt(2 * Q_ERR), 2 * Q_ERR / s if s > 0 else math.inf) + ANGLE_SLACK


def transition(du, frm, to, dv, lin_vel, ang_vel, atan2):
    """(cost, length, angle) of the straight transition frm -> to, left with direction du and continued with direction dv."""
    p = (to[0] - frm[0], to[1] - frm[1])
    ln = math.sqrt(p[0] * p[0] + p[1] * p[1])
    an = _angle(du, p, atan2) + _angle(p, dv, atan2)
    return lin_vel * ln + ang_vel * an, ln, an


def weight(cost):
    w = float(np.rint(100.0 * cost))
    return int(w) if w < SELF_WEIGHT else SELF_WEIGHT


def weight_matrix(routes, pose, G, cfg, fns=None, tables=False, bounds=False):
    """routes [n * G][3] (node c * G + g), pose (x, y, theta).  int [N, N], N = n * G + 1, the robot last.  tables: also the float cost / length / angle.
    bounds: also, per entry, how far the reference's arccos angle can lie from the angle here (``arccos_error`` of the entry's two angles)."""
    sincos, atan2 = fns or _oracle_fns()
    N = len(routes) + 1
    R = N - 1
    x, y, th = (float(v) for v in pose)
    s, c = sincos(th)
    rdir = ((x + 0.1 * c) - x, (y + 0.1 * s) - y)
    dirs = [(r[2][0] - r[1][0], r[2][1] - r[1][1]) for r in routes] + [rdir]
    start = [r[0] for r in routes] + [(x, y)]
    end = [r[2] for r in routes] + [(x, y)]
    W = np.zeros((N, N), np.int64)
    T = np.zeros((3, N, N))
    B = np.zeros((N, N))
    for u in range(N):
        for v in range(N):
            if u == v:
                W[u, v] = SELF_WEIGHT
            elif u != R and v != R and u // G == v // G:
                W[u, v] = 0
            else:
                T[:, u, v] = transition(dirs[u], end[u], start[v], dirs[v], cfg["lin_vel"], cfg["ang_vel"], atan2)
                W[u, v] = weight(T[0, u, v])
                if bounds:
                    p = (start[v][0] - end[u][0], start[v][1] - end[u][1])
                    B[u, v] = arccos_error(_angle(dirs[u], p, atan2)) + arccos_error(_angle(p, dirs[v], atan2))
    if bounds:
        return W, T, B
    return (W, T) if tables else W


def solve(W, n, G):
    """The backward set DP.  Returns (cost, tour): the optimum and the lexicographically smallest optimal tour (node indices, the robot left out)."""
    N = n * G + 1
    R = N - 1
    W = np.asarray(W, np.int64)[:N, :N]
    if n == 0:
        return 0, []
    cl = np.arange(R) // G
    h = np.zeros((1 << n, R), np.int64)          # rows of nodes whose cluster is in S are computed too and never read
    h[0] = W[:R, R]
    for S in range(1, 1 << n):
        us = np.nonzero((S >> cl) & 1)[0]
        h[S] = (W[:R, us] + h[S ^ (1 << cl[us]), us][None, :]).min(1)
    W, h = W.tolist(), h.tolist()
    full = (1 << n) - 1
    target = min(W[R][u] + h[full ^ (1 << (u // G))][u] for u in range(R))
    cost, tour, cur, S = target, [], R, full
    while S:
        for u in range(R):
            if (S >> (u // G)) & 1 and W[cur][u] + h[S ^ (1 << (u // G))][u] == target:
                break
        else:
            raise AssertionError("no successor attains h")
        S ^= 1 << (u // G)
        target = h[S][u]
        tour.append(u)
        cur = u
    return cost, tour


def brute_force(W, n, G, ties=False):
    """Every cluster order times every node choice; the smallest (cost, tour).  ties: also the number of tours that attain the smallest cost."""
    N = n * G + 1
    R = N - 1
    W = np.asarray(W)
    best, count = None, 0
    for order in itertools.permutations(range(n)):
        for pick in itertools.product(range(G), repeat=n):
            tour = [c * G + g for c, g in zip(order, pick)]
            seq = [R] + tour + [R]
            cost = sum(int(W[a, b]) for a, b in zip(seq[:-1], seq[1:]))
            count = 1 if best is None or cost < best[0] else count + (cost == best[0])
            if best is None or (cost, tour) < best:
                best = (cost, tour)
    best = best if n else (0, [])
    return best + (count if n else 1,) if ties else best


def track_init(path, length, pose, Lfc):
    """TargetCourse.init_setpoint on the path: (1, setpoint x, setpoint y)."""
    x, y = float(pose[0]), float(pose[1])
    best, ind = None, 0
    for i in range(length):
        dx, dy = x - path[i][0], y - path[i][1]
        d2 = dx * dx + dy * dy
        if best is None or d2 < best:
            best, ind = d2, i
    while True:
        dx, dy = x - path[ind][0], y - path[ind][1]
        if not Lfc > math.sqrt(dx * dx + dy * dy) or ind + 1 >= length:
            break
        ind += 1
    return 1, float(path[ind][0]), float(path[ind][1])


def plan(pose, boxes, counts, goals, boundary, cfg=None, fns=None, n_max=None):
    """One env.  boxes [B, V, 2] with counts [B], goals [G, 2, 2], boundary [nb, 2].  Returns a dict: status, n_push, W (int [N, N] or None), tour, cost,
    path [2 n + 1, 3], length, track (id, sx, sy), clusters (box indices), routes."""
    c = dict(DEFAULTS, **(cfg or {}))
    sincos, atan2 = fns or _oracle_fns()
    goals = np.asarray(goals, np.float64).reshape(-1, 2, 2)
    G = len(goals)
    boxes, counts = np.asarray(boxes, np.float64), np.asarray(counts)
    out = dict(status=INVALID, n_push=0, W=None, tour=[], cost=0, path=np.zeros((0, 3)), length=0, track=None, clusters=[], routes=[])
    bad = not np.isfinite(np.asarray(pose, np.float64)).all() or not np.isfinite(goals).all()
    for b in range(len(counts)):
        k = int(counts[b])
        if k == 0:
            continue
        if k < 3 or k > boxes.shape[1] or not np.isfinite(boxes[b, :k]).all():
            bad = True
    if bad:
        return out
    bd = [tuple(v) for v in np.asarray(boundary, np.float64).tolist()]
    scale = 10.0 ** int(c["round_decimals"])
    flags = 0
    clusters, routes = [], []
    for b in range(len(counts)):
        k = int(counts[b])
        if k == 0:
            continue
        box = [tuple(v) for v in boxes[b, :k].tolist()]
        if not intersects(bd, box):
            continue
        poly = shrink(box, c["shrink"])
        if poly is None:
            flags |= FLAG_VANISHED
            continue
        clusters.append(b)
        for g in range(G):
            r, deg = push_route(box, poly, tuple(goals[g, 0].tolist()), tuple(goals[g, 1].tolist()), c["extend"], scale)
            if deg:
                flags |= FLAG_DEGENERATE
            routes.append(r)
    n = len(clusters)
    out.update(n_push=n, clusters=clusters, routes=routes)
    x, y, th = (float(v) for v in pose)
    if n > (c["max_boxes"] if n_max is None else n_max):
        out["status"] = CAP | flags
        return out
    W = weight_matrix(routes, pose, G, c, (sincos, atan2))
    cost, tour = solve(W, n, G)
    path = [(x, y, th)]
    for u in tour:
        r = routes[u]
        hd = atan2(r[2][1] - r[0][1], r[2][0] - r[0][0])
        path += [(r[0][0], r[0][1], hd), (r[2][0], r[2][1], hd)]
    path = np.asarray(path, np.float64).reshape(-1, 3)
    out.update(status=(OK if n else NOTHING_TO_PUSH) | flags, W=W, tour=tour, cost=cost, path=path, length=len(path),
               track=track_init(path, len(path), pose, c["Lfc"]))
    return out


def track(path, length, pose, state, v_scale, w_scale, cfg=None, fns=None):
    """One call of the tracker for one env.  state (id, sx, sy).  Returns ((speed, omega) scaled, diag, new state); NaN, -1 and the state untouched for
    a length below 2, a negative id or a non-finite pose or counted waypoint."""
    c = dict(DEFAULTS, **(cfg or {}))
    sincos, atan2 = fns or _oracle_fns()
    path = np.asarray(path, np.float64).reshape(-1, 3)
    length = min(int(length), len(path))
    i, sx, sy = int(state[0]), float(state[1]), float(state[2])
    x, y, yaw = (float(v) for v in pose)
    if length < 2 or i < 0 or not (np.isfinite(path[:length]).all() and math.isfinite(x) and math.isfinite(y) and math.isfinite(yaw)):
        return (math.nan, math.nan), -1, (i, sx, sy)
    if i >= length:
        return (0.0, 0.0), i, (i, sx, sy)
    dx, dy = x - path[i][0], y - path[i][1]
    if math.sqrt(dx * dx + dy * dy) < c["switch_dist"]:
        i += 1
        if i >= length:
            return (0.0, 0.0), i, (i, sx, sy)
        sx, sy = float(path[i][0]), float(path[i][1])
    theta_d = atan2(sy - y, sx - x)
    s, co = sincos(theta_d - yaw)
    omega = atan2(s, co) / c["dt"]
    s, co = sincos(yaw)
    vx, vy = co * c["target_speed"], s * c["target_speed"]
    speed = math.sqrt(vx * vx + vy * vy)
    return (speed / v_scale, omega / w_scale), i, (i, sx, sy)


def load_golden():
    with open(os.path.join(GOLDEN, "gtsp_golden.json")) as f:
        G = json.load(f)
    Z = np.load(os.path.join(GOLDEN, "gtsp_golden.npz"))
    return G, Z
