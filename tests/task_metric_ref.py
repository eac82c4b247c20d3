"""Math-only restatement of the task-driven episode metric (DESIGN.md "Task-driven metrics"): python floats and math.sqrt, no numpy reductions, no graph
library.  tests/test_task_metrics_cpu.py holds it against benchpush_amd.metrics.TaskDrivenMetric and against bp_task_metric_row; the GPU tests use the host
class itself."""
import math

NAN, INF = float("nan"), float("inf")


def div(a, b):
    """IEEE division of two doubles (python raises for b == 0)."""
    if b != 0.0 and not math.isnan(b):
        return a / b
    if math.isnan(a) or math.isnan(b) or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def area_centroid(poly):
    """(|a|, cx, cy): shoelace sums in vertex order, the centroid with the signed a."""
    n = len(poly)
    sa = sx = sy = 0.0
    for i in range(n):
        x, y = float(poly[i][0]), float(poly[i][1])
        xn, yn = float(poly[(i + 1) % n][0]), float(poly[(i + 1) % n][1])
        cr = x * yn - xn * y
        sa += cr
        sx += (x + xn) * cr
        sy += (y + yn) * cr
    a = sa / 2
    return abs(a), div(sx, 6 * a), div(sy, 6 * a)


def norm(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def mst_cost(cent, d, robot):
    """Prim from box 0 over boxes 0..k-1, goal leaves k..2k-1 (edge d[i]) and the robot 2k; the frontier is a list in entry order, the first smallest key
    wins, a key that shrinks stays in place; the total is summed in the order the edges are taken."""
    k = len(cent)
    if k == 0:
        return 0.0
    R = 2 * k
    key = {j: norm(cent[0][0] - cent[j][0], cent[0][1] - cent[j][1]) for j in range(1, k)}
    key[R] = norm(robot[0] - cent[0][0], robot[1] - cent[0][1])
    key[k] = d[0]
    front = list(range(1, k)) + [R, k]
    total = 0.0
    while front:
        at = 0
        for q in range(1, len(front)):
            if key[front[q]] < key[front[at]]:
                at = q
        v = front.pop(at)
        total += key[v]
        if v != R and v >= k:
            continue
        for b in front:
            if b < k:
                w = norm(robot[0] - cent[b][0], robot[1] - cent[b][1]) if v == R else norm(cent[v][0] - cent[b][0], cent[v][1] - cent[b][1])
                if not key[b] < w:
                    key[b] = w
        if v == R:
            continue
        if R in front:
            w = norm(robot[0] - cent[v][0], robot[1] - cent[v][1])
            if not key[R] < w:
                key[R] = w
        key[k + v] = d[v]
        front.append(k + v)
    return total


def row(boxes_acxy, completed, goals, start, robot_mass, l0, total_work, reward, steps):
    """The six columns: efficiency, effort, reward, success, length, total_work."""
    cent, d, mmd = [], [], 0.0
    for (a, cx, cy), s in zip(boxes_acxy, completed):
        if not s:
            continue
        best = min(norm(g[0] - cx, g[1] - cy) for g in goals)
        cent.append((cx, cy)); d.append(best)
        mmd += best * a
    own = robot_mass * l0
    return [div(mst_cost(cent, d, start), l0), div(own + mmd, own + total_work), reward, div(float(len(cent)), float(len(completed))), float(steps),
            total_work]


def path_length(points):
    """l0: the sum of the step lengths of the rounded robot positions, in step order."""
    l0 = 0.0
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        l0 += norm(x0 - x1, y0 - y1)
    return l0
