"""Dubins shortest paths between two poses (numpy / math only; imports neither torch nor the package, so any interpreter can load it by file path).

Restated from the published construction (L. E. Dubins 1957; the six words LSL, LSR, RSL, RSR, RLR, LRL in the normalised frame of Shkel & Lumelsky
2001, as the widely used ``dubins`` package computes them): a path is three segments of lengths (t, p, q) in units of the turning radius.  The
interface mirrors what the reference's ``get_points_on_dubins_path`` calls: ``shortest_path(q0, q1, rho)`` -> ``path_length()`` and
``sample_many(step)``, whose samples are taken at 0, step, 2 * step, ... < length, so the end point is not included.  Parity with that package is
unpinned: it is absent here."""
import math

LSL, LSR, RSL, RSR, RLR, LRL = range(6)
WORDS = ("LSL", "LSR", "RSL", "RSR", "RLR", "LRL")
_TWO_PI = 2.0 * math.pi


def mod2pi(t):
    return t - _TWO_PI * math.floor(t / _TWO_PI)


def _words(alpha, beta, d):
    sa, sb, ca, cb, cab = math.sin(alpha), math.sin(beta), math.cos(alpha), math.cos(beta), math.cos(alpha - beta)
    out = [None] * 6
    p2 = 2.0 + d * d - 2.0 * cab + 2.0 * d * (sa - sb)
    if p2 >= 0.0:
        tmp = math.atan2(cb - ca, d + sa - sb)
        out[LSL] = (mod2pi(tmp - alpha), math.sqrt(p2), mod2pi(beta - tmp))
    p2 = -2.0 + d * d + 2.0 * cab + 2.0 * d * (sa + sb)
    if p2 >= 0.0:
        p = math.sqrt(p2)
        tmp = math.atan2(-ca - cb, d + sa + sb) - math.atan2(-2.0, p)
        out[LSR] = (mod2pi(tmp - alpha), p, mod2pi(tmp - mod2pi(beta)))
    p2 = -2.0 + d * d + 2.0 * cab - 2.0 * d * (sa + sb)
    if p2 >= 0.0:
        p = math.sqrt(p2)
        tmp = math.atan2(ca + cb, d - sa - sb) - math.atan2(2.0, p)
        out[RSL] = (mod2pi(alpha - tmp), p, mod2pi(beta - tmp))
    p2 = 2.0 + d * d - 2.0 * cab + 2.0 * d * (sb - sa)
    if p2 >= 0.0:
        tmp = math.atan2(ca - cb, d - sa + sb)
        out[RSR] = (mod2pi(alpha - tmp), math.sqrt(p2), mod2pi(tmp - beta))
    tmp = (6.0 - d * d + 2.0 * cab + 2.0 * d * (sa - sb)) / 8.0
    if abs(tmp) <= 1.0:
        phi = math.atan2(ca - cb, d - sa + sb)
        p = mod2pi(_TWO_PI - math.acos(tmp))
        t = mod2pi(alpha - phi + mod2pi(p / 2.0))
        out[RLR] = (t, p, mod2pi(alpha - beta - t + mod2pi(p)))
    tmp = (6.0 - d * d + 2.0 * cab + 2.0 * d * (sb - sa)) / 8.0
    if abs(tmp) <= 1.0:
        phi = math.atan2(ca - cb, d + sa - sb)
        p = mod2pi(_TWO_PI - math.acos(tmp))
        t = mod2pi(-alpha - phi + p / 2.0)
        out[LRL] = (t, p, mod2pi(mod2pi(beta) - alpha - t + mod2pi(p)))
    return out


def _segment(t, q, kind):
    x, y, th = q
    if kind == "L":
        return (x + math.sin(th + t) - math.sin(th), y - math.cos(th + t) + math.cos(th), th + t)
    if kind == "R":
        return (x - math.sin(th - t) + math.sin(th), y + math.cos(th - t) - math.cos(th), th - t)
    return (x + math.cos(th) * t, y + math.sin(th) * t, th)


class DubinsPath:
    def __init__(self, q0, q1, rho, word=None):
        if not rho > 0.0:
            raise ValueError("dubins: the turning radius must be positive")
        self.q0, self.q1, self.rho = tuple(map(float, q0)), tuple(map(float, q1)), float(rho)
        dx, dy = self.q1[0] - self.q0[0], self.q1[1] - self.q0[1]
        d = math.sqrt(dx * dx + dy * dy) / self.rho
        theta = mod2pi(math.atan2(dy, dx)) if d > 0.0 else 0.0
        cands = _words(mod2pi(self.q0[2] - theta), mod2pi(self.q1[2] - theta), d)
        best = None
        for w, prm in enumerate(cands):
            if prm is None or (word is not None and w != word):
                continue
            cost = prm[0] + prm[1] + prm[2]
            if best is None or cost < best[0]:
                best = (cost, w, prm)
        if best is None:
            raise ValueError("dubins: no path of the requested word")
        self.word, self.params = best[1], best[2]

    def path_type(self):
        return self.word

    def segment_length(self, i):
        return self.params[i] * self.rho

    def path_length(self):
        return (self.params[0] + self.params[1] + self.params[2]) * self.rho

    def sample(self, t):
        """The pose at arc length t, 0 <= t <= path_length()."""
        if t < 0.0 or t > self.path_length():
            raise ValueError("dubins: sample outside the path")
        tp = t / self.rho
        kinds = WORDS[self.word]
        p1, p2 = self.params[0], self.params[1]
        qi = (0.0, 0.0, self.q0[2])
        q1 = _segment(p1, qi, kinds[0])
        q2 = _segment(p2, q1, kinds[1])
        if tp < p1:
            q = _segment(tp, qi, kinds[0])
        elif tp < p1 + p2:
            q = _segment(tp - p1, q1, kinds[1])
        else:
            q = _segment(tp - p1 - p2, q2, kinds[2])
        return (q[0] * self.rho + self.q0[0], q[1] * self.rho + self.q0[1], mod2pi(q[2]))

    def sample_many(self, step):
        """(configurations, distances) at 0, step, 2 * step, ... < path_length(); the end point is not included."""
        if not step > 0.0:
            raise ValueError("dubins: the step must be positive")
        qs, ts = [], []
        x, length = 0.0, self.path_length()
        while x < length:
            qs.append(self.sample(x))
            ts.append(x)
            x += step
        return qs, ts


def shortest_path(q0, q1, rho):
    return DubinsPath(q0, q1, rho)


def path(q0, q1, rho, word):
    return DubinsPath(q0, q1, rho, word)
