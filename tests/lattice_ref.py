"""Numpy + heapq restatement of the lattice search (DESIGN.md "Lattice search"; include/benchpush_amd.h: bp_lattice_search): AStar.search of the
reference's a_star_search.py for the high-level planner (goal_pos=None, occ_map=None, smoothing off), on integer lattice nodes.  The kernel is held to
it with ==.  Helper of test_lattice_cpu.py and test_gpu_lattice.py; tests/golden/make_golden_lattice.py runs it next to the reference's own AStar.

Python floats are binary64 and nothing fuses, so every expression below is the operation order of the device code."""
import heapq
import math
import os
import struct

import numpy as np

FOUND, NO_PATH, CAP, SKIPPED = 0, 1, 2, 3
TWO_PI = 2 * math.pi
KEY_OFF, KEY_LIM = 4096, 4096          # |i|, |j| < 4096 sub-units: key = (j + 4096) << 18 | (i + 4096) << 5 | h
COORD_MAX = 1e9                        # a start or goal beyond this (or not finite) has no path: no conversion to int is attempted
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_sincos = None


def sincos(x):
    """The library's deterministic sin / cos (the oracle's orc_sincos, bit-identical to bp_sincos on the device)."""
    global _sincos
    if _sincos is None:
        from oracle import oracle as orc
        _sincos = orc.sincos
    return _sincos(x)


# ---- bp_acos: fdlibm's e_acos.c, operation by operation ---------------------------------------------------------------------------------------
_PIO2_HI, _PIO2_LO, _PI = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
_PS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
       7.91534994289814532176e-04, 3.47933107596021167570e-05)
_QS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)


def _words(x):
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b >> 32, b & 0xFFFFFFFF


def _pq(z):
    p = z * (_PS[0] + z * (_PS[1] + z * (_PS[2] + z * (_PS[3] + z * (_PS[4] + z * _PS[5])))))
    q = 1.0 + z * (_QS[0] + z * (_QS[1] + z * (_QS[2] + z * _QS[3])))
    return p / q


def bp_acos(x):
    x = float(x)
    hx, lx = _words(x)
    ix = hx & 0x7FFFFFFF
    if ix >= 0x3FF00000:                       # |x| >= 1 or NaN
        if ((ix - 0x3FF00000) | lx) == 0:
            return 0.0 if hx < 0x80000000 else _PI + 2.0 * _PIO2_LO
        return math.nan
    if ix < 0x3FE00000:                        # |x| < 0.5
        if ix <= 0x3C600000:
            return _PIO2_HI + _PIO2_LO
        r = _pq(x * x)
        return _PIO2_HI - (x - (_PIO2_LO - x * r))
    if hx >= 0x80000000:                       # x < -0.5
        z = (1.0 + x) * 0.5
        s = math.sqrt(z)
        w = _pq(z) * s - _PIO2_LO
        return _PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5                        # x > 0.5
    s = math.sqrt(z)
    df = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", s))[0] & 0xFFFFFFFF00000000))[0]
    c = (z - df * df) / (s + df)
    w = _pq(z) * s + c
    return 2.0 * (df + w)


# ---- heuristic ---------------------------------------------------------------------------------------------------------------------------------
def dubins_h(x, y, th, goal, r, b0, b1):
    """dubins_heuristic(q, goal, r_min, (b0, b1))[0] of common/dubins_helpers/heuristic.py with bp_sincos / bp_acos / IEEE sqrt."""
    if y >= goal:
        return 0.0
    s, c = sincos(th)
    m = 1.0 if (th <= math.pi / 2 or th >= 3 * math.pi / 2) else -1.0
    mr = m * r
    omega_y = y + mr * c
    if omega_y >= goal:
        n = 0.0 if th <= math.pi / 2 else (math.pi if th <= 3 * math.pi / 2 else 2 * math.pi)
        d = omega_y - goal
        theta = m * bp_acos(d / r) + n
        h = r * abs(th - theta)
        rad = r * r - d * d
        xx = (x - mr * s) + m * (math.sqrt(rad) if rad >= 0.0 else math.nan)
    else:
        h = (r * min(abs(math.pi / 2 - th), abs(5 * math.pi / 2 - th)) + goal) - omega_y
        xx = mr * (1.0 - s) + x
    if b0 > xx or xx > b1:
        if 0.0 <= th <= math.pi:
            h = math.inf
        else:
            omega_y = y - (omega_y - y)
            omega_x = x + mr * s
            if b0 > omega_x or omega_x > b1:
                h = math.inf
            else:
                h = (r * max(abs(math.pi / 2 - th), abs(5 * math.pi / 2 - th)) + goal) - omega_y
                xx = (-m) * r * (1.0 - s) + x
                if b0 > xx or xx > b1:
                    h = math.inf
    return h


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------
class Tables:
    """The primitive tables of one search configuration as the C ABI takes them.

    edges    per base heading a list of (ex, ey, eh): ex, ey in lattice units (floats such as 1.5), eh the edge heading
    lengths  per base heading a list of path lengths in cells
    nh       number of headings (8 or 16), nb = nh / 4 base headings; unit = cells per lattice unit; den = sub-units per lattice unit
    max_val  half side of the masks: S = 2 * max_val + 1; r = turning radius in cells"""

    def __init__(self, edges, lengths, nh, unit, den, max_val, r):
        self.nh, self.nb, self.unit, self.den, self.max_val, self.r = int(nh), int(nh) // 4, float(unit), int(den), int(max_val), float(r)
        assert len(edges) == self.nb and len(lengths) == self.nb
        self.ne_max = max(len(e) for e in edges)
        self.iedges = []
        for es in edges:
            row = []
            for ex, ey, eh in es:
                ix, iy = ex * self.den, ey * self.den
                assert ix == int(ix) and iy == int(iy), "edge is not a multiple of the sub-unit"
                row.append((int(ix), int(iy), int(eh)))
            self.iedges.append(row)
        self.edges = [list(map(tuple, es)) for es in edges]
        self.lengths = [list(map(float, ls)) for ls in lengths]
        self.S = 2 * self.max_val + 1

    def key_index(self, h, k):
        """Index of the mask of edge k taken from a node of heading h = q * nb + b."""
        return h * self.ne_max + k

    def arrays(self):
        """(edges float64 [nb, ne_max, 2], headings int32 [nb, ne_max], lengths float64 [nb, ne_max], counts int32 [nb]) for the C ABI."""
        e = np.zeros((self.nb, self.ne_max, 2))
        hd = np.zeros((self.nb, self.ne_max), np.int32)
        ln = np.zeros((self.nb, self.ne_max))
        cnt = np.zeros(self.nb, np.int32)
        for b in range(self.nb):
            cnt[b] = len(self.edges[b])
            for k, (ex, ey, eh) in enumerate(self.edges[b]):
                e[b, k], hd[b, k], ln[b, k] = (ex, ey), eh, self.lengths[b][k]
        return e, hd, ln, cnt


def succ_heading(h, eh, nb, nh):
    """The integer heading rule: quadrant of the node times nb plus the edge heading."""
    return ((h // nb) * nb + eh) % nh


def float_heading(h, eh, nb, nh):
    """The reference's rule (AStar.concat): int(((eh * spacing + h * spacing - spacing * b) % 2pi) / spacing) in floating point."""
    spacing = 2 * np.pi / nh
    b = h % nb
    heading = (eh * spacing + h * spacing - spacing * b) % (2 * np.pi)
    return int(heading / spacing)


def rot_edge(ex, ey, q):
    return ((ex, ey), (-ey, ex), (-ex, -ey), (ey, -ex))[q]


def pack_masks(masks):
    """bool [keys, S, S] -> int64 [keys, S]: bit c of word r is cell (row r, column c)."""
    masks = np.asarray(masks, bool)
    K, S, S2 = masks.shape
    assert S == S2 and S <= 64
    w = (masks.astype(np.uint64) << np.arange(S, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)
    return w.view(np.int64)


def unpack_masks(words, S):
    w = np.asarray(words).view(np.uint64)
    return ((w[..., None] >> np.arange(S, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def swath_cost(cost_map, word_rows, ix, iy, mv, lo, hi):
    """Sum of the map over the set bits of the mask centred on (ix, iy); +inf if a set bit leaves rows [lo, hi) or columns [0, W)."""
    W = cost_map.shape[1]
    rows = []
    for r, word in enumerate(word_rows):
        word = int(word) & 0xFFFFFFFFFFFFFFFF
        if not word:
            continue
        row = iy + r - mv
        if row < lo or row >= hi:
            return math.inf
        c0 = ix - mv
        rs = 0.0
        c = 0
        while word:
            if word & 1:
                col = c0 + c
                if col < 0 or col >= W:
                    return math.inf
                rs += float(cost_map[row, col])
            word >>= 1
            c += 1
        rows.append(rs)
    total = 0.0
    for rs in rows:
        total += rs
    return total


class Result:
    pass


def lattice_search(cost_map, start, goal_y, T, masks, weight=1.0, h_baseline=False, margin=0, max_expansions=1 << 30, node_capacity=1 << 30,
                   queue_capacity=1 << 30, max_path_nodes=1 << 30, reverse_ties=False):
    """One search.  masks: int64 / uint64 [keys, S] (pack_masks), keys indexed by Tables.key_index.  Returns a Result with status, g, expanded,
    n_nodes, nodes [n, 3] (X, Y, world heading), edges [n] (b * ne_max + k, -1 for the start), inodes [n] integer (i, j, h), and the statistics
    max_queue, improved (relaxations that lowered a queued node) and n_table (nodes ever seen).  reverse_ties pops the LARGEST key among equal f
    (only the golden maker uses it, to see whether a case depends on the tie rule)."""
    cost_map = np.asarray(cost_map, np.float64)
    H, W = cost_map.shape
    x0, y0, th0 = (float(v) for v in start)
    goal_y = float(goal_y)
    R = Result()
    R.status, R.g, R.expanded, R.n_nodes, R.nodes, R.edges, R.inodes = NO_PATH, math.inf, 0, 0, np.zeros((0, 3)), np.zeros(0, np.int32), []
    R.max_queue, R.improved, R.n_table = 0, 0, 0
    vals = (x0, y0, th0, goal_y)
    if not all(math.isfinite(v) and abs(v) <= COORD_MAX for v in vals) or not (0.0 <= x0 <= W and 0.0 <= y0 <= H):
        return R
    th0m = th0 % TWO_PI
    s0, c0 = sincos(th0m)
    u = T.unit / T.den
    spacing = TWO_PI / T.nh
    lo = max(0, int(y0) - margin)
    hi = min(H, int(goal_y) + margin)
    mv = T.max_val
    words = np.asarray(masks).view(np.uint64)

    def pos(i, j):
        a, b = i * u, j * u
        return x0 + (c0 * a - s0 * b), y0 + (s0 * a + c0 * b)

    def world_heading(h):
        t = h * spacing + th0m
        return t - TWO_PI if t >= TWO_PI else t

    def heur(X, Y, h):
        if h_baseline:
            return max(0.0, goal_y - Y)
        return dubins_h(X, Y, world_heading(h), goal_y, T.r, 0.0, float(W))

    def fscore(g, X, Y, h):
        f = g + weight * heur(X, Y, h) if weight else g
        return math.inf if f != f else f

    def key(i, j, h):
        return ((j + KEY_OFF) << 18) | ((i + KEY_OFF) << 5) | h

    sgn = -1 if reverse_ties else 1
    start_n = (0, 0, 0)
    g = {start_n: 0.0}
    parent, via, closed = {start_n: None}, {start_n: -1}, set()
    heap = [(fscore(0.0, x0, y0, 0), sgn * key(0, 0, 0), start_n)]
    R.max_queue = 1
    goal = None
    while heap:
        _, _, node = heapq.heappop(heap)
        if node in closed:
            continue
        i, j, h = node
        X, Y = pos(i, j)
        if Y >= goal_y:
            goal = node
            break
        if R.expanded >= max_expansions:
            R.status = CAP
            break
        closed.add(node)
        R.expanded += 1
        b, q = h % T.nb, h // T.nb
        ix, iy = int(X), int(Y)
        stop = False
        for k, (ex, ey, eh) in enumerate(T.iedges[b]):
            rx, ry = rot_edge(ex, ey, q)
            i2, j2, h2 = i + rx, j + ry, (q * T.nb + eh) % T.nh
            X2, Y2 = pos(i2, j2)
            if not (0.0 < X2 < W and 0.0 < Y2 < H):
                continue
            assert abs(i2) < KEY_LIM and abs(j2) < KEY_LIM
            n2 = (i2, j2, h2)
            if n2 in closed:
                continue
            sw = swath_cost(cost_map, words[T.key_index(h, k)], ix, iy, mv, lo, hi)
            t = (g[node] + sw) + T.lengths[b][k]
            if t < g.get(n2, math.inf):
                if n2 in g:
                    R.improved += 1
                elif len(g) >= node_capacity:
                    R.status, stop = CAP, True
                    break
                if len(heap) >= queue_capacity:
                    R.status, stop = CAP, True
                    break
                g[n2], parent[n2], via[n2] = t, node, b * T.ne_max + k
                heapq.heappush(heap, (fscore(t, X2, Y2, h2), sgn * key(i2, j2, h2), n2))
                R.max_queue = max(R.max_queue, len(heap))
        if stop:
            break
    R.n_table = len(g)
    if goal is None or goal == start_n:
        return R
    chain = [goal]
    while parent[chain[-1]] is not None:
        chain.append(parent[chain[-1]])
    if len(chain) > max_path_nodes:
        R.status = CAP
        return R
    chain.reverse()
    R.status, R.g, R.n_nodes, R.inodes = FOUND, g[goal], len(chain), chain
    R.nodes = np.array([pos(i, j) + (world_heading(h),) for i, j, h in chain])
    R.edges = np.array([via[n] for n in chain], np.int32)
    return R


def load_golden():
    import json
    G = np.load(os.path.join(GOLDEN, "lattice_golden.npz"))
    with open(os.path.join(GOLDEN, "lattice_golden.json")) as f:
        M = json.load(f)
    return G, M


def golden_rtol(n):
    """Non-negative terms: any summation order lies within (n - 1) * 2^-53 relative of the exact sum, two orders within twice that."""
    return 2 * n * 2.0 ** -53


def golden_map(seed, H=120, W=40):
    """Every cell drawn from (0.5, 10): no two partial costs tie (numpy's legacy RandomState: stable)."""
    return np.random.RandomState(seed).uniform(0.5, 10.0, (H, W))


def tables_from_prims(prims, max_val):
    """Tables of a planning.LatticePrimitives (or any object with edges, num_headings, scale, den, turning_radius, length(b, k))."""
    nb = prims.num_base_h
    return Tables(prims.edges, [[prims.length(b, k) for k in range(len(prims.edges[b]))] for b in range(nb)], prims.num_headings, prims.scale,
                  prims.den, max_val, prims.turning_radius)


def restated_masks(samples, counts, nh, ne_max, footprint, halves, theta0, max_val):
    """generate_swath (common/swath.py:15-88, planning branch) with the primitive rotated by theta0 + q * 90 deg itself, on the restated rasteriser:
    bool [nh * ne_max, S, S].  samples(b, k) -> [3, P] path of primitive k of base heading b; counts[b] edges; halves = the two widened ship halves."""
    from swath_ref import swath_ref
    nb, S = nh // 4, 2 * max_val + 1
    blank = np.zeros((S, S))
    out = np.zeros((nh * ne_max, S, S), bool)
    for h in range(nh):
        b, q = h % nb, h // nb
        rot = theta0 + q * (np.pi / 2)
        c, s = np.cos(rot), np.sin(rot)
        for k in range(counts[b]):
            sm = np.asarray(samples(b, k), np.float64)
            path = np.stack([c * sm[0] - s * sm[1] + float(max_val), s * sm[0] + c * sm[1] + float(max_val), np.remainder(sm[2] + rot, 2 * np.pi)], 1)
            m, _ = swath_ref(blank, path, footprint)
            for half in halves:
                cut, _ = swath_ref(blank, path[:1], half)
                m &= ~cut
            out[h * ne_max + k] = m
    return out
