"""Ship poses and floe fields for the differential fuzz of the observation and cost-map rasterisers (tests/test_gpu_fuzz_obs.py), and maze layouts for
the maze observation.

The parity tests compare k_observe / k_observe_global / k_costmap / k_observe_maze with the oracle along rollouts that start at x = 8-10 m, y = 1 m, heading
pi/2.  This generator aims at what such rollouts never reach: windows that hang over every border of the map, a bow or stern outside it, 33-96 floes in
the window, floes with negative coordinates, and vertices / edge crossings that sit on a raster row or a pixel centre (corners on the 1/25 m lattice: one
raster pixel is 1/25 m).  A scene is a trial dict in the reference's pickle schema, as in fuzz_scenes.py, plus scene['fuzz'] = {'family': ...}.

Family = seed % 6:
  0  ship centre x in (0.05, 2.9)                      window columns < 0
  1  x in (9.1, 11.95)                                 window columns >= Wg
  2  y in (0.05, 0.95) or (35.1, 39.95)                window rows < 0 / >= Hg
  3  within 1 m of a border, heading within 0.5 rad of its outward normal, one in four with the centre up to 0.5 m outside the map
  4  interior pose, 33-96 small floes in the 6 m x 6 m window (a jittered 0.5 m grid; none overlaps another)
  5  interior pose, cost-map floes of radius 0.3-1.2 m over the whole map, several straddling x = 0, x = 12, y = 0
"""
import math

import numpy as np

from fuzz_scenes import _blob, _ob, _rect, fuzz_params  # noqa: F401  (fuzz_params: for the tests that import this module)

MAP_W, MAP_H = 12.0, 40.0      # configs/ship_ice.yaml: occ.map_width / map_height
PIX = 25                       # occ.m_to_pix_scale: raster pixels per metre
WIN, VSHIFT = 6.0, 2.0         # the egocentric window (local_w = local_h) and its forward shift
GAP = 0.08                     # clearance between floes that must not touch (twice the shape radius 0.02, and some)
OBS_SCENES, OBS_BASE_SEED, MAZE_LAYOUTS = 384, 0, 192   # the default batch: tests/test_fuzz_poses_cpu.py asserts what it covers
# cost-map configurations of the fuzz: (scale, m, n, alpha, ship_mass, horizon, margin, vs); ship_pos_y is per env, y * scale - 1
COSTMAP_CONFIGS = ((1, 40, 12, 10, 1, None, 1, 1.3), (2.5, 40, 12, 10, 1, 3, 0, 2.0), (5, 76, 12, 10, 1, None, 3, 1.50000001), (8, 40, 12, 2.5, 3.0, 8, 2, 0.7))
DIRS = ((1, 0), (0, 1), (1, 1), (1, -1), (1, 2), (2, 1), (1, -2), (2, -1), (2, 3), (3, 2), (2, -3), (3, -2))   # lattice edge directions: slopes 1:1, 1:2, 2:3


def _heading(rng):
    """Uniform in (-pi, pi], one in four exactly 0, +-pi/2 or pi."""
    if rng.random() < 0.25:
        return (0.0, math.pi / 2, -math.pi / 2, math.pi)[int(rng.integers(4))]
    return -rng.uniform(-math.pi, math.pi)


def _bound(v):
    v = np.asarray(v, np.float64)
    c = v.mean(0)
    return c, float(np.sqrt(((v - c) ** 2).sum(1)).max())


def _lattice_rect(rng, pos):
    """Axis-parallel rectangle whose corners are multiples of 1/25 m."""
    i, j = int(round(pos[0] * PIX)), int(round(pos[1] * PIX))
    a, b = int(rng.integers(2, 14)), int(rng.integers(2, 14))
    k = np.array([[i, j], [i + a, j], [i + a, j + b], [i, j + b]], np.float64)
    return k / PIX


def _lattice_poly(rng, pos):
    """Triangle or parallelogram with corners on the 1/25 m lattice and edges along two of DIRS: such an edge passes through pixel centres on rows that
    hold no vertex."""
    i, j = int(round(pos[0] * PIX)), int(round(pos[1] * PIX))
    while True:
        d1, d2 = DIRS[int(rng.integers(len(DIRS)))], DIRS[int(rng.integers(len(DIRS)))]
        if d1[0] * d2[1] - d1[1] * d2[0] != 0:
            break
    m, n = int(rng.integers(2, 6)), int(rng.integers(2, 6))
    p0 = np.array([i, j])
    a, b = m * np.array(d1), n * np.array(d2)
    k = [p0, p0 + a, p0 + b] if rng.random() < 0.5 else [p0, p0 + a, p0 + a + b, p0 + b]
    return np.array(k, np.float64) / PIX


def _floe(rng, pos, rlo, rhi):
    """One floe of a random kind at `pos`: (vertices, bounding circle)."""
    kind = rng.random()
    if kind < 0.32:
        v = _blob(rng, pos, rng.uniform(rlo, rhi))["vertices"]
    elif kind < 0.4:
        v = _rect(pos, rng.uniform(rlo, 2 * rhi), rng.uniform(rlo, 2 * rhi), rng.uniform(0, math.pi))    # a rectangle off the lattice, any angle
    elif kind < 0.7:
        v = _lattice_rect(rng, pos)
    else:
        v = _lattice_poly(rng, pos)
    return v, _bound(v)


def _round_floe(rng, centre, r):
    """6..14 points near a circle of radius r, evenly spread: a floe that fills most of its circle (cost-map cells are up to 1 m wide)."""
    n = int(rng.integers(6, 15))
    ang = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) * (2 * math.pi / n)
    rad = r * rng.uniform(0.8, 1.0, n)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1) + np.asarray(centre)


def _free(placed, c, r):
    return all((c[0] - p[0]) ** 2 + (c[1] - p[1]) ** 2 > (r + p[2] + GAP) ** 2 for p in placed)


def _scatter(rng, obs, placed, n, lo, hi, rlo, rhi, tries=8):
    """Up to n floes of random kinds in the box [lo, hi], none touching a floe placed before."""
    for _ in range(n):
        for _ in range(tries):
            pos = rng.uniform(lo, hi)
            v, (c, r) = _floe(rng, pos, rlo, rhi)
            if _free(placed, c, r):
                obs.append(_ob(v))
                placed.append((c[0], c[1], r))
                break


def _straddlers(rng, obs, placed, n, axis, at, lo, hi, rlo=0.35, rhi=0.6):
    """n blobs whose centre lies 0.02-0.3 m beyond the border `at` of coordinate `axis` (negative coordinates for at = 0) and which reach back into the map."""
    for _ in range(n):
        for _ in range(8):
            pos = np.zeros(2)
            pos[axis] = at + (-1.0 if at == 0.0 else 1.0) * rng.uniform(0.02, 0.3)
            pos[1 - axis] = rng.uniform(lo, hi)
            v = _blob(rng, pos, rng.uniform(rlo, rhi))["vertices"]
            c, r = _bound(v)
            if _free(placed, c, r):
                obs.append(_ob(v))
                placed.append((c[0], c[1], r))
                break


def make_obs_scene(seed):
    rng = np.random.default_rng(seed)
    fam = seed % 6
    th = _heading(rng)
    x, y = rng.uniform(3.5, 8.5), rng.uniform(2.0, 30.0)      # interior pose (families 4 and 5)
    if fam == 0:
        x = rng.uniform(0.05, 2.9)
    elif fam == 1:
        x = rng.uniform(9.1, 11.95)
    elif fam == 2:
        x = rng.uniform(0.5, 11.5)
        y = rng.uniform(0.05, 0.95) if rng.random() < 0.5 else rng.uniform(35.1, 39.95)
    elif fam == 3:
        side = (seed // 6) % 4                                  # x = 0, x = 12, y = 0, y = 40
        d = -rng.uniform(0.0, 0.5) if (seed // 24) % 4 == 0 else rng.uniform(0.0, 1.0)   # distance of the centre from the border, negative: outside
        th = (math.pi, 0.0, -math.pi / 2, math.pi / 2)[side] + rng.uniform(-0.5, 0.5)
        if rng.random() < 0.25:
            th += math.pi                                       # stern first
        th = math.atan2(math.sin(th), math.cos(th))
        if side < 2:
            x, y = (d if side == 0 else MAP_W - d), rng.uniform(1.5, 34.0)
        else:
            x, y = rng.uniform(1.0, 11.0), (d if side == 2 else MAP_H - d)
    wlo = np.array([x - WIN / 2, y + VSHIFT - WIN / 2])       # the window in metres
    obs, placed = [], []
    if fam == 4:
        # 33-96 candidates: cells of a 12 x 12 grid of pitch 0.5 m inside the window, each floe within 0.22 m of its cell centre; a few larger floes across
        # the window's edge
        n = int(rng.integers(36, 61)) if (seed // 6) % 2 == 0 else int(rng.integers(68, 89))
        cells = rng.permutation(144)[:n]
        for cidx in cells:
            cc = wlo + 0.25 + 0.5 * np.array([cidx % 12, cidx // 12]) + rng.uniform(-0.08, 0.08, 2)
            kind = rng.random()
            if kind < 0.6:
                v = _blob(rng, cc, rng.uniform(0.05, 0.13))["vertices"]
            else:
                i, j = int(round(cc[0] * PIX)), int(round(cc[1] * PIX))
                a, b = int(rng.integers(1, 4)), int(rng.integers(1, 4))
                v = (np.array([[i - a, j - b], [i + a, j - b], [i + a, j + b], [i - a, j + b]], np.float64) if kind < 0.8
                     else np.array([[i - a, j - b], [i + a, j], [i - a + 1, j + b]], np.float64)) / PIX
            obs.append(_ob(v))
        for _ in range(int(rng.integers(0, 7))):
            s = int(rng.integers(4))
            t = rng.uniform(-0.2, WIN + 0.2)
            off = -0.26 if s % 2 == 0 else WIN + 0.26
            cc = wlo + (np.array([off, t]) if s < 2 else np.array([t, off]))
            v = _blob(rng, cc, rng.uniform(0.1, 0.2))["vertices"]
            c, r = _bound(v)
            if _free(placed, c, r):
                obs.append(_ob(v))
                placed.append((c[0], c[1], r))
    elif fam == 5:
        _straddlers(rng, obs, placed, int(rng.integers(2, 5)), 0, 0.0, y - 1.0, y + 6.0, 0.4, 1.0)
        _straddlers(rng, obs, placed, int(rng.integers(2, 5)), 0, MAP_W, y - 1.0, y + 6.0, 0.4, 1.0)
        _straddlers(rng, obs, placed, int(rng.integers(1, 4)), 1, 0.0, 0.5, 11.5, 0.4, 1.0)
        n = int(rng.integers(40, 52))
        for q in range(n):                                      # one in three within the planner's horizon of the ship, the others anywhere on the map
            lo, hi = (np.array([-0.3, -0.3]), np.array([MAP_W + 0.3, MAP_H])) if q % 3 else (np.array([-0.3, y - 1.0]), np.array([MAP_W + 0.3, y + 7.0]))
            for _ in range(16):
                pos, r = rng.uniform(lo, hi), rng.uniform(0.3, 1.2)
                v = _round_floe(rng, pos, r) if q % 4 else _blob(rng, pos, r)["vertices"]
                c, r = _bound(v)
                if _free(placed, c, r):
                    obs.append(_ob(v))
                    placed.append((c[0], c[1], r))
                    break
    else:
        if fam == 0 or (fam == 3 and x < 1.0):
            _straddlers(rng, obs, placed, int(rng.integers(1, 4)), 0, 0.0, wlo[1] + 0.3, wlo[1] + WIN - 0.3)
        if y < 1.0:
            _straddlers(rng, obs, placed, int(rng.integers(1, 4)), 1, 0.0, max(wlo[0], 0.0) + 0.3, min(wlo[0] + WIN, MAP_W) - 0.3)
        _scatter(rng, obs, placed, int(rng.integers(0, 54)), wlo - 0.6, wlo + WIN + 0.6, 0.1, 0.5)
        if rng.random() < 0.5:                                  # a few floes on the bow and on whatever lies there: contacts from the first sub-step
            bow = np.array([x + math.cos(th), y + math.sin(th)])
            for _ in range(int(rng.integers(1, 4))):
                obs.append(_blob(rng, bow + rng.uniform(-0.5, 0.5, 2), rng.uniform(0.12, 0.4)))
    return {"ship_state": (float(x), float(y), float(th)), "goal": (0.0, 9.0), "obstacles": obs, "fuzz": {"family": fam}}


def make_obs_scenes(n, base_seed=0):
    return [make_obs_scene(base_seed + i) for i in range(n)]


def make_overflow_scenes(base_seed=0):
    """Two scenes for the capacity flag of k_observe (OBS_MAXCAND = 96): 90 floes and 140 floes inside the window of an interior pose, on a 12 x 12 grid."""
    out = []
    for q, n in enumerate((90, 140)):
        rng = np.random.default_rng(base_seed + q)
        x, y, th = rng.uniform(4.0, 8.0), rng.uniform(3.0, 20.0), _heading(rng)
        wlo = np.array([x - WIN / 2, y + VSHIFT - WIN / 2])
        obs = []
        for cidx in rng.permutation(144)[:n]:
            cc = wlo + 0.25 + 0.5 * np.array([cidx % 12, cidx // 12]) + rng.uniform(-0.08, 0.08, 2)
            obs.append(_blob(rng, cc, rng.uniform(0.05, 0.13)))
        out.append({"ship_state": (float(x), float(y), float(th)), "goal": (0.0, 9.0), "obstacles": obs, "fuzz": {"family": 4}})
    return out


MAZE_BOXES = 20


def make_maze_layouts(n, version, base_seed=0):
    """Layouts of maze-NAMO-v0 (dict(centres, walls, start)) for the observation fuzz: the start anywhere in [0.3, W - 0.3] x [0.3, L - 0.3], a third of the
    headings exact multiples of pi/2 (the rotated sample coordinates are then integers), half of the 20 boxes centred on multiples of 1/16 m (their corners
    lie on pixel centres: 16 pixels per metre, box size 0.5 m), a few boxes on the robot, the others anywhere -- on walls, on each other."""
    from benchpush_amd.config import default_cfg, maze_walls, merge_user_cfg
    cfg = merge_user_cfg(default_cfg("maze_namo"), {"num_obstacles": MAZE_BOXES, "maze_version": version})
    cfg.env = cfg.env1 if version == 1 else cfg.env2
    width, length, nbox = float(cfg.env.width), float(cfg.env.length), MAZE_BOXES
    walls = np.array(maze_walls(cfg), np.float64)
    rng = np.random.default_rng(base_seed + 7000 * version)
    out = []
    for i in range(n):
        th = (0.0, math.pi / 2, math.pi, -math.pi / 2)[int(rng.integers(4))] if i % 3 == 0 else rng.uniform(-math.pi, math.pi)
        start = np.array([rng.uniform(0.3, width - 0.3), rng.uniform(0.3, length - 0.3), th])
        c = np.stack([rng.uniform(0.3, width - 0.3, nbox), rng.uniform(0.3, length - 0.3, nbox)], -1)
        k = int(rng.integers(0, 6))
        c[:k] = start[:2] + rng.uniform(-1.2, 1.2, (k, 2))
        c[nbox // 2:] = np.round(c[nbox // 2:] * 16) / 16
        out.append({"centres": c, "walls": walls, "start": start})
    return out
