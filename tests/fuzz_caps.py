"""Constructed ship-ice scenes that reach the fixed in-kernel capacities of the physics sub-step (DESIGN.md "In-kernel capacities") and the lane / stride
edges of its per-body loops; the scenes of tests/test_fuzz_caps_cpu.py (oracle alone: every scene hits what it names) and tests/test_gpu_fuzz_caps.py
(== with the oracle at and below a capacity, the documented flag and nothing else above it).

Like tests/fuzz_scenes.py: a scene is a trial dict in the reference's pickle schema, run with fuzz_params (ONE settle sub-step, 40 sub-steps per env step,
shape radius 0.02 or 0) for 3 env steps, so every contact exists from the first sub-step.  With the default collision slop of 0.1 m an overlap of up to
0.05 m produces no bias impulse: what does not touch the ship stays where it is put, as a cold arbiter that still holds its arbiter lane, its colour and
the velocity slots of its two bodies.  That makes the counts below exact by construction; the oracle confirms them in the CPU test.

One function per family, fixed seeds, the target value is an argument.  LEGAL[family] are the targets "two under, one under, exactly at" the capacity,
OVER[family] "one over, several over"; make_scenes() serves only the former, make_over_scenes() only the latter, so an over-capacity scene cannot get
into an at-capacity batch by accident.

  colours     a dynamic 20-gon hub whose edge towards the ship is overlapped by the bow and k - 1 further edges by one small box each (GAPS / TILTS of
              fuzz_scenes): k arbiters share the hub, the solve order needs k colours.  Capacity 16.
  neighbours  the same star with 3 .. 9 touching boxes and tiny boxes that touch nothing in the corners of the hub's AABB, so that the hub's Verlet list
              (fat AABBs: AABB grown by the skin; the ship counts) has n entries.  Capacity BP_KADJ = 24.
  lanes       a family-3 chain on the bow, a grid of touching boxes ahead of it (m x n: m (n - 1) + n (m - 1) links; with sharp corners, radius 0, the
              diagonal neighbours overlap in a corner as well: 2 (m - 1)(n - 1) more) and isolated touching pairs, n arbiters in all.  Capacity 64.
  slots       isolated touching pairs (one arbiter lane, two velocity slots each) and one box on the bow: slots are handed out to the bodies of every
              arbiter and never returned within a step, so 1 (ship) + 2 pairs + boxes on the bow are in use.  Capacity BP_NSLOT = 96.  This
              construction works for damping == 0 and != 0 alike; "many floes touched one after another" cannot be had in 3 steps of 2.4 cm.
  purge       the hub's list is full, two listed bars have since been driven out of fat overlap, a floe driven by the ship arrives: see purge_scene.
  pair_lanes, pair_slots   the last two families around the paired kernel's half-wave limits (32 lanes, 40 slots): below the solo capacities, so no
              flag may appear and the result equals the oracle; the env merely leaves its pair.  make_scenes() puts an ordinary small scene
              (fuzz_scenes.make_scene) into every other env, so the other half of a pair is ordinary.
  mid_lanes, mid_slots   midstep_scene: the last lane / slot is taken in the first env step, not in the settle sub-step, and one lane is held by a stale arbiter.
  maze        maze_lanes_layout: the lane capacity once through substep<BP_ENV_MAZE>, 62, 63, 64 | 65, 69 arbiters from a pile of overlapping boxes.
  edges       fields of nb = 63 .. 449 bodies (the ship is body 0), nearly all of them tiny boxes far from the ship; the bodies that collide -- the
              box on the bow and its two-contact parallel-edge partner, then a family-3 chain behind them, and a cold touching pair at the end of the
              field -- have indices that straddle 63|64 and 127|128 and end at nb - 1.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fuzz_scenes import GAPS, SHIP_HEAD, TILTS, _ob, _rect, _rot, fuzz_params, make_scene  # noqa: E402,F401

SUBSTEPS, STEPS = 40, 3
SKIN = 0.06                       # P.skin of the ship-ice handle (csrc/bp_capi.hip)
TOUCH = tuple(g for g in GAPS if g < 0)     # the GAPS that certainly touch
CAPACITY = {"colours": 16, "neighbours": 24, "lanes": 64, "slots": 96, "pair_lanes": 32, "pair_slots": 40}
LEGAL = {"colours": (14, 15, 16), "neighbours": (22, 23, 24), "lanes": (62, 63, 64), "slots": (94, 95, 96),
         "pair_lanes": (31, 32, 33, 36), "pair_slots": (39, 40, 41, 44)}
OVER = {"colours": (17, 18), "neighbours": (25, 27), "lanes": (65, 68), "slots": (97, 100)}
EDGE_NB = (63, 64, 65, 127, 128, 129, 192, 193, 448, 449)
HUB_EDGES = 20


def _ship(rng):
    th = math.pi / 2 + rng.uniform(-0.4, 0.4)
    sx, sy = rng.uniform(4.5, 7.5), rng.uniform(3.0, 5.0)
    bow = np.array([sx, sy]) + _rot(SHIP_HEAD, th)
    fwd = np.array([math.cos(th), math.sin(th)])
    return (float(sx), float(sy), float(th)), bow, fwd, np.array([-fwd[1], fwd[0]])


def _trial(ship_state, obs, **meta):
    t = {"ship_state": ship_state, "goal": (0.0, 9.0), "obstacles": obs}
    t.update(meta)           # what the scene is meant to reach; the loaders read the three keys above only
    return t


def _ordinary(seed, radius):
    sc = make_scene(seed, radius)
    return _trial(sc["ship_state"], sc["obstacles"], family="ordinary", target=0)


def _far_lattice(rng, n, y0=14.0, pitch=0.36):
    """n tiny boxes on a lattice far from the ship: no two fat AABBs meet, nothing ever moves."""
    out = []
    per_row = int((11.0 - 1.0) / pitch)
    for k in range(n):
        c = np.array([1.0 + pitch * (k % per_row), y0 + pitch * (k // per_row)]) + rng.uniform(-0.02, 0.02, 2)
        out.append(_ob(_rect(c, rng.uniform(0.05, 0.1), rng.uniform(0.05, 0.1), rng.uniform(0, math.pi))))
    return out


def _far_pairs(rng, npairs, radius, y0=14.0, pitch=0.5):
    """npairs isolated pairs of touching boxes far from the ship: one cold arbiter and two velocity slots each."""
    out = []
    per_row = int((11.0 - 1.0) / pitch)
    for k in range(npairs):
        c = np.array([1.0 + pitch * (k % per_row), y0 + pitch * (k // per_row)])
        phi = rng.uniform(0, math.pi)
        u = np.array([math.cos(phi), math.sin(phi)])
        w = rng.uniform(0.08, 0.12)
        gap = 2 * radius + TOUCH[int(rng.integers(len(TOUCH)))]
        off = np.array([-u[1], u[0]]) * rng.uniform(-0.03, 0.03)
        out += [_ob(_rect(c - u * (w + gap) / 2, w, rng.uniform(0.08, 0.12), phi)),
                _ob(_rect(c + u * (w + gap) / 2 + off, w, rng.uniform(0.08, 0.12), phi + TILTS[int(rng.integers(len(TILTS)))]))]
    return out


def star_scene(seed, radius, ntouch, nidle, family, target):
    """The hub of HUB_EDGES edges, overlapped by the bow, with `ntouch` boxes that touch one edge each and `nidle` tiny boxes inside its AABB that touch
    nothing: the hub has ntouch + 1 arbiters (as many colours) and ntouch + nidle + 1 neighbours."""
    rng = np.random.default_rng(seed)
    ship_state, bow, fwd, left = _ship(rng)
    th, n, rsum = ship_state[2], HUB_EDGES, 2 * radius
    R = rng.uniform(0.95, 1.1)
    apo, edge = R * math.cos(math.pi / n), 2 * R * math.sin(math.pi / n)
    c = bow + fwd * (apo + rsum + TOUCH[int(rng.integers(len(TOUCH)))])
    psi0 = th + math.pi                                    # direction from the hub's centre to the middle of the edge that faces the bow
    ang = psi0 - math.pi / n + 2 * math.pi * np.arange(n) / n
    hub = _ob(c + R * np.stack([np.cos(ang), np.sin(ang)], -1))
    free = [k for k in range(2, n - 1)]                    # not the bow's edge nor its two neighbours
    assert ntouch <= len(free)
    boxes, centres = [], []
    for k in rng.permutation(free)[:ntouch]:
        psi = psi0 + 2 * math.pi * k / n
        u = np.array([math.cos(psi), math.sin(psi)])
        hb = rng.uniform(0.06, 0.12)
        cb = c + u * (apo + hb / 2 + rsum + TOUCH[int(rng.integers(len(TOUCH)))]) + np.array([-u[1], u[0]]) * rng.uniform(-0.1, 0.1) * edge
        boxes.append(_ob(_rect(cb, hb, rng.uniform(0.5, 0.6) * edge, psi + TILTS[int(rng.integers(len(TILTS)))])))   # _rect's first side lies along u
        centres.append(cb)
    hv = hub["vertices"]
    lo, hi = hv.min(0) + 0.03, hv.max(0) - 0.03
    cand = rng.uniform(lo, hi, (20000, 2))
    d = cand - c
    cand = cand[(np.hypot(d[:, 0], d[:, 1]) > R + 0.1) & ~((d @ fwd < 0) & (np.abs(d @ left) < 0.75))]     # clear of the hub and of the ship's lane
    for p in cand:
        if len(centres) == ntouch + nidle:
            break
        if all(np.hypot(*(p - q)) >= (0.2 if i < ntouch else 0.075) for i, q in enumerate(centres)):
            centres.append(p)
            boxes.append(_ob(_rect(p, 0.02, 0.02, rng.uniform(0, math.pi))))
    assert len(centres) == ntouch + nidle, "no room for the idle neighbours"
    obs = boxes
    hub_at = int(rng.integers(0, len(obs) + 1))            # the hub's body index decides on which side of the pair keys it stands
    obs.insert(hub_at, hub)
    return _trial(ship_state, obs, family=family, target=target, hub=hub_at + 1)


def purge_scene(seed, radius):
    """The one branch of the list rebuild that only a FULL list reaches: a reciprocal insertion that first purges stale entries.  A diamond hub that nothing
    touches (so its own list is never rebuilt) has 24 neighbours after the settle sub-step: 20 idle tiny boxes in the two pockets of its AABB on the ship's side, and in each of
    the other two a heavy box Y with a thin bar X standing 0.32 m deep in its far side, X's fat AABB 2 cm inside the hub's.  The overlap is deeper than the slop, so
    the bias impulse drives X out of Y and away from the hub: 8 cm within the first env step (X's list is rebuilt 6 cm out; the hub's entry for it is stale
    from then on).  A floe Z stands 0.19 m deep in the ship's flank beside the bow, 3 cm short of the hub's fat AABB; the ship's infinite mass drives it
    towards the hub more slowly: under 5.5 cm in the first env step, over 7 cm after the third.  When Z's list is rebuilt the hub does not have it, the
    hub's list is full, the two stale bars are purged and Z goes in: no flag."""
    rng = np.random.default_rng(seed)
    rsum = 2 * radius
    sx, sy, th = float(rng.uniform(7.0, 8.0)), float(rng.uniform(3.0, 5.0)), math.pi / 2          # heading +y: the port flank is the line x = sx - 0.25
    zw, zh = rng.uniform(0.45, 0.55), rng.uniform(0.25, 0.35)
    zov = rng.uniform(0.185, 0.2) - rsum                       # penetration = overlap + radius sum
    zc = np.array([sx - 0.25 + zov - zw / 2, sy - rng.uniform(0.2, 0.5)])
    Z = _ob(_rect(zc, zw, zh, 0.0))
    r = rng.uniform(0.95, 1.05)                                # the hub: |x| + |y| <= r around hc, AABB [-r, r]^2
    hc = np.array([zc[0] - zw / 2 - radius - (2 * SKIN + rng.uniform(0.025, 0.035)) - radius - r, zc[1] + rng.choice([-1, 1]) * rng.uniform(0.25, 0.4)])
    hub = _ob(hc + r * np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], float))
    obs = []
    for (px, py) in ((-1, 1), (-1, -1)):                        # the two pockets away from the ship
        ys = rng.uniform(0.72, 0.78)                           # Y: a box of side ys; pocket coordinates (mirrored by px, py), the hub is |x| + |y| <= r
        depth = rng.uniform(0.31, 0.33) - rsum                 # penetration = overlap + radius sum
        xb = r + 2 * SKIN - 0.02 + 2 * radius                  # X's near end: its fat AABB reaches 2 cm into the hub's
        ytop = xb + depth                                      # Y's far side lies `depth` beyond X's near end
        ylo = ytop - ys
        xlo = max(r + 0.1 - ylo, 0.12)                         # Y's corner nearest the hub lies on |x| + |y| = r + 0.1
        xc = xlo + ys / 2 + rng.uniform(-0.03, 0.03)
        Yb = np.array([[xlo, ylo], [xlo + ys, ylo], [xlo + ys, ytop], [xlo, ytop]])
        Xb = np.array([[xc - 0.025, xb], [xc + 0.025, xb], [xc + 0.025, xb + 0.6], [xc - 0.025, xb + 0.6]])
        if rng.random() < 0.5:                                 # the same along the other axis
            Yb, Xb = Yb[:, ::-1], Xb[:, ::-1]
        obs += [_ob(hc + Yb * [px, py]), _ob(hc + Xb * [px, py])]
    stale = [len(obs) - 3, len(obs) - 1]
    used = [np.sign(o["vertices"].mean(0) - hc) for o in obs[::2]]
    centres = []
    cand = rng.uniform(-r + 0.03, r - 0.03, (20000, 2))
    cand = cand[(np.abs(cand).sum(1) > r + 0.1) & (cand[:, 0] < r - 0.1) & ~np.array([any((np.sign(c) == u).all() for u in used) for c in cand])]
    for p in cand:
        if len(centres) == 20:
            break
        if all(np.hypot(*(p - q)) >= 0.075 for q in centres):
            centres.append(p)
            obs.append(_ob(_rect(hc + p, 0.02, 0.02, rng.uniform(0, math.pi))))
    assert len(centres) == 20
    # body order: the hub, the bars and Z at random places
    order = list(rng.permutation(len(obs)))
    obs = [obs[i] for i in order]
    stale = [order.index(i) for i in stale]
    hub_at, z_at = sorted(int(v) for v in rng.integers(0, len(obs) + 1, 2))
    obs.insert(hub_at, hub)
    stale = [i + (1 if i >= hub_at else 0) for i in stale]
    z_at += 1
    obs.insert(z_at, Z)
    stale = [i + (1 if i >= z_at else 0) for i in stale]
    return _trial((sx, sy, th), obs, family="purge", target=24, hub=hub_at + 1, stale=[i + 1 for i in stale], arrives=z_at + 1)


def make_purge_scenes(radius, n=16):
    return [purge_scene(8000 + 10 * i + (1 if radius else 0), radius) for i in range(n)]


def colours_scene(seed, radius, k):
    return star_scene(seed, radius, k - 1, int(np.random.default_rng(seed + 77).integers(0, 4)) if k <= 16 else 0, "colours", k)


def neighbours_scene(seed, radius, n):
    ntouch = int(np.random.default_rng(seed + 78).integers(3, 10))
    return star_scene(seed, radius, ntouch, n - 1 - ntouch, "neighbours", n)


def grid_links(m, n, radius):
    return m * (n - 1) + n * (m - 1) + (0 if radius > 0 else 2 * (m - 1) * (n - 1))


def lanes_scene(seed, radius, target, family="lanes", max_slots=None):
    """`target` arbiters in all: a family-3 chain of k boxes on the bow (k arbiters, the ship's included; these are the ones that are solved, come apart
    and meet again while the lanes are full), a touching m x n grid ahead of it and isolated pairs.  The grid stands clear of the chain: the ship would
    shift the column it pushes along its neighbours and make new links, and the count would no longer be the construction's.  Velocity slots stay
    below their own capacity (pair_lanes: below the half-wave's 40 as well, so that the lanes alone decide what the paired kernels do)."""
    rng = np.random.default_rng(seed)
    ship_state, bow, fwd, left = _ship(rng)
    k = int(rng.integers(2, 5))
    shapes = [(m, n) for m in range(2, 7) for n in range(2, 8)
              if grid_links(m, n, radius) + k <= target and 1 + k + m * n + 2 * (target - k - grid_links(m, n, radius)) <= (max_slots or (38 if family == "pair_lanes" else 90))]
    m, n = shapes[int(rng.integers(len(shapes)))]
    rsum = 2 * radius
    phi = ship_state[2] + rng.choice([0.0, 1e-9, 0.02])
    u = np.array([math.cos(phi), math.sin(phi)])
    w = rng.uniform(0.25, 0.4)
    c = bow + u * (w / 2 + rsum - rng.uniform(1e-3, 0.03))
    chain = []
    for _ in range(k):
        chain.append(_ob(_rect(c, w, rng.uniform(0.3, 0.6), phi)))
        c = c + u * (w + rsum + TOUCH[int(rng.integers(len(TOUCH)))])
    gw, gh = rng.uniform(0.16, 0.24), rng.uniform(0.12, 0.2)
    pw, ph = gw + rsum - 1e-3, gh + rsum - 1e-3            # pitch: every link overlaps by 1 mm
    ga = rng.uniform(0, math.pi)
    gu = np.array([math.cos(ga), math.sin(ga)])
    gv = np.array([-gu[1], gu[0]])
    g0 = np.array([rng.uniform(4.0, 8.0), rng.uniform(10.5, 11.5)])
    grid = [_ob(_rect(g0 + gu * (ph * (r - (m - 1) / 2)) + gv * (pw * (q - (n - 1) / 2)), gh, gw, ga)) for r in range(m) for q in range(n)]
    obs = chain + grid + _far_pairs(rng, target - k - grid_links(m, n, radius), radius)
    order = rng.permutation(len(obs))
    return _trial(ship_state, [obs[i] for i in order], family=family, target=target, grid=(m, n))


def slots_scene(seed, radius, target, family="slots"):
    """Isolated touching pairs and one box (target even) or none (odd) on the bow: 1 + 2 pairs + boxes on the bow velocity slots."""
    rng = np.random.default_rng(seed)
    ship_state, bow, fwd, left = _ship(rng)
    onbow = 1 - target % 2
    obs = _far_pairs(rng, (target - 1 - onbow) // 2, radius)
    if onbow:
        a = rng.uniform(0.3, 0.6)
        obs.append(_ob(_rect(bow + fwd * (a / 2 + 2 * radius - rng.uniform(1e-3, 0.03)) + left * rng.uniform(-0.1, 0.1), a, a, ship_state[2])))
    order = rng.permutation(len(obs))
    return _trial(ship_state, [obs[i] for i in order], family=family, target=target)


def edges_scene(seed, radius, nb):
    """nb bodies (ship included).  The chain on the bow -- box A, its parallel-edge partner B with two contacts, then up to four boxes behind B -- takes the
    body indices 63|64 and 126 .. 129 where the field has them and the last ones below; a cold touching pair sits at nb - 2, nb - 1 in the larger fields."""
    rng = np.random.default_rng(seed)
    ship_state, bow, fwd, left = _ship(rng)
    rsum = 2 * radius
    if nb >= 130:
        idx = [63, 64, 126, 127, 128, 129]
    elif nb >= 127:
        idx = [63, 64] + list(range(nb - 4, nb))
    elif nb >= 65:
        idx = [63, 64]
    else:
        idx = [nb - 2, nb - 1]
    tail = [nb - 2, nb - 1] if nb >= 190 else []
    phi = ship_state[2] + rng.choice([0.0, 1e-9, 0.02])
    u = np.array([math.cos(phi), math.sin(phi)])
    w = rng.uniform(0.25, 0.4)
    c = bow + u * (w / 2 + rsum - rng.uniform(1e-3, 0.03))
    chain = []
    for k in range(len(idx)):
        off = np.array([-u[1], u[0]]) * (rng.uniform(0.2, 0.4) * (1 if rng.random() < 0.5 else -1) if k == 1 else 0.0)   # B: partial tangential overlap
        chain.append(_ob(_rect(c + off, w, rng.uniform(0.5, 0.8), phi + (TILTS[int(rng.integers(len(TILTS)))] if k == 1 else 0.0))))
        c = c + u * (w + rsum + TOUCH[int(rng.integers(len(TOUCH)))])
    special = dict(zip(idx, chain))
    special.update(zip(tail, _far_pairs(rng, 1, radius, y0=11.0)))
    far = iter(_far_lattice(rng, nb - 1 - len(special)))
    obs = [special[i] if i in special else next(far) for i in range(1, nb)]
    return _trial(ship_state, obs, family="edges", target=nb, contact_idx=idx, tail_idx=tail)


_MAKERS = {"colours": colours_scene, "neighbours": neighbours_scene, "lanes": lanes_scene, "slots": slots_scene,
           "pair_lanes": lambda s, r, t: lanes_scene(s, r, t, "pair_lanes"), "pair_slots": lambda s, r, t: slots_scene(s, r, t, "pair_slots")}
_BASE = {"colours": 1000, "neighbours": 2000, "lanes": 3000, "slots": 4000, "pair_lanes": 5000, "pair_slots": 6000, "edges": 7000}


def make_scenes(family, radius, per_target=6):
    """The at- and below-capacity scenes of a family: per_target scenes for each value of LEGAL[family], in turn.  The pair_* families alternate with ordinary
    small scenes."""
    out = []
    for i in range(per_target):
        for t in LEGAL[family]:
            out.append(_MAKERS[family](_BASE[family] + 100 * t + 10 * i + (1 if radius else 0), radius, t))
            if family.startswith("pair_"):
                out.append(_ordinary(len(out), radius))
    return out


def make_over_scenes(family, radius, per_target=4):
    """[ordinary, over, ordinary, over, ..., ordinary]: the over-capacity scenes of a family (OVER[family]), each between two ordinary small scenes."""
    out = [_ordinary(0, radius)]
    for i in range(per_target):
        for t in OVER[family]:
            out.append(_MAKERS[family](_BASE[family] + 100 * t + 10 * i + (1 if radius else 0), radius, t))
            out.append(_ordinary(len(out), radius))
    return out


def make_edge_batches(radius, per_nb=2):
    """Batches of field scenes that share a handle, by the body capacity the handle gets (nb rounded up to a multiple of 8): up to 192 (moving list of
    192), 193 (-> 200: the moving list grows with the field), 448 (the largest the paired kernel is built for) and 449 (-> 456: pairing refused).  Every
    batch also holds a scene without any floe."""
    groups = {192: [n for n in EDGE_NB if n <= 192], 200: [193, 65], 448: [448, 129], 456: [449, 64]}
    out = {}
    for cap, nbs in groups.items():
        sc = [edges_scene(_BASE["edges"] + 10 * nb + i + (5 if radius else 0), radius, nb) for nb in nbs for i in range(per_nb)]
        empty = _trial(_ship(np.random.default_rng(cap))[0], [], family="edges", target=1, contact_idx=[], tail_idx=[])
        out[cap] = [empty] + sc
    return out


MID_LEGAL = {"lanes": (63, 64), "slots": (95, 96)}
MID_OVER = {"lanes": (65,), "slots": (97,)}


def _gadget(g0, radius, catch, gap):
    """Contacts that change in the middle of a step, driven by a bias impulse: a plate X (1.1 x 0.6) stands 0.32 m deep in the top of a box Y (0.75) and is
    driven upwards out of it from the first sub-step on.  `catch`: a small box S under X's overhang touches X by 1 mm and loses it in the first sub-step; its
    arbiter stays cached for the three sub-steps of the persistence and holds its lane.  A small box T waits `gap` above X: 2 mm -- X meets it while S's stale
    arbiter still holds a lane --, 1 cm -- a few sub-steps later.  T's arbiter and T's velocity slot are new in the first env step, not in the settle sub-step."""
    rsum = 2 * radius
    xb = g0[1] + 0.375 - (0.32 - rsum)                       # X's lower side
    obs = [_ob(_rect(g0, 0.75, 0.75, 0.0)), _ob(_rect((g0[0], xb + 0.3), 1.1, 0.6, 0.0))]
    if catch:
        obs.append(_ob(_rect((g0[0] + 0.48, xb - rsum + 1e-3 - 0.05), 0.1, 0.1, 0.0)))
    obs.append(_ob(_rect((g0[0], xb + 0.6 + rsum + gap + 0.05), 0.1, 0.1, 0.0)))
    return obs


def midstep_scene(seed, radius, kind, target, max_slots=None):
    """A capacity that is reached (or passed) only while a step runs.  lanes: a lanes_scene of target - 3 arbiters and the gadget with S: target - 1 lanes after
    the settle sub-step, `target` in the first step, one of them held by a stale arbiter (fewer active arbiters than lanes).  slots: a slots_scene of
    target - 3 slots and the gadget without S: Y and X hold slots from the settle sub-step, T takes the last one in the first step."""
    rng = np.random.default_rng(seed + 5)
    g0 = np.array([1.3, 8.0]) + rng.uniform(0, 0.2, 2)
    base = lanes_scene(seed, radius, target - 3, max_slots=max_slots) if kind == "lanes" else slots_scene(seed, radius, target - 3)
    obs = base["obstacles"] + _gadget(g0, radius, kind == "lanes", 0.002 if kind == "lanes" else 0.01)
    order = rng.permutation(len(obs))
    return _trial(base["ship_state"], [obs[i] for i in order], family="mid_" + kind, target=target)


def make_midstep_scenes(kind, radius, per_target=4):
    return [midstep_scene(8500 + 100 * t + 10 * i + (1 if radius else 0), radius, kind, t) for i in range(per_target) for t in MID_LEGAL[kind]]


def make_midstep_over_scenes(kind, radius, per_target=4):
    out = [_ordinary(0, radius)]
    for i in range(per_target):
        for t in MID_OVER[kind]:
            out += [midstep_scene(8500 + 100 * t + 10 * i + (1 if radius else 0), radius, kind, t), _ordinary(len(out) + 1, radius)]
    return out


PAIR_KEYS, PAIR_SLOTS = 26, 34           # the limits at which an env leaves its pair inside the scheduler (BP_PP_KEYS, BP_PP_SLOTS; csrc/bp_capi.hip)


def make_pair_leave_scenes(radius, leave, n=4):
    """For the scheduler's pairs (BP_PAIR=2): envs that are admitted to a pair -- exactly 26 arbiter lanes, or exactly 34 velocity slots, after the settle
    sub-step, the other count well inside -- and, with leave=True, pass that limit by one in the first env step (midstep_scene), so that they leave their pair
    while it runs; with leave=False the same counts without the gadget, which stay where they are.  Every other env is an ordinary small scene."""
    out = []
    for i in range(n):
        for kind, lim in (("lanes", PAIR_KEYS), ("slots", PAIR_SLOTS)):
            seed = 8700 + 20 * i + (1 if radius else 0) + (10 if kind == "slots" else 0)
            if leave:
                sc = midstep_scene(seed, radius, kind, lim + 1, max_slots=PAIR_SLOTS - 6)
            else:
                sc = lanes_scene(seed, radius, lim, max_slots=PAIR_SLOTS - 6) if kind == "lanes" else slots_scene(seed, radius, lim)
            out += [_trial(sc["ship_state"], sc["obstacles"], family="pair_leave_" + kind, target=lim + (1 if leave else 0)), _ordinary(len(out) + 1, radius)]
    return out


MAZE_LEGAL, MAZE_OVER, MAZE_BOXES, MAZE_HALF = (62, 63, 64), (65, 69), 20, 0.5


def maze_lanes_layout(seed, target, walls):
    """maze-NAMO-v0 (substep<BP_ENV_MAZE>), its 20 axis-parallel boxes of 1 m x 1 m dropped where the caller likes: `target` arbiters after the settle
    sub-step.  A pile: 2 x 8 boxes (2 x 9 for target 69) on a lattice of pitch 0.45 m in the left room, so that every two boxes at most two lattice steps
    apart overlap (9 m - 12 pairs for m columns: 60, 69) and boxes three steps apart stay 0.35 m clear -- overlaps deeper than the slop, so the bias impulses
    drive the pile apart from the first sub-step on and its arbiters age out of the lanes while the step runs; and in the right room the other boxes as cold
    touching figures: two pairs (2 links), a triangle (3), a triangle with a fourth box on its side (4), two triangles on one base (5), for 69 nothing."""
    rng = np.random.default_rng(seed)
    m = 9 if target == 69 else 8
    extra = target - (9 * m - 12)
    o = np.array([1.6, 2.2]) + rng.uniform(0, 0.3, 2)
    c = [o + 0.45 * np.array([q, r]) + rng.uniform(-0.01, 0.01, 2) for r in range(2) for q in range(m)]
    p = 2 * MAZE_HALF + 0.04 + np.array([TOUCH[int(i)] for i in rng.integers(0, len(TOUCH), 4)])     # touching pitches (shape radius 0.02)
    a = np.array([9.3, 2.5]) + rng.uniform(0, 0.3, 2)
    b, up, down = a + [p[0], 0], a + [p[0] / 2, p[1]], a + [p[0] / 2, -p[2]]
    far = [np.array([9.5, 7.0]), np.array([12.0, 7.0])]
    if m == 9:
        assert extra == 0
        c += far
    else:
        c += {2: [a, b, a + [0, 4.0], b + [0, 4.0]], 3: [a, b, up, far[0]], 4: [a, b, up, b + [p[3], 0]], 5: [a, b, up, down]}[extra]
    order = rng.permutation(MAZE_BOXES)
    start = np.array([rng.uniform(2.0, 5.0), rng.uniform(11.5, 13.0), rng.uniform(-math.pi, math.pi)])
    return {"centres": np.array(c)[order], "walls": np.array(walls, np.float64), "start": start, "family": "maze_lanes", "target": target}


def maze_ordinary_layout(seed, walls):
    """An ordinary maze layout: the boxes spread over both rooms, a few of them right at the robot."""
    rng = np.random.default_rng(seed)
    start = np.array([rng.uniform(2.0, 5.0), rng.uniform(11.5, 13.0), rng.uniform(-math.pi, math.pi)])
    c = np.stack([rng.uniform(1.0, 14.0, MAZE_BOXES), rng.uniform(1.0, 10.5, MAZE_BOXES)], -1)
    k = int(rng.integers(1, 4))
    c[:k] = start[:2] + rng.uniform(-1.2, 1.2, (k, 2))
    return {"centres": c, "walls": np.array(walls, np.float64), "start": start, "family": "ordinary", "target": 0}


def make_maze_layouts(walls, per_target=6):
    return [maze_lanes_layout(9000 + 100 * t + i, t, walls) for i in range(per_target) for t in MAZE_LEGAL]


def make_maze_over_layouts(walls, per_target=2):
    out = [maze_ordinary_layout(9900, walls)]
    for i in range(per_target):
        for t in MAZE_OVER:
            out += [maze_lanes_layout(9000 + 100 * t + i, t, walls), maze_ordinary_layout(9901 + len(out), walls)]
    return out


def actions_for(n, seed=11):
    return np.random.default_rng(seed).uniform(-1, 1, (STEPS, n)).astype(np.float32).astype(np.float64)


def fat_neighbours(bodies_aabb, i, radius):
    """Entries of body i's Verlet list if it were rebuilt now: bodies whose AABB (grown by the shape radius and the skin) meets body i's."""
    lo, hi = bodies_aabb[:, 0] - radius - SKIN, bodies_aabb[:, 1] + radius + SKIN
    ov = (lo[i] <= hi).all(1) & (lo <= hi[i]).all(1)
    ov[i] = False
    return int(ov.sum())
