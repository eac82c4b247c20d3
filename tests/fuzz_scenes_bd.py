"""Fuzzed box-delivery-v0 / area-clearing-v0 scenes for the differential fuzz of the fourth copy of the sub-step (tests/test_gpu_fuzz_bd.py).

The suite's parity tests for these two tasks play the scenes of the rejection-sampling generators (box_delivery_scenario.generate_boxes,
area_clearing_scenario.generate_trial): boxes that never start on each other, on a column, the divider, the robot or the receptacle.  This generator keeps
the static geometry of those modules (generate_boundary / static_shapes) and replaces only `start` and `boxes`.  Scene i belongs to family i % 4:

  0  unconstrained: every centre uniform over the range the reference draws from, no rejection, any heading; the robot anywhere in its range
  1  boxes on the robot: 1-4 boxes re-centred within NEAR of the robot (contacts with base, wheels and bumper from the first sub-step)
  2  constructed contacts: a box face parallel to a wall / a column, divider or wall-segment face / another box's face at a gap from GAPS and a relative
     angle from ANGLES, a vertex-to-vertex pair, a box pushed into a room corner (box-delivery: the three corner triangles of radius 0.02), and on the
     walled area-clearing layouts a box at the rounded end of a wall segment
  3  the task's own edges: box-delivery -- boxes straddling the receptacle's edges, two boxes wholly inside it, a box in front of the bumper of a robot
     aimed at the receptacle; area-clearing -- box centres and inner faces within EDGE_OFFS of a clearance-boundary edge, a box wholly outside at
     reset, a box in a corner of the outer boundary

Every centre STARTS inside the reference's own range.  That does not keep every box in the room: generate_boxes does not look at the corners, a centre on
a corner's triangles is a legal draw of the reference, and prevent_boundary_intersection then throws that box through the wall in the first sub-step (the
thin triangle's shortest way out).  Family 0 makes such draws (about 1 scene in 1000); the constructed corner box of family 2 is brought down the
diagonal ONTO the triangles instead, because a box INSIDE them would be thrown out in every scene and the family would test nothing else.  A trial carries, besides the scenario modules' keys, `fuzz`: {'family', 'constructs': [{'kind', 'boxes', ...}]} -- what was built, for the
tests of the generator itself.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from benchpush_amd import area_clearing_scenario as A
from benchpush_amd import box_delivery_scenario as S
from benchpush_amd.config import default_cfg

GAPS = (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-4)     # between the rounded surfaces of the two shapes
ANGLES = (0.0, 1e-12, 1e-9, 1e-4)                  # relative angle of the two facing faces
EDGE_OFFS = (0.0, 1e-9, -1e-9, 1e-3, -1e-3)        # area-clearing: signed distance (outward) from a clearance-boundary edge
STRADDLE_OFFS = (0.0, 1e-9, -1e-9, 1e-3, -1e-3, 0.1, -0.1)   # box-delivery: box centre relative to a receptacle edge
BOX_R = 0.02                                       # create_polygon's shape radius of a box (both tasks)


def _unit(a):
    return np.array([math.cos(a), math.sin(a)])


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


class _Room:
    """What the constructions need to know about one trial's static geometry."""

    def __init__(self, box_lo, box_hi, start_lo, start_hi, half, nbox, near, reach):
        self.box_lo, self.box_hi = np.array(box_lo, np.float64), np.array(box_hi, np.float64)
        self.start_lo, self.start_hi = np.array(start_lo, np.float64), np.array(start_hi, np.float64)
        self.half, self.nbox, self.near, self.reach = float(half), int(nbox), float(near), float(reach)
        self.walls = []      # faces (p0, p1, outward normal, shape radius): the room's own walls
        self.faces = []      # faces of columns / divider / wall segments / static obstacles
        self.corners = []    # (corner point, inward diagonal signs (sx, sy) rotated as given, inset, kind)
        self.wall_ends = []  # (end point, outward direction, shape radius) of area-clearing wall segments

    def in_box_range(self, c, tol=0.0):
        return bool(np.all(c >= self.box_lo - tol) and np.all(c <= self.box_hi + tol))


def bd_room(cfg, boundary):
    L, W, n = S.room_dims(cfg)
    half = float(cfg.boxes.box_size) / 2
    size = max(cfg.agent.length, cfg.agent.width)
    R = _Room((-L / 2 + half, -W / 2 + half), (L / 2 - half, W / 2 - half), (-L / 2 + size, -W / 2 + size), (L / 2 - size, W / 2 - size), half, n,
              near=0.6, reach=float(cfg.agent.front_bumper_vertices[0][0]))
    R.L, R.W = L, W
    R.walls = [((-L / 2, -W / 2), (-L / 2, W / 2), (1.0, 0.0), 0.0), ((L / 2, -W / 2), (L / 2, W / 2), (-1.0, 0.0), 0.0),
               ((-L / 2, -W / 2), (L / 2, -W / 2), (0.0, 1.0), 0.0), ((-L / 2, W / 2), (L / 2, W / 2), (0.0, -1.0), 0.0)]
    for ob in boundary:
        if ob["type"] in ("column", "divider"):
            (x, y), l, w = ob["position"], ob["length"], ob["width"]
            R.faces += [((x - l / 2, y - w / 2), (x + l / 2, y - w / 2), (0.0, -1.0), 0.0), ((x - l / 2, y + w / 2), (x + l / 2, y + w / 2), (0.0, 1.0), 0.0),
                        ((x - l / 2, y - w / 2), (x - l / 2, y + w / 2), (-1.0, 0.0), 0.0)]
            if ob["type"] == "column":
                R.faces.append(((x + l / 2, y - w / 2), (x + l / 2, y + w / 2), (1.0, 0.0), 0.0))
        elif ob["type"] == "corner":
            h = float(ob["heading"])
            c, s = math.cos(h), math.sin(h)
            R.corners.append((np.array(ob["position"], np.float64), np.array([c * 1 - s * -1, s * 1 + c * -1]), 0.0, "triangles"))   # the local (1, -1) diagonal
        elif ob["type"] == "receptacle":
            R.recept = (np.array(ob["position"], np.float64), float(ob["length"]))
    return R


def ac_room(cfg):
    lay = A.env_layout(cfg)
    ox0, ox1, oy0, oy1 = A._extent(lay.outer_boundary)
    bx0, bx1, by0, by1 = A._extent(lay.boundary)
    d = float(cfg.obstacle_size)
    R = _Room((ox0 + d, oy0 + d), (ox1 - d, oy1 - d), (bx0 + 0.5, by0 + 0.5), (bx1 - 0.5, by1 - 0.5), d, int(cfg.num_obstacles), near=1.0,
              reach=float(cfg.agent.front_bumper_vertices[0][0]))
    r = 0.1   # static_shapes: every static polygon of this task is rounded by 0.1
    R.walls = [((ox0, oy0), (ox0, oy1), (1.0, 0.0), r), ((ox1, oy0), (ox1, oy1), (-1.0, 0.0), r), ((ox0, oy0), (ox1, oy0), (0.0, 1.0), r),
               ((ox0, oy1), (ox1, oy1), (0.0, -1.0), r)]
    for w in (lay.walls if "walls" in lay else []):
        a, b = np.array(w[0], np.float64), np.array(w[1], np.float64)
        u = (b - a) / np.linalg.norm(b - a)
        nrm = np.array([-u[1], u[0]])
        for sg in (1.0, -1.0):
            R.faces.append((tuple(a + sg * 0.1 * nrm), tuple(b + sg * 0.1 * nrm), tuple(sg * nrm), r))
        R.wall_ends += [(a, -u, r), (b, u, r)]
    for so in (lay.static_obstacles if "static_obstacles" in lay else []):
        v = np.array(so, np.float64)
        cen = v.mean(0)
        for k in range(len(v)):
            p0, p1 = v[k], v[(k + 1) % len(v)]
            e = p1 - p0
            nrm = np.array([e[1], -e[0]]) / np.linalg.norm(e)
            if nrm @ ((p0 + p1) / 2 - cen) < 0:
                nrm = -nrm
            R.faces.append((tuple(p0), tuple(p1), tuple(nrm), r))
    for cx, sx in ((ox0, 1.0), (ox1, -1.0)):
        for cy, sy in ((oy0, 1.0), (oy1, -1.0)):
            R.corners.append((np.array([cx, cy]), np.array([sx, sy]), r + BOX_R, "outer"))
    bd = np.array(lay.boundary, np.float64)
    cen = bd.mean(0)
    R.edges = []
    for k in range(len(bd)):
        p0, p1 = bd[k], bd[(k + 1) % len(bd)]
        e = p1 - p0
        nrm = np.array([e[1], -e[0]]) / np.linalg.norm(e)
        if nrm @ ((p0 + p1) / 2 - cen) < 0:
            nrm = -nrm
        R.edges.append((p0, p1, nrm))
    R.boundary = bd
    return R


def box_corners(box, half):
    """World corners of a box [x, y, heading] (the polygon itself, without its radius)."""
    c, s = math.cos(box[2]), math.sin(box[2])
    loc = np.array([[half, half], [-half, half], [-half, -half], [half, -half]])
    return np.stack([c * loc[:, 0] - s * loc[:, 1], s * loc[:, 0] + c * loc[:, 1]], -1) + np.asarray(box[:2])


# ---- the pieces ----
def _uniform_boxes(rng, R, n):
    b = np.zeros((n, 3))
    b[:, 0] = rng.uniform(R.box_lo[0], R.box_hi[0], n)
    b[:, 1] = rng.uniform(R.box_lo[1], R.box_hi[1], n)
    b[:, 2] = rng.uniform(0, 2 * math.pi, n)
    return b


def _uniform_start(rng, R):
    return np.array([rng.uniform(R.start_lo[0], R.start_hi[0]), rng.uniform(R.start_lo[1], R.start_hi[1]), rng.uniform(0, 2 * math.pi)])


def _aim_start(rng, R, target, standoff):
    """A start pose whose bumper looks at `target` from `standoff` away (clipped into the robot's range; the heading stays)."""
    h = rng.uniform(0, 2 * math.pi)
    p = np.clip(np.asarray(target) - standoff * _unit(h), R.start_lo, R.start_hi)
    return np.array([p[0], p[1], h])


def _on_face(rng, R, face, margin):
    """A box whose face is parallel (to `angle`) to a static face, `gap` away from it: (box, gap, angle, face normal)."""
    p0, p1, nrm, r = (np.array(x, np.float64) if i < 3 else x for i, x in enumerate(face))
    gap, ang = _pick(rng, GAPS), _pick(rng, ANGLES)
    ln = np.linalg.norm(p1 - p0)
    t = (p1 - p0) / ln
    s = rng.uniform(min(margin, ln / 2), max(ln - margin, ln / 2))
    c = p0 + t * s + nrm * (r + BOX_R + R.half + gap)
    base = math.atan2(nrm[1], nrm[0])
    return np.array([c[0], c[1], base + ang]), gap, ang, base


def _construct_contacts(rng, R, boxes, walled):
    cons = []
    k = 0
    # a face parallel to a room wall
    b, gap, ang, base = _on_face(rng, R, _pick(rng, R.walls), 1.0 + R.half)
    boxes[k] = b; cons.append(dict(kind="wall", boxes=[k], gap=gap, angle=ang, normal=base)); k += 1
    # a face parallel to a column / divider / wall-segment / static-obstacle face (the plain rooms: a second wall)
    b, gap, ang, base = _on_face(rng, R, _pick(rng, R.faces if R.faces else R.walls), 0.0 if R.faces else 1.0 + R.half)
    if not R.in_box_range(b[:2]):     # a face that looks out of the room (the divider's far side never does; a wall segment's outer side may)
        b, gap, ang, base = _on_face(rng, R, _pick(rng, R.walls), 1.0 + R.half)
    boxes[k] = b; cons.append(dict(kind="face", boxes=[k], gap=gap, angle=ang, normal=base)); k += 1
    # two boxes face to face, partial tangential overlap
    ext = 2 * (2 * R.half + 2 * BOX_R) + 0.1
    phi = rng.uniform(0, 2 * math.pi)
    ca = rng.uniform(R.box_lo + ext, R.box_hi - ext)
    gap, ang = _pick(rng, GAPS), _pick(rng, ANGLES)
    off = rng.uniform(0.2, 0.8) * 2 * R.half * (1 if rng.random() < 0.5 else -1)
    cb = ca + _unit(phi) * (2 * R.half + 2 * BOX_R + gap) + _unit(phi + math.pi / 2) * off
    boxes[k] = [ca[0], ca[1], phi]; boxes[k + 1] = [cb[0], cb[1], phi + ang]
    cons.append(dict(kind="pair", boxes=[k, k + 1], gap=gap, angle=ang)); k += 2
    # vertex to vertex along a diagonal
    phi = rng.uniform(0, 2 * math.pi)
    ca = rng.uniform(R.box_lo + ext, R.box_hi - ext)
    dgl = _unit(phi + math.pi / 4)
    gap = _pick(rng, GAPS)
    lat = _pick(rng, (0.0, 1e-9, -1e-9, 1e-3))
    cb = ca + dgl * (2 * R.half * math.sqrt(2) + 2 * BOX_R + gap) + _unit(phi + 3 * math.pi / 4) * lat
    boxes[k] = [ca[0], ca[1], phi]; boxes[k + 1] = [cb[0], cb[1], phi + _pick(rng, (0.0, 1e-9, math.pi / 2))]
    cons.append(dict(kind="vertex", boxes=[k, k + 1], gap=gap, lateral=lat)); k += 2
    # a box in a room corner
    pos, sg, inset, ckind = _pick(rng, R.corners)
    h = _pick(rng, (0.0, 1e-9, 0.3, math.pi / 4))
    if ckind == "triangles":
        # box-delivery: the corner is filled by three triangles of radius 0.02 whose inner edges form a chamfer; the middle one lies on the line
        # x - y = 1 + S - C of the corner's frame.  The box comes down the diagonal until its nearest corner (or, turned by pi / 4, its face) is `gap` from
        # that edge's rounded surface, shifted along the edge so that it reaches a neighbouring triangle as well.  (A box whose CENTRE starts inside the
        # triangles is thrown through the wall by prevent_boundary_intersection in the first sub-step: see the module docstring.)
        gap = _pick(rng, GAPS + (-0.01, -0.03))
        dhat = -sg / math.sqrt(2)
        reach = max(float((box_corners([0.0, 0.0, h], R.half) @ dhat).max()), 0.0)
        dist = (1 + S._S - S._C) / math.sqrt(2) + 0.02 + BOX_R + reach + gap
        c = pos + sg * dist / math.sqrt(2) + np.array([sg[0], -sg[1]]) / math.sqrt(2) * rng.uniform(-0.15, 0.15)
        cons.append(dict(kind="corner", boxes=[k], gap=gap, corner=pos.tolist(), diagonal=sg.tolist()))
    else:
        gap = _pick(rng, GAPS)
        c = pos + sg * (inset + R.half + gap)
        h = _pick(rng, (0.0, 1e-9, 1e-4))
        cons.append(dict(kind="corner", boxes=[k], gap=gap, corner=pos.tolist(), diagonal=sg.tolist()))
    boxes[k] = [c[0], c[1], h]
    k += 1
    if walled and R.wall_ends:
        end, out, r = _pick(rng, R.wall_ends)
        gap = _pick(rng, GAPS)
        side = np.array([-out[1], out[0]])
        c = end + out * (r + BOX_R + R.half + gap) + side * rng.uniform(-0.1 - R.half, 0.1 + R.half)   # from face-on to corner-on the rounded end
        boxes[k] = [c[0], c[1], math.atan2(out[1], out[0]) + _pick(rng, (0.0, 1e-9, 1e-4, math.pi / 4))]
        cons.append(dict(kind="wall_end", boxes=[k], gap=gap, end=end.tolist())); k += 1
    return cons


def _bd_edges(rng, R, boxes):
    """Family 3 of box-delivery: returns (constructs, start)."""
    (rx, ry), size = R.recept
    cons = []
    # two boxes straddle the receptacle's two inner edges (x = rx - size/2 and y = ry - size/2)
    o0, o1 = _pick(rng, STRADDLE_OFFS), _pick(rng, STRADDLE_OFFS)
    boxes[0] = [rx - size / 2 + o0, ry + 0.4 + rng.uniform(-0.01, 0.01), rng.uniform(0, 2 * math.pi)]
    boxes[1] = [rx + 0.4 + rng.uniform(-0.01, 0.01), ry - size / 2 + o1, rng.uniform(0, 2 * math.pi)]
    cons.append(dict(kind="straddle", boxes=[0], axis=0, edge=rx - size / 2, off=o0))
    cons.append(dict(kind="straddle", boxes=[1], axis=1, edge=ry - size / 2, off=o1))
    # two boxes wholly inside: both are delivered by the first step that leaves them there
    boxes[2] = [rx - 0.33 + rng.uniform(-0.03, 0.03), ry - 0.33 + rng.uniform(-0.03, 0.03), rng.uniform(0, 2 * math.pi)]
    boxes[3] = [rx + 0.33 + rng.uniform(-0.03, 0.03), ry + 0.33 + rng.uniform(-0.03, 0.03), rng.uniform(0, 2 * math.pi)]
    cons.append(dict(kind="inside", boxes=[2, 3]))
    # the robot aimed at the receptacle, a box just in front of its bumper
    th = rng.uniform(0.2, math.pi / 2 - 0.2)
    dist = rng.uniform(1.7, 2.6)
    p = np.clip(np.array([rx, ry]) - dist * _unit(th), R.start_lo, R.start_hi)
    h = math.atan2(ry - p[1], rx - p[0]) + _pick(rng, (0.0, 1e-9, 0.05, -0.05))
    gap, ang = _pick(rng, GAPS), _pick(rng, ANGLES)
    c = p + _unit(h) * (R.reach + 2 * BOX_R + R.half + gap)      # bumper and box are both rounded by 0.02
    boxes[4] = [c[0], c[1], h + ang]
    cons.append(dict(kind="bumper", boxes=[4], gap=gap, angle=ang))
    return cons, np.array([p[0], p[1], h])


def _ac_edges(rng, R, boxes):
    """Family 3 of area-clearing: returns (constructs, start or None)."""
    cons = []
    k = 0
    for kind in ("centre_on_edge",) * 4 + ("face_on_edge",) * 2:
        p0, p1, nrm = _pick(rng, R.edges)
        off = _pick(rng, EDGE_OFFS)
        ln = np.linalg.norm(p1 - p0)
        s = rng.uniform(0.1, 0.9) * ln
        if kind == "centre_on_edge":
            c = p0 + (p1 - p0) / ln * s + nrm * off
            h = rng.uniform(0, 2 * math.pi)
        else:       # the box outside, its inner face parallel to the edge at `off`: > 0 cleared, < 0 not, 0 on the line
            c = p0 + (p1 - p0) / ln * s + nrm * (R.half + off)
            h = math.atan2(nrm[1], nrm[0])
        boxes[k] = [c[0], c[1], h]
        cons.append(dict(kind=kind, boxes=[k], off=off, p0=p0.tolist(), p1=p1.tolist(), normal=nrm.tolist())); k += 1
    # wholly outside at reset
    p0, p1, nrm = _pick(rng, R.edges)
    ln = np.linalg.norm(p1 - p0)
    c = p0 + (p1 - p0) / ln * rng.uniform(0.1, 0.9) * ln + nrm * rng.uniform(R.half * math.sqrt(2) + 0.05, R.half * math.sqrt(2) + 0.6)
    c = np.clip(c, R.box_lo, R.box_hi)
    boxes[k] = [c[0], c[1], rng.uniform(0, 2 * math.pi)]
    cons.append(dict(kind="outside", boxes=[k])); k += 1
    # in a corner of the outer boundary, touching both walls to within a gap of GAPS
    pos, sg, inset, _ = _pick(rng, R.corners)
    gap = _pick(rng, GAPS)
    c = pos + sg * (inset + R.half + gap)
    boxes[k] = [c[0], c[1], _pick(rng, (0.0, 1e-9, 1e-4))]
    cons.append(dict(kind="outer_corner", boxes=[k], gap=gap, corner=pos.tolist())); k += 1
    start = None
    if rng.random() < 0.5:      # the robot behind one of the edge boxes
        j = int(rng.integers(0, 6))
        start = _aim_start(rng, R, boxes[j, :2], R.reach + R.half + rng.uniform(0.05, 0.5))
    return cons, start


def _fuzz(rng, R, fam, task):
    boxes = _uniform_boxes(rng, R, R.nbox)
    start = _uniform_start(rng, R)
    cons = []
    if fam == 1:
        k = int(rng.integers(1, 5))
        rad = R.near * np.sqrt(rng.uniform(0, 1, k))
        ang = rng.uniform(0, 2 * math.pi, k)
        boxes[:k, :2] = np.clip(start[:2] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1), R.box_lo, R.box_hi)
        cons.append(dict(kind="on_robot", boxes=list(range(k))))
    elif fam == 2:
        cons = _construct_contacts(rng, R, boxes, walled=bool(R.wall_ends))
        if rng.random() < 0.5:   # the robot next to one of the constructed contacts, looking at it
            j = int(rng.integers(0, len(cons)))
            start = _aim_start(rng, R, boxes[cons[j]["boxes"][0], :2], R.reach + R.half + rng.uniform(0.05, 0.5))
    elif fam == 3:
        cons, st = _bd_edges(rng, R, boxes) if task == "bd" else _ac_edges(rng, R, boxes)
        start = start if st is None else st
    for b in boxes:
        assert R.in_box_range(b[:2]), ("a fuzzed box left the reference's range", b, fam)
    assert np.all(start[:2] >= R.start_lo) and np.all(start[:2] <= R.start_hi)
    return start, boxes, cons


ROOMS = 8   # distinct rooms per batch: a handle builds its configuration-space, distance and receptacle maps once per distinct static geometry (0.1 - 0.2 s each)


def make_bd_trials(cfg, n, seed):
    """n box-delivery trials; the room of scene i (its columns / divider) is the scenario module's own draw for RandomState(seed + (i // 4) % ROOMS): every
    room sees every family."""
    out = []
    for i in range(n):
        rs = np.random.RandomState(seed + (i // 4) % ROOMS)
        boundary, _ = S.generate_boundary(cfg, rs, S.random_start(cfg, rs))
        R = bd_room(cfg, boundary)
        start, boxes, cons = _fuzz(np.random.default_rng([seed, i]), R, i % 4, "bd")
        out.append(dict(start=start, boxes=boxes, boundary=boundary, statics=S.static_shapes(boundary), fuzz=dict(family=i % 4, constructs=cons)))
    return out


def make_ac_trials(cfg, n, seed):
    R = ac_room(cfg)
    statics = A.static_shapes(cfg)
    out = []
    for i in range(n):
        start, boxes, cons = _fuzz(np.random.default_rng([seed, i]), R, i % 4, "ac")
        out.append(dict(start=start, boxes=boxes, statics=statics, fuzz=dict(family=i % 4, constructs=cons)))
    return out


# ---- the cases of tests/test_gpu_fuzz_bd.py and their oracle side (no GPU, no torch: tests/test_fuzz_scenes_bd_cpu.py plays them too) ----
STEPS, STEP_LIMIT = 3, 300
_SWEEP = os.environ.get("BP_FUZZ_SCENES")      # BP_FUZZ_SCENES=<n> for a longer one-off sweep (the floors below scale with n)

# (task, layout, action type, scenes, seed, floors): the floors are HALF of what the oracle alone shows on these seeds (oracle run on the CPU, counts in
# the comments), over the scenes of the case: scenes with work > 0 in some step, scenes whose robot hit a wall / column in some step, env steps that ran
# into STEP_LIMIT, and boxes delivered (box-delivery) or scenes that end with box_count > 0 (area-clearing)
# A floor of 0 asserts nothing, and says so here once for all of them: the velocity cases never reach STEP_LIMIT (a velocity step is 100 sim steps), and in
# small_empty, clear_env_small, clear_env and walled_env the robot (almost) never touches a wall within three steps (half of 1 or 0 is 0).  Wall hits are
# held by the three cases with columns or the divider, STEP_LIMIT by the six heading / position cases.
CASES = {
    "bd-small_columns-heading": ("bd", "small_columns", "heading", 96, 11000, dict(work=44, hit=7, limited=130, task=31)),   # oracle: 88 scenes with work, 15 with a hit, 261 limited steps, 63 boxes delivered
    "bd-large_divider-heading": ("bd", "large_divider", "heading", 48, 12100, dict(work=23, hit=3, limited=67, task=14)),   # oracle: 47, 6, 134, 28
    "bd-small_empty-position": ("bd", "small_empty", "position", 96, 13000, dict(work=44, hit=0, limited=140, task=31)),   # oracle: 88, 1, 280, 63
    "bd-large_columns-velocity": ("bd", "large_columns", "velocity", 48, 14000, dict(work=23, hit=2, limited=0, task=17)),   # oracle: 46, 5, 0 (a velocity step is 100 sim steps), 35
    "ac-clear_env_small-heading": ("ac", "clear_env_small", "heading", 96, 21000, dict(work=45, hit=0, limited=144, task=48)),   # oracle: 91, 0 (the walls are 2 m outside the robot's range), 288, 96
    "ac-walled_env_with_columns-position": ("ac", "walled_env_with_columns", "position", 96, 22000, dict(work=32, hit=18, limited=123, task=48)),   # oracle: 65, 36, 246, 96
    "ac-clear_env-velocity": ("ac", "clear_env", "velocity", 96, 23000, dict(work=34, hit=0, limited=0, task=48)),   # oracle: 68, 0, 0, 96
    "ac-walled_env-heading": ("ac", "walled_env", "heading", 96, 24000, dict(work=39, hit=0, limited=144, task=48)),   # oracle: 79, 0, 288, 96
}

def case_setup(case, damping=0.0, nscenes=None, seed=None):
    """(cfg, cfg overrides for the env, scenes, actions [STEPS, E(, 2)], oracle factory) of a case."""
    task, layout, atype, n, seed0, _ = CASES[case]
    n = int(nscenes or _SWEEP or n)
    seed = seed0 if seed is None else seed
    if task == "bd":
        cfg = default_cfg("box_delivery")
        cfg.env.obstacle_config = layout
        over = {"env": {"obstacle_config": layout}, "agent": {"action_type": atype}, "sim": {"damping": damping}}
    else:
        cfg = default_cfg("area_clearing")
        cfg.env = layout
        over = {"env": layout, "agent": {"action_type": atype}, "sim": {"damping": damping}}
    cfg.agent.action_type = atype
    cfg.sim.damping = damping
    scenes = (make_bd_trials if task == "bd" else make_ac_trials)(cfg, n, seed)
    rng = np.random.default_rng(seed + 7)
    if atype == "heading":
        actions = rng.uniform(-1, 1, (STEPS, n))
    elif atype == "position":
        actions = rng.integers(0, 224 * 224, (STEPS, n)).astype(np.float64)
    else:
        actions = np.stack([rng.uniform(-0.5, 0.5, (STEPS, n)), rng.uniform(-1, 1, (STEPS, n))], -1)

    def make_oracle(scene):
        from oracle.oracle_bd import OracleAreaClearing, OracleBoxDelivery
        if task == "bd":
            bp = S.box_delivery_params(cfg)
            bp["num_boxes"] = len(scene["boxes"])
            bp["step_limit"] = STEP_LIMIT
            return OracleBoxDelivery(S.box_delivery_physics_params(cfg), bp, cfg)
        bp = A.area_clearing_params(cfg)
        bp["step_limit"] = STEP_LIMIT
        return OracleAreaClearing(A.area_clearing_physics_params(cfg), bp, cfg)

    return cfg, over, scenes, actions, make_oracle


def oracle_scene(make_oracle, scene, acts, observe=True):
    """One scene through the oracle: first observation, per step (info, reward, terminated, truncated, shape states, alive), last observation, stats."""
    o = make_oracle(scene)
    obs0 = o.reset(scene, observe=observe)
    n = 6 + len(scene["boxes"])
    steps = []
    obs = None
    for t in range(len(acts)):
        obs, r, term, trunc, info = o.step(acts[t], observe=observe and t == len(acts) - 1)
        steps.append((np.array(list(info.values())), r, term, trunc, o.shape_states()[:n].copy(), o.alive().astype(bool)))
    return dict(obs0=obs0, steps=steps, obs=obs, stats=o.stats())


def oracle_case(make_oracle, scenes, actions, observe=True):
    from oracle.oracle_bd import bdlib
    bdlib()     # the ctypes prototypes are set up here, in the main thread: a handle created while another thread is still inside the lazy setup would
                # be returned through the default `int` restype
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        return list(pool.map(lambda e: oracle_scene(make_oracle, scenes[e], actions[:, e], observe), range(len(scenes))))


def teeth(task, ref):
    """What the oracle's own records say about how much the scenes collide."""
    from oracle.oracle_bd import AC_INFO_KEYS, BD_INFO_KEYS
    k = {n: i for i, n in enumerate(BD_INFO_KEYS if task == "bd" else AC_INFO_KEYS)}
    out = dict(work=0, hit=0, limited=0, task=0)
    for r in ref:
        infos = [s[0] for s in r["steps"]]
        out["work"] += any(i[k["work"]] > 0 for i in infos)
        out["hit"] += any(i[k["robot_hit_obstacle"]] != 0 for i in infos)
        out["limited"] += sum(i[k["substeps"]] > STEP_LIMIT for i in infos)
        out["task"] += int(infos[-1][k["cumulative_boxes"]]) if task == "bd" else int(infos[-1][k["box_count"]] > 0)
    return out
