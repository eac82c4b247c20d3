"""Writes tests/golden/gtsp_golden.{json,npz}: recorded output of the reference's own GTSP baseline code (TransitionGraphLookup, GTSPFileGenerator,
GTSPSolver.evaluate_tour, PlanningBasedPolicy.plan_path / act with the DP controller), next to which the restatement of tests/gtsp_ref.py is run.

Run once, from the repository root, after the oracle library is built:

    python tests/golden/make_golden_gtsp.py /path/to/reference/checkout

The reference is imported as it is, with the stand-ins of make_golden_lattice.py plus three of this job's own, because shapely and the GLNS solver
are not available where this runs:
  * ``LineString`` is a duck type with ``coords`` and ``length``, all that transition_graph_lookup.py and extend_linestring_at_start use;
  * ``Polygon(..).intersects``, ``Polygon(..).buffer(-0.4)`` and ``shortest_line`` answer with the restatement's separating-axis test and its nearest
    pair (before extension and rounding, which the reference's own lines then do);
  * ``GTSPSolver.find_classic_tour`` returns the restatement's optimal tour in the place of GLNS's output.
So the golden pins the transition tables, the rounding of the instance file, evaluate_tour, the path and the controller -- not shapely's buffer and
shortest_line, and not GLNS.  Only data is recorded.  The scenes are chosen so that no 100 * cost lies near a half-integer (the reference's arccos and
the restatement's atan2 differ by up to 4.2e-8 for near-parallel directions, gtsp_ref.arccos_error); the smallest distance that occurred is recorded."""
import contextlib
import io
import json
import math
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import make_golden_lattice as mgl   # noqa: E402
import gtsp_ref as R                # noqa: E402

BOUNDARY = [[-5.0, -5.0], [-5.0, 5.0], [5.0, 5.0], [5.0, -5.0]]          # clear_env
GOALS = [[BOUNDARY[i], BOUNDARY[(i + 1) % 4]] for i in range(4)]
# (seed, boxes, straddling boxes, pose); act sequences are recorded for the scenes with at most 3 boxes
SCENES = [(1, 1, 0, (0.3, -0.2, 1.1)), (2, 2, 0, (-1.4, 2.2, -2.0)), (3, 3, 0, (2.1, 0.4, 0.3)), (4, 4, 1, (-0.6, -3.1, 2.7)),
          (5, 5, 0, (3.3, 3.0, -0.4)), (6, 6, 2, (0.0, 0.0, math.pi / 2)), (7, 7, 0, (-3.2, 1.9, 0.0)), (8, 8, 0, (1.2, -1.7, -3.0)),
          (9, 9, 1, (4.1, -4.2, 1.9)), (10, 10, 0, (-2.5, -2.4, 0.8)), (11, 10, 1, (0.7, 3.6, -1.2)), (12, 3, 1, (-4.0, 4.0, -0.7))]
NEAR_HALF = 1e-5      # no 100 * cost of a recorded scene is this near a half-integer: arccos against atan2 moves 100 * cost by 6.6e-6 at the most
                      # (two angles, each off by up to gtsp_ref.arccos_error(0) = 4.2e-8 where the directions are parallel, times 100 * pi / 4)
assert 2 * R.arccos_error(0.0) * 100 * math.pi / 4 < NEAR_HALF


class LineString:
    def __init__(self, coords):
        self.coords = [tuple(float(v) for v in c) for c in np.asarray(coords, np.float64).tolist()]

    @property
    def length(self):
        return sum(math.sqrt((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2) for a, b in zip(self.coords[:-1], self.coords[1:]))


class Polygon:
    shrink = None

    def __init__(self, verts, shrunk=None):
        self.verts = [tuple(float(v) for v in p) for p in np.asarray(verts, np.float64).tolist()]
        self.shrunk = shrunk

    def intersects(self, other):
        return R.intersects(self.verts, other.verts)

    def buffer(self, d):
        return Polygon(self.verts, R.shrink(self.verts, -d))


def shortest_line(poly, goal):
    bp, gp, _ = R.nearest_pair(poly.verts, poly.shrunk, goal.coords[0], goal.coords[1])
    return LineString([bp, gp])


def scene(seed, n, straddle, attempt=0):
    rng = np.random.default_rng(1000 + seed + 100 * attempt)
    boxes = np.zeros((n, 20, 2))
    for b in range(n):
        while True:
            if b < straddle:
                side = int(rng.integers(0, 4))
                t, off = rng.uniform(-3.5, 3.5), rng.uniform(4.7, 5.2)
                cx, cy = [(-off, t), (t, off), (off, t), (t, -off)][side]
            else:
                cx, cy = rng.uniform(-4.0, 4.0, 2)
            if all(math.hypot(cx - q[0], cy - q[1]) > 1.5 for q in boxes[:b, :4].mean(1)):
                break
        a, h = rng.uniform(0, math.pi / 2), 0.5
        boxes[b, :4] = [[cx + h * (math.cos(a) * sx - math.sin(a) * sy), cy + h * (math.sin(a) * sx + math.cos(a) * sy)]
                        for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    return boxes, np.full(n, 4, np.int32)


def main(ref_root):
    mgl.install_stubs()
    sys.meta_path.append(mgl._MockFinder(only={"skimage", "torchvision"}))
    sh, shg = mgl._MockModule("shapely"), mgl._MockModule("shapely.geometry")
    shg.Polygon, shg.LineString, shg.Point = Polygon, LineString, object
    sh.geometry, sh.shortest_line = shg, shortest_line
    sys.modules["shapely"], sys.modules["shapely.geometry"] = sh, shg
    sys.path.insert(0, ref_root)
    from benchpush.baselines.area_clearing.planning_based import policy as pol
    from benchpush.baselines.area_clearing.planning_based.GTSPPlanner import solve_gtsp

    meta = {"boundary": BOUNDARY, "goals": GOALS, "near_half": NEAR_HALF, "scenes": []}
    arrays = {}
    min_half, max_table, max_act = 1.0, 0.0, 0.0
    cwd = os.getcwd()
    for seed, n, straddle, pose in SCENES:
        attempt = 0
        while True:       # the first draw of the scene with no cost near a half-integer
            boxes, counts = scene(seed, n, straddle, attempt)
            r0 = R.plan(pose, boxes, counts, GOALS, BOUNDARY, fns=R.LIBM)
            T0 = R.weight_matrix(r0["routes"], pose, 4, R.DEFAULTS, R.LIBM, tables=True)[1][0]
            if np.abs((100.0 * T0) % 1.0 - 0.5)[T0 > 0].min() > 10 * NEAR_HALF:
                break
            attempt += 1
        r = R.plan(pose, boxes, counts, GOALS, BOUNDARY, fns=R.LIBM)
        assert (r["status"] & 0xFF) == R.OK and r["n_push"] == n, (seed, r["status"], r["n_push"])
        N = 4 * n + 1
        Wm, T = R.weight_matrix(r["routes"], pose, 4, R.DEFAULTS, R.LIBM, tables=True)
        robot_id = N
        solve_gtsp.GTSPSolver.find_classic_tour = lambda self, prop, _t=[robot_id] + [u + 1 for u in r["tour"]] + [robot_id]: (list(_t), 0.0)
        p = pol.PlanningBasedPolicy(None)
        p.boundary_polygon = Polygon(BOUNDARY)
        p.boundary_goals = [LineString(g) for g in GOALS]
        captured = {}
        orig = pol.TransitionGraphLookup.compute_transition_graph
        orig_eval = solve_gtsp.GTSPSolver.evaluate_tour

        def grab(robot_pose, obs, paths, _o=orig):
            captured["graph"], captured["paths"] = _o(robot_pose, obs, paths), paths
            return captured["graph"]

        def grab_eval(self, tour, lookup, robot_node, _o=orig_eval):
            captured["eval"] = _o(self, tour, lookup, robot_node)
            return captured["eval"]
        pol.TransitionGraphLookup.compute_transition_graph = staticmethod(grab)
        solve_gtsp.GTSPSolver.evaluate_tour = grab_eval
        tmp = tempfile.mkdtemp()
        os.chdir(tmp)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                p.plan_path(list(pose), None, [b[:c].tolist() for b, c in zip(boxes, counts)])
            with open("AreaClearingGTSP.gtsp") as f:
                lines = f.read().split("\n")
        finally:
            os.chdir(cwd)
            pol.TransitionGraphLookup.compute_transition_graph = staticmethod(orig)
            solve_gtsp.GTSPSolver.evaluate_tour = orig_eval
        k = lines.index("EDGE_WEIGHT_SECTION")
        rows = np.asarray([[int(v) for v in ln.split()] for ln in lines[k + 1:k + 1 + N]], np.int64)
        # write_to_file multiplies the diagonal's SELF_WEIGHT by 100 like every weight; the rows are recorded with the matrix's own 99999999 there
        assert (np.diag(rows) == R.SELF_WEIGHT * 100).all()
        rows[np.arange(N), np.arange(N)] = R.SELF_WEIGHT
        # the reference's rounded push paths are the restatement's routes
        ref_routes = [list(ls.coords) for per_box in captured["paths"] for ls in per_box]
        assert ref_routes == [[tuple(q) for q in rt] for rt in r["routes"]], "scene %d: push paths differ" % seed
        # the reference's tables, laid out as [cost, length, angle][u][v]; an entry that the reference never computes stays 0
        g = captured["graph"]
        start = [rt[0] for rt in r["routes"]] + [(pose[0], pose[1])]
        end = [rt[2] for rt in r["routes"]] + [(pose[0], pose[1])]
        keys = {}
        for u in range(N):
            for v in range(N):
                if u != v and (u == N - 1 or v == N - 1 or u // 4 != v // 4):
                    keys.setdefault((tuple(end[u]), tuple(start[v])), []).append((u, v))
        assert all(len(v) == 1 for v in keys.values()), "scene %d: two transitions share their coordinates" % seed
        Tref = np.zeros((3, N, N))
        for key, ((u, v),) in keys.items():
            Tref[:, u, v] = g.cost_lookup[key], g.length_lookup[key], g.angle_lookup[key]
        frac = np.abs((100.0 * Tref[0]) % 1.0 - 0.5)[Tref[0] > 0]
        min_half = min(min_half, float(frac.min()))
        assert frac.min() > NEAR_HALF, "scene %d: a cost within %g of a half-integer; pick another seed" % (seed, NEAR_HALF)
        max_table = max(max_table, float(np.abs(Tref - T).max()))
        final_nodes, _, tcost, tlen, tang, _ = captured["eval"]
        rec = {"seed": seed, "n": n, "straddle": straddle, "attempt": attempt, "pose": list(pose), "tour": r["tour"], "cost": r["cost"],
               "final_nodes": [nd.node_id - 1 for nd in final_nodes], "transition_cost": float(tcost), "transition_length": float(tlen),
               "total_angle": float(tang), "status": r["status"], "act": None}
        assert np.array_equal(rows, Wm), "scene %d: integer rows differ in %d entries" % (seed, int((rows != Wm).sum()))
        arrays["boxes_%d" % seed], arrays["rows_%d" % seed], arrays["tables_%d" % seed] = boxes[:, :4], rows, Tref
        arrays["path_%d" % seed] = np.asarray(p.path, np.float64)
        if n <= 3:
            # the reference's act over a scripted pose sequence: the pose moves 0.3 along the heading the controller asks for
            q = pol.PlanningBasedPolicy(None)
            q.plan_path = lambda agent_pos, observation, obstacles, _q=q, _p=p: setattr(_q, "path", _p.path)
            x, y, yaw = pose
            poses, outs = [], []
            state = R.track_init(r["path"], r["length"], pose, R.DEFAULTS["Lfc"])
            for call in range(400):
                v, om = q.act(None, agent_pos=[x, y, yaw], obstacles=None)
                (sv, so), diag, state = R.track(r["path"], r["length"], (x, y, yaw), state, 1.0, 1.0, fns=R.LIBM)
                max_act = max(max_act, abs(float(v) - sv), abs(float(om) - so))
                assert diag == q.current_point_id, (seed, call, diag, q.current_point_id)
                poses.append([x, y, yaw])
                outs.append([float(v), float(om), int(q.current_point_id)])
                if v == 0.0 and om == 0.0 and q.current_point_id >= len(q.path):
                    break
                yaw = yaw + float(om) * 0.8 if call % 7 else yaw + 0.9 * float(om) * 0.8     # now and then short of the heading asked for
                yaw = math.atan2(math.sin(yaw), math.cos(yaw))
                x, y = x + 0.3 * math.cos(yaw), y + 0.3 * math.sin(yaw)
            assert outs[-1][:2] == [0.0, 0.0], "scene %d: the scripted robot did not reach the end of the path" % seed
            rec["act"] = {"poses": poses, "out": outs}
        meta["scenes"].append(rec)
    meta.update(min_half_distance=min_half, max_table_diff=max_table, max_act_diff=max_act)
    with open(os.path.join(HERE, "gtsp_golden.json"), "w") as f:
        json.dump(meta, f)
    np.savez_compressed(os.path.join(HERE, "gtsp_golden.npz"), **arrays)
    print("scenes %d, min distance to a half-integer %.3g, max table difference %.3g, max act difference %.3g"
          % (len(meta["scenes"]), min_half, max_table, max_act))


if __name__ == "__main__":
    main(sys.argv[1])
