"""Writes tests/golden/rrt_golden.{json,npz}: recorded output of the reference's own RRT (``RRTPlanner._run_rrt``, baselines/maze_NAMO/planning_based/
RRT/rrt.py), of its policy's ``prune_by_distance`` and of ``DP.ideal_control`` (common/controller/dp.py), next to which the restatement of
tests/rrt_ref.py is run.

Run once, from the repository root, with an interpreter that has numpy (torch is not needed):

    python tests/golden/make_golden_rrt.py /path/to/reference/checkout

The reference is imported as it is, with the stand-ins of make_golden_lattice.py (shapely, yaml, matplotlib and the simulator's dependencies are mocked
where absent; this job calls nothing of them).  The planner and the policy are built with ``__new__``; the planner's ``cfg`` is a namespace with the
values of rrt_config.yaml.  ``_run_rrt`` is given a duck-typed scene -- ``bounds``, ``walls_infl = None`` and ``seg_hit``, the restatement's own
predicate (the reference's is shapely's) -- which also records every (near node, new node, verdict) that passes through it: that is the node list, the
parents and the iteration count of the reference's run.  The name ``random`` inside rrt.py is a recorder in front of ``random.Random(seed)`` whose
``uniform(a, b)`` is CPython's ``a + (b - a) * random()``; since the Mersenne Twister of a seed is the same everywhere, the draws are recorded as the
seed, their number and the first and last few.

Only data is recorded.  Per run: the scene, the statuses, per pass the iterations and tree sizes, the tree of the pass that ended the search (in full
up to 4000 nodes, as sha256 of the float64 / int32 bytes above that), the densified path that ``_run_rrt`` returned and ``prune_by_distance`` of it.
Next to every run the restatement runs in the reference's arithmetic (``hypot=math.hypot``) on the same draws and must agree with ``==``; ``argmin_diff``
counts the iterations in which the reference's ``min(key=hypot)`` and the first minimum of d2 name different nodes."""
import contextlib
import hashlib
import io
import json
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import make_golden_lattice as mgl   # noqa: E402
import rrt_ref as R                 # noqa: E402

FULL_TREE_MAX = 4000
REF_CFG = dict(step=0.05, goal_radius=0.01, goal_bias=0.01, max_nodes=26000, densify_ds=0.08, seed=42)
SMALL_CFG = dict(REF_CFG, step=0.25, max_nodes=2000)
MIN_R = 0.86


class RecordingRandom:
    """Stands where rrt.py says ``random``: the draws of random.Random(seed), counted."""

    def __init__(self, seed):
        self.rng, self.draws = random.Random(seed), []

    def random(self):
        u = self.rng.random()
        self.draws.append(u)
        return u

    def uniform(self, a, b):
        return a + (b - a) * self.random()


class RecordingScene(R.Scene):
    def __init__(self, *a):
        super().__init__(*a)
        self.begin(None)

    def begin(self, start):
        self.nodes, self.parents, self.index, self.calls = [start], [-1], {id(start): 0}, 0

    def seg_hit(self, a, b, boxes_blocking):
        self.calls += 1
        verdict = super().seg_hit(a, b, boxes_blocking)
        if verdict == "none":
            self.index[id(b)] = len(self.nodes)
            self.nodes.append(b)                       # keeps the object alive, so its id stays its own
            self.parents.append(self.index[id(a)])
        return verdict


def square(cx, cy, half=0.25):
    return [(cx - half, cy - half), (cx + half, cy - half), (cx + half, cy + half), (cx - half, cy + half)]


def maze_scene(version, layout_seed):
    from benchpush_amd.envs.maze_namo import _maze_cfg
    from benchpush_amd.config import maze_walls
    from benchpush_amd.maze_scenario import generate_layout
    cfg = _maze_cfg({"maze_version": version})
    walls = maze_walls(cfg)
    lay = generate_layout(cfg, walls, layout_seed)
    boxes = [square(float(c[0]), float(c[1]), cfg.obstacle_size / 2) for c in lay["centres"]]
    return dict(walls=walls, boxes=boxes, start=[float(lay["start"][0]), float(lay["start"][1])], goal=[float(cfg.env.goal_x), float(cfg.env.goal_y)],
                inflate_radius=2.25 * MIN_R)


def small_scenes():
    room = [[0, 0, 4, 0], [4, 0, 4, 3], [4, 3, 0, 3], [0, 3, 0, 0]]
    tri = [(2.0, 0.9), (2.6, 1.5), (1.9, 1.8)]
    return {
        "open_room": dict(walls=room, boxes=[], start=[0.5, 0.5], goal=[3.5, 2.5], inflate_radius=0.2),
        "divider": dict(walls=room + [[2, 0, 2, 2]], boxes=[], start=[0.6, 0.6], goal=[3.4, 0.6], inflate_radius=0.25),
        "boxes_in_the_way": dict(walls=room, boxes=[square(1.5, 1.2, 0.3), square(2.6, 2.0, 0.25), tri], start=[0.5, 1.5], goal=[3.5, 1.5],
                                 inflate_radius=0.2),
        # a door that only a box closes: pass 0 uses up its nodes, pass 1 goes through the box
        "box_in_the_door": dict(walls=room + [[2, 0, 2, 1.2], [2, 1.8, 2, 3]], boxes=[[(1.9, 1.0), (2.1, 1.0), (2.1, 2.0), (1.9, 2.0)]], start=[0.7, 1.5],
                                goal=[3.3, 1.5], inflate_radius=0.1),
        "walled_off": dict(walls=room + [[2, 0, 2, 3]], boxes=[], start=[0.7, 1.5], goal=[3.3, 1.5], inflate_radius=0.1),
        "no_geometry": dict(walls=[], boxes=[], start=[-2.0, -2.0], goal=[2.0, 1.0], inflate_radius=0.3),
    }


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_reference(rrt, policy, sc, cfg, seed):
    planner = rrt.RRTPlanner.__new__(rrt.RRTPlanner)
    planner.cfg = types.SimpleNamespace(**cfg)
    rec = RecordingRandom(seed)
    rrt.random = rec
    scene = RecordingScene(sc["walls"], sc["boxes"], sc["inflate_radius"])
    start, goal = tuple(sc["start"]), tuple(sc["goal"])
    passes, path, status = [], None, R.FALLBACK
    for p, blocking in enumerate((True, False)):       # RRTPlanner.plan: boxes block, then they do not
        scene.begin(start)
        path = planner._run_rrt(start, goal, scene, boxes_blocking=blocking)
        nodes, parents = list(scene.nodes), list(scene.parents)
        if path is not None:                           # the goal node that _run_rrt appended after its last seg_hit
            nodes.append(goal)
            parents.append(len(nodes) - 2)
        passes.append(dict(iterations=scene.calls, n_nodes=len(nodes)))
        if path is not None:
            status = R.FOUND if p == 0 else R.FOUND_IGNORING_BOXES
            break
    if path is None:
        path = [start, goal]
    with contextlib.redirect_stdout(io.StringIO()):
        pruned = policy.prune_by_distance(np.array(path), min_dist=0.3)
    return dict(status=status, passes=passes, nodes=np.asarray(nodes, np.float64), parents=np.asarray(parents, np.int32),
                raw=np.asarray(path, np.float64), pruned=np.asarray(pruned, np.float64), draws=rec.draws)


def main(ref_root):
    mgl.install_stubs()
    sys.meta_path.append(mgl._MockFinder(only={"skimage", "torchvision", "shapely", "yaml", "matplotlib"}))
    sys.path.insert(0, ref_root)
    with contextlib.redirect_stdout(io.StringIO()):
        from benchpush.baselines.maze_NAMO.planning_based.RRT import rrt
        from benchpush.baselines.maze_NAMO.planning_based.policy import PlanningBasedPolicy
        from benchpush.common.controller.dp import DP
    policy = PlanningBasedPolicy.__new__(PlanningBasedPolicy)

    runs = [("maze1_layout0", maze_scene(1, 0), REF_CFG, 42), ("maze2_layout0", maze_scene(2, 0), REF_CFG, 42), ("maze1_layout1", maze_scene(1, 1), REF_CFG, 42)]
    runs += [(name, sc, SMALL_CFG, 42 + i) for i, (name, sc) in enumerate(small_scenes().items())]
    meta, arrays = [], {}
    for name, sc, cfg, seed in runs:
        ref = run_reference(rrt, policy, sc, cfg, seed)
        draws = ref["draws"]
        it = iter(draws)
        audit = {}
        mine = R.rrt_plan(sc["start"], sc["goal"], sc["walls"], sc["boxes"], 0, dict(cfg, inflate_radius=sc["inflate_radius"], max_waypoints=1 << 20),
                          sampler=lambda p, k, j: next(it), hypot=math.hypot, audit=audit)
        agree = (mine["status"] == ref["status"] and mine["n_nodes"][:len(ref["passes"])] == [p["n_nodes"] for p in ref["passes"]]
                 and np.array_equal(np.asarray(mine["nodes"]), ref["nodes"]) and mine["parents"] == ref["parents"].tolist()
                 and (ref["status"] == R.FALLBACK or np.array_equal(np.asarray(mine["raw"]), ref["raw"]))
                 and np.array_equal(np.asarray(mine["path"]), ref["pruned"]) and next(it, None) is None)
        full = len(ref["nodes"]) <= FULL_TREE_MAX
        m = dict(name=name, scene=sc, cfg=cfg, seed=seed, status=ref["status"], passes=ref["passes"], n_draws=len(draws), first_draws=draws[:4],
                 last_draws=draws[-4:], nodes_sha256=sha(ref["nodes"]), parents_sha256=sha(ref["parents"]), full_tree=full, raw_points=len(ref["raw"]),
                 pruned_points=len(ref["pruned"]), restatement_agrees=bool(agree), argmin_diff=int(audit.get("argmin_diff", 0)))
        meta.append(m)
        if full:
            arrays[name + "/nodes"], arrays[name + "/parents"] = ref["nodes"], ref["parents"]
        arrays[name + "/raw"], arrays[name + "/pruned"] = ref["raw"], ref["pruned"]
        print("%-18s status %d, passes %s, raw %d points, pruned %d, %d draws, restatement agrees: %s, argmin differences: %d"
              % (name, ref["status"], ref["passes"], len(ref["raw"]), len(ref["pruned"]), len(draws), agree, m["argmin_diff"]))
        assert agree, name

    # the controller: DP(...).ideal_control over poses near, far and past the end of the recorded pruned paths
    ctrl = dict(dt=0.8, Lfc=0.5, target_speed=0.15)
    action_scale = (math.pi / 2) / 15
    rng = np.random.RandomState(20240702)
    track, worst = [], 0.0
    for name in ("maze1_layout0", "maze2_layout0", "boxes_in_the_way", "open_room"):
        path = arrays[name + "/pruned"]
        poses, outs, idx = [], [], []
        for t in range(40):
            i = rng.randint(0, len(path))
            far = t % 4 == 3
            off = rng.normal(0, 2.0 if far else 0.2, 2)
            pose = [round(float(path[i, 0] + off[0]), 6), round(float(path[i, 1] + off[1]), 6), round(float(rng.uniform(-math.pi, math.pi)), 6)]
            if t % 10 == 9:      # past the end
                d = path[-1] - path[-2]
                pose[0], pose[1] = round(float(path[-1, 0] + 3 * d[0]), 6), round(float(path[-1, 1] + 3 * d[1]), 6)
            if t == 0:
                pose[0], pose[1] = float(path[0, 0]), float(path[0, 1])
            dp = DP(x=pose[0], y=pose[1], yaw=pose[2], cx=path.T[0], cy=path.T[1], ch=np.zeros(len(path)), **ctrl)
            omega, _ = dp.ideal_control(*pose)
            near = int(dp.target_course.search_target_index(pose[0], pose[1])[1])
            target = int(np.flatnonzero((path[:, 0] == dp.setpoint[0]) & (path[:, 1] == dp.setpoint[1]))[0])
            act, (mn, mt) = R.track_waypoints_ref(path, pose, action_scale, fns=R.LIBM)
            assert (mn, mt) == (near, target), (name, pose, mn, mt, near, target)
            worst = max(worst, abs(act - float(omega) / action_scale))
            poses.append(pose), outs.append(float(omega) / action_scale), idx.append([near, target])
        track.append(dict(path=name, poses=poses, actions=outs, indices=idx))

    out = dict(min_r=MIN_R, runs=meta, track=track, action_scale=action_scale, track_cfg=dict(Lfc=0.5, dt=0.8), max_action_diff=worst)
    with open(os.path.join(HERE, "rrt_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "rrt_golden.npz"), **arrays)
    print("wrote rrt_golden.json (%d bytes) and rrt_golden.npz (%d bytes); controller: largest action difference %.3g over %d calls"
          % (os.path.getsize(os.path.join(HERE, "rrt_golden.json")), os.path.getsize(os.path.join(HERE, "rrt_golden.npz")), worst,
             sum(len(t["poses"]) for t in track)))


if __name__ == "__main__":
    main(sys.argv[1])
