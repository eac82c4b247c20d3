"""bp_gtsp_plan / bp_gtsp_track on the GPU against the restatement of tests/gtsp_ref.py: == for the integers, bit for bit for the float64 paths and
actions.  E <= 8 everywhere; every launch's reference is computed once per module."""
import math

import numpy as np
import pytest
import torch

import gtsp_ref as R

pytestmark = pytest.mark.gpu
E = 8
BD = [[-5.0, -5.0], [-5.0, 5.0], [5.0, 5.0], [5.0, -5.0]]          # clear_env, the default layout and the golden's
GOALS = np.asarray([[BD[i], BD[(i + 1) % 4]] for i in range(4)], np.float64)


def sq(cx, cy, a=0.0, h=0.5):
    return [[cx + h * (math.cos(a) * sx - math.sin(a) * sy), cy + h * (math.sin(a) * sx + math.cos(a) * sy)] for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def env():
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    e = BatchedAreaClearingEnv(E, cfg={"agent": {"action_type": "velocity"}})
    e.reset()
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _scene_inputs(golden, B=13):
    """poses [12, 3], boxes [12, B, 20, 2], counts [12, B] of the golden scenes."""
    G, Z = golden
    S = G["scenes"]
    poses, boxes, counts = np.zeros((len(S), 3)), np.zeros((len(S), B, 20, 2)), np.zeros((len(S), B), np.int32)
    for i, s in enumerate(S):
        poses[i] = s["pose"]
        boxes[i, :s["n"], :4] = Z["boxes_%d" % s["seed"]]
        counts[i, :s["n"]] = 4
    return poses, boxes, counts


def _random_boxes(rng, n, B=13):
    boxes, counts = np.zeros((B, 20, 2)), np.zeros(B, np.int32)
    for b in range(n):
        boxes[b, :4] = sq(rng.uniform(-4.3, 4.3), rng.uniform(-4.3, 4.3), rng.uniform(0, 1.5))
        counts[b] = 4
    return boxes, counts


@pytest.fixture(scope="module")
def batches(env, golden):
    """name -> (inputs, GTSPPlan on the host as a dict, the restatement per env).  Four launches."""
    from benchpush_amd.planning import GTSPConfig
    gp, gb, gc = _scene_inputs(golden)
    rng = np.random.default_rng(11)
    out = {}

    def run(name, poses, boxes, counts, goals, **kw):
        cfg = GTSPConfig(**kw)
        plan = env.gtsp_plan(dev(poses), dev(boxes), dev(counts), dev(goals.reshape(-1, 4)), config=cfg, return_weights=True)
        host = {k: getattr(plan, k).cpu().numpy() for k in plan._fields}
        ref = [R.plan(poses[e], boxes[e], counts[e], goals, BD, cfg=dict(max_boxes=cfg.max_boxes)) for e in range(E)]
        out[name] = (dict(poses=poses, boxes=boxes, counts=counts, goals=goals, cfg=cfg), host, ref)

    run("golden_0_7", gp[:8], gb[:8], gc[:8], GOALS)                       # n = 1 .. 8
    # the last four golden scenes (n = 9, 10, 10, 3) and four edge cases
    poses, boxes, counts = np.zeros((E, 3)), np.zeros((E, 13, 20, 2)), np.zeros((E, 13), np.int32)
    poses[:4], boxes[:4], counts[:4] = gp[8:], gb[8:], gc[8:]
    poses[4:] = [(0.3, 0.2, 1.0), (1.0, -2.0, -0.5), (0.0, 0.0, math.pi / 2), (-1.0, 1.0, 2.5)]
    boxes[4, 0, :4], counts[4, 0] = sq(5.5 + 1e-6, 0.4), 4                  # env 4: a box just outside the boundary: nothing to push
    boxes[5, 3, :4], counts[5, 3] = sq(0.7, 1.1, 0.4), 4                    # env 5: n = 1, in slot 3
    boxes[6, 0, :4], boxes[6, 1, :4], counts[6, :2] = sq(2.0, 0.0), sq(-2.0, 0.0), 4     # env 6: n = 2, mirror images about the robot's heading: equal weights
    boxes[7, 0, :4], boxes[7, 2, :4], boxes[7, 3, :4] = sq(1.0, 1.0, 0.3), sq(5.05, -2.0, 0.1), sq(-2.0, -3.0, 1.0)
    counts[7, [0, 2, 3]] = 4                                                # env 7: a count of 0 in the middle, and a box straddling the edge x = 5
    run("golden_8_11_edges", poses, boxes, counts, GOALS)
    # at the cap and past it
    poses, boxes, counts = rng.uniform(-3, 3, (E, 3)), np.zeros((E, 13, 20, 2)), np.zeros((E, 13), np.int32)
    for e, n in enumerate([12, 13, 11, 0, 2, 1, 3, 4]):
        boxes[e], counts[e] = _random_boxes(rng, n)
    run("cap_12", poses, boxes, counts, GOALS, max_boxes=12)
    # three goal segments: N = 3 n + 1, no multiple of the wave size
    poses = rng.uniform(-3, 3, (E, 3))
    for e, n in enumerate([6, 5, 7, 1, 2, 3, 4, 6]):
        boxes[e], counts[e] = _random_boxes(rng, n)
    run("three_goals", poses, boxes, counts, GOALS[:3], max_boxes=8)
    return out


def _check(host, ref, e, G, fill=0):
    """`fill`: what the caller's buffers held before the launch (a fresh plan is zeroed); the kernel writes the N x N block of `weights` and no more."""
    r = ref[e]
    n = r["n_push"]
    N = n * G + 1
    print("env %d: n %d status %#x / %#x cost %d / %d" % (e, n, host["status"][e], r["status"], host["cost"][e], r["cost"]))
    assert host["status"][e] == r["status"] and host["n_push"][e] == n
    if (r["status"] & 0xFF) in (R.CAP, R.INVALID):
        assert host["lengths"][e] == 0
        return
    assert host["cost"][e] == r["cost"] and host["tour"][e, :n].tolist() == r["tour"]
    assert np.array_equal(host["weights"][e, :N, :N], r["W"])
    rest = host["weights"][e].copy()
    rest[:N, :N] = fill
    assert (rest == fill).all()
    assert host["lengths"][e] == r["length"] == 2 * n + 1
    assert host["paths"][e, :2 * n + 1].tobytes() == np.ascontiguousarray(r["path"]).tobytes()          # bit for bit
    assert (int(host["track_id"][e]), float(host["track_setpoint"][e, 0]), float(host["track_setpoint"][e, 1])) == r["track"]


@pytest.mark.parametrize("name", ["golden_0_7", "golden_8_11_edges", "cap_12", "three_goals"])
def test_plan_equals_the_restatement(batches, name):
    inp, host, ref = batches[name]
    G = len(inp["goals"])
    for e in range(E):
        _check(host, ref, e, G)


def test_the_batches_hold_the_cases_they_are_meant_to(batches, golden):
    S = golden[0]["scenes"]
    _, host, ref = batches["golden_0_7"]
    assert [r["n_push"] for r in ref] == [s["n"] for s in S[:8]] and [r["tour"] for r in ref] == [s["tour"] for s in S[:8]]
    assert host["cost"].tolist() == [s["cost"] for s in S[:8]]                                     # the optimum recorded with the reference's own rows
    _, host, ref = batches["golden_8_11_edges"]
    assert [r["n_push"] for r in ref] == [9, 10, 10, 3, 0, 1, 2, 3]
    assert ref[4]["status"] == R.NOTHING_TO_PUSH and host["lengths"][4] == 1
    assert ref[5]["clusters"] == [3] and ref[7]["clusters"] == [0, 2, 3] and ref[7]["status"] == R.OK | R.FLAG_DEGENERATE
    W, c, t = ref[6]["W"], ref[6]["cost"], ref[6]["tour"]                                             # the tie: another tour costs the same
    others = [(a, b) for a in range(8) for b in range(8) if a // 4 != b // 4 and [a, b] != t and W[8, a] + W[a, b] + W[b, 8] == c]
    assert others and all(t < [a, b] for a, b in others)
    _, host, ref = batches["cap_12"]
    assert ref[0]["n_push"] == 12 and (ref[0]["status"] & 0xFF) == R.OK and (ref[1]["status"] & 0xFF) == R.CAP and host["n_push"][1] == 13
    _, host, ref = batches["three_goals"]
    assert ref[0]["n_push"] == 6 and ref[0]["W"].shape == (19, 19)


def test_active_out_reuse_nan_and_independence(env, batches):
    from benchpush_amd.planning import GTSPPlan
    inp, host, ref = batches["golden_8_11_edges"]
    poses, boxes, counts, cfg = inp["poses"].copy(), inp["boxes"].copy(), inp["counts"].copy(), inp["cfg"]
    # the other envs' inputs change, env 1 and env 7 keep theirs; env 2 gets a NaN pose; envs 4 and 5 are not active
    rng = np.random.default_rng(5)
    for e in (0, 3, 6):
        boxes[e, :, :4] += rng.uniform(-0.3, 0.3, (13, 1, 2))
        poses[e] += 0.25
    poses[2, 1] = math.nan
    active = np.ones(E, np.uint8)
    active[[4, 5]] = 0
    mark = -7
    out = GTSPPlan(*[torch.full(tuple(v.shape), mark, dtype=torch.from_numpy(v).dtype).cuda() for v in (host[k] for k in GTSPPlan._fields)])
    got = env.gtsp_plan(dev(poses), dev(boxes), dev(counts), dev(GOALS.reshape(-1, 4)), dev(active), config=cfg, out=out, return_weights=True)
    assert got is out
    h2 = {k: getattr(got, k).cpu().numpy() for k in got._fields}
    for e in (1, 7):
        _check(h2, ref, e, 4, fill=mark)
        for k in ("cost", "n_push", "lengths", "track_id"):
            assert h2[k][e] == host[k][e]
        assert h2["paths"][e, :host["lengths"][e]].tobytes() == host["paths"][e, :host["lengths"][e]].tobytes()
    for e in (0, 3, 6):
        _check(h2, [R.plan(poses[i], boxes[i], counts[i], GOALS, BD) for i in range(E)], e, 4, fill=mark)
    assert h2["status"][2] == R.INVALID and h2["lengths"][2] == 0 and h2["n_push"][2] == 0
    for e in (4, 5):                                                               # SKIPPED: nothing but the status is written
        assert h2["status"][e] == R.SKIPPED
        for k in got._fields:
            if k != "status":
                assert (h2[k][e] == mark).all(), k


def test_tracker_equals_the_restatement_over_the_golden_sequences(env, golden, batches):
    from benchpush_amd.planning import GTSPConfig, GTSPPlan
    G, _ = golden
    S = [s for s in G["scenes"] if s["act"] is not None][:4]
    gp, gb, gc = _scene_inputs(golden)
    idx = [G["scenes"].index(s) for s in S] + [0, 0, 0, 0]
    cfg = GTSPConfig()
    plan = env.gtsp_plan(dev(gp[idx]), dev(gb[idx]), dev(gc[idx]), config=cfg)
    tr = plan.tracker()
    paths, lens = plan.paths.cpu().numpy(), plan.lengths.cpu().numpy()
    state = [(int(plan.track_id[e]), *plan.track_setpoint[e].tolist()) for e in range(E)]
    vs, ws = env.target_speed, env.max_yaw_rate_step
    calls = max(len(s["act"]["poses"]) for s in S)
    switches = ends = 0
    out = None
    for k in range(calls):
        poses, active = np.zeros((E, 3)), np.zeros(E, np.uint8)
        for e, s in enumerate(S):
            if k < len(s["act"]["poses"]):
                poses[e], active[e] = s["act"]["poses"][k], 1
        out = env.track_pushes(plan, tr, dev(poses), dev(active), config=cfg, out=out)
        a, d = out[0].cpu().numpy(), out[1].cpu().numpy()
        ids, sp = tr.ids.cpu().numpy(), tr.setpoint.cpu().numpy()
        for e in range(E):
            if not active[e]:
                assert np.isnan(a[e]).all() and d[e] == -1 and (int(ids[e]), *sp[e].tolist()) == state[e]       # NaN, and the state as it was
                continue
            (rv, rw), rd, st = R.track(paths[e], lens[e], poses[e], state[e], vs, ws)
            assert (a[e, 0], a[e, 1], d[e]) == (rv, rw, rd) and (int(ids[e]), *sp[e].tolist()) == st
            assert d[e] == S[e]["act"]["out"][k][2]                                                            # the reference's own current_point_id
            switches += st[0] != state[e][0]
            ends += rd >= lens[e] and (rv, rw) == (0.0, 0.0)
            state[e] = st
    assert switches >= 10 and ends >= len(S)
    # a path of the pose alone (nothing to push) and a NaN pose: NaN, -1
    _, host, _ = batches["golden_8_11_edges"]
    p2 = GTSPPlan(*[None if host[k] is None else dev(host[k]) for k in GTSPPlan._fields])
    t2 = p2.tracker()
    poses = batches["golden_8_11_edges"][0]["poses"].copy()
    poses[0, 2] = math.nan
    a, d = env.track_pushes(p2, t2, dev(poses), config=cfg)
    assert torch.isnan(a[[0, 4]]).all() and d[[0, 4]].tolist() == [-1, -1] and not torch.isnan(a[[1, 2, 3, 5, 6, 7]]).any()
    assert torch.equal(t2.ids[[0, 4]], p2.track_id[[0, 4]]) and torch.equal(t2.setpoint[[0, 4]], p2.track_setpoint[[0, 4]])


def test_refusals_raise_before_any_launch(env, batches):
    from benchpush_amd import _lib
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    from benchpush_amd.planning import GTSPConfig, GTSPPlan, GTSPTrackerState
    inp, host, _ = batches["golden_0_7"]
    poses, boxes, counts, goals = dev(inp["poses"]), dev(inp["boxes"]), dev(inp["counts"]), dev(GOALS.reshape(-1, 4))
    mark = 123
    out = GTSPPlan(*[torch.full(tuple(v.shape), mark, dtype=torch.from_numpy(v).dtype).cuda() for v in (host[k] for k in GTSPPlan._fields)])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((getattr(out, k) == mark).all()) for k in out._fields)
    with pytest.raises(_lib.BpError):
        env.gtsp_plan(poses, boxes, counts, goals, config=GTSPConfig(max_boxes=13))
    with pytest.raises(_lib.BpError):
        env.gtsp_workspace_bytes(GTSPConfig(max_boxes=13))
    with pytest.raises(_lib.BpError):
        env.gtsp_plan(poses, boxes, counts, torch.zeros((9, 4), dtype=torch.float64).cuda(), config=GTSPConfig(num_goals=9))
    need = env.gtsp_workspace_bytes()
    assert need == E * 1024 * 40 * 4
    with pytest.raises(_lib.BpError):
        env.gtsp_plan(poses, boxes, counts, goals, workspace=torch.empty(need - 16, dtype=torch.uint8).cuda(), out=out, return_weights=True)
    for bad in (dict(poses=poses.float()), dict(poses=poses.cpu()), dict(poses=poses[:, :2].contiguous()), dict(poses=poses.t().contiguous().t()),
                dict(counts=counts.long()), dict(boxes=boxes[:, :, :, :1].contiguous()), dict(goals=goals[:3]), dict(goals=goals.reshape(-1, 2)),
                dict(active=torch.ones(E - 1, dtype=torch.uint8).cuda()), dict(workspace=torch.empty(need, dtype=torch.int32).cuda()),
                dict(boxes=None)):
        kw = dict(dict(poses=poses, boxes=boxes, counts=counts, goals=goals), **bad)
        with pytest.raises(ValueError):
            env.gtsp_plan(out=out, return_weights=True, **kw)
    tr = GTSPTrackerState(E, env.device)
    with pytest.raises(ValueError):
        env.track_pushes(out, tr, poses.float())
    with pytest.raises(ValueError):
        env.track_pushes(out, GTSPTrackerState(E - 1, env.device))
    assert untouched()
    # a maze handle: the library refuses it
    import ctypes as C
    from benchpush_amd.envs.ship_ice import _ptr
    maze = BatchedMazeEnv(E, num_layouts=2)
    try:
        maze.reset()
        cfg = GTSPConfig(v_scale=0.2, w_scale=0.1).as_struct(num_goals=4)
        ws = torch.empty(need, dtype=torch.uint8).cuda()
        rc = maze.L.bp_gtsp_plan(maze.h, C.byref(cfg), _ptr(poses), _ptr(boxes), _ptr(counts), 13, 20, _ptr(goals), None, _ptr(ws), need, _ptr(out.status),
                                 _ptr(out.n_push), _ptr(out.tour), _ptr(out.cost), _ptr(out.paths), _ptr(out.lengths), _ptr(out.track_id),
                                 _ptr(out.track_setpoint), None, maze._stream())
        assert rc == -1 and b"area-clearing handles only" in maze.L.bp_last_error(maze.h)
        rc = maze.L.bp_gtsp_track(maze.h, C.byref(cfg), _ptr(out.paths), _ptr(out.lengths), _ptr(poses), None, _ptr(tr.ids), _ptr(tr.setpoint),
                                  _ptr(torch.zeros((E, 2), dtype=torch.float64).cuda()), _ptr(torch.zeros(E, dtype=torch.int32).cuda()), maze._stream())
        assert rc == -1
        rc = env.L.bp_gtsp_plan(env.h, C.byref(cfg), None, _ptr(boxes), _ptr(counts), 13, 20, _ptr(goals), None, _ptr(ws), need, _ptr(out.status),
                                _ptr(out.n_push), _ptr(out.tour), _ptr(out.cost), _ptr(out.paths), _ptr(out.lengths), _ptr(out.track_id),
                                _ptr(out.track_setpoint), None, env._stream())
        assert rc == -1 and b"NULL" in env.L.bp_last_error(env.h)
    finally:
        maze.close()
    assert untouched()


def test_end_to_end_from_the_env_state():
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    env = BatchedAreaClearingEnv(4, cfg={"agent": {"action_type": "velocity"}})
    try:
        env.reset()
        plan = env.gtsp_plan(return_weights=True)
        verts, cnt = env.world_polys()
        boxes, counts = verts[:, 6:6 + env.nbox].cpu().numpy(), cnt[:, 6:6 + env.nbox].cpu().numpy()
        pb, pc = env.push_box_polys()
        assert np.array_equal(pb.cpu().numpy(), boxes) and np.array_equal(pc.cpu().numpy(), counts)
        poses = env.info[:, :3].cpu().numpy()
        gnp, gdev = env.boundary_goals()
        assert gnp.shape == (4, 2, 2) and np.array_equal(gnp, GOALS)
        host = {k: getattr(plan, k).cpu().numpy() for k in plan._fields}
        ref = [R.plan(poses[e], boxes[e], counts[e], gnp, BD) for e in range(4)]
        for e in range(4):
            _check(host, ref, e, 4)
            assert ref[e]["n_push"] == env.nbox == 10 and (ref[e]["status"] & 0xFF) == R.OK
        tr = plan.tracker()
        for _ in range(5):
            actions, diag = env.track_pushes(plan, tr)
            assert not torch.isnan(actions).any() and (diag >= 1).all()
            env.step(actions)
        env.check_errors()
        assert float((env.info[:, :2] - torch.from_numpy(poses[:, :2]).cuda()).abs().max()) > 0.0       # the robots moved
    finally:
        env.close()


def test_policy_evaluate_returns_the_five_tuple():
    from benchpush_amd.baselines.area_clearing.planning_based.policy import PlanningBasedPolicy
    p = PlanningBasedPolicy(glns_executable_path=None, cfg=None, t_max=5, num_trials=2)
    success, eff, effort, rewards, name = p.evaluate(1)
    assert name == "GTSP" and len(success) == len(eff) == len(effort) == len(rewards) == 1
    assert all(math.isfinite(v) for v in (success[0], eff[0], effort[0], rewards[0]))
    # the reference's single-env surface on the device
    p.update_boundary_and_obstacles(BD, [], [])
    v, om = p.act(None, agent_pos=(0.3, -0.2, 1.1), obstacles=[sq(1.0, 1.0, 0.3), sq(-2.0, 2.0, 0.0)])
    boxes = np.zeros((2, 20, 2))
    boxes[0, :4], boxes[1, :4] = sq(1.0, 1.0, 0.3), sq(-2.0, 2.0, 0.0)
    r = R.plan((0.3, -0.2, 1.1), boxes, [4, 4], GOALS, BD)
    assert p.path.tobytes() == np.ascontiguousarray(r["path"]).tobytes() and p.current_point_id == 1
    (rv, rw), _, _ = R.track(r["path"], r["length"], (0.3, -0.2, 1.1), r["track"], 1.0, 1.0)
    assert (v, om) == (rv, rw)
    p.reset()
    assert p.path is None
    p.close()


def test_goal_pieces_whose_end_is_nearest_a_box_edge(env):
    """Boundary edges cut short, as walls cut them: rotated boxes beside a piece's end, where the end projected onto a box edge is strictly nearer than
    every vertex pair -- a branch that whole edges never reach."""
    from benchpush_amd.planning import GTSPConfig
    goals = np.asarray([[[-5.0, 1.5], [-5.0, 5.0]], [[1.5, 5.0], [5.0, 5.0]], [[5.0, 5.0], [5.0, 1.5]], [[-1.5, -5.0], [-5.0, -5.0]]])
    rng = np.random.default_rng(3)
    poses, boxes, counts = rng.uniform(-3, 3, (E, 3)), np.zeros((E, 13, 20, 2)), np.zeros((E, 13), np.int32)
    boxes[0, 0, :4], counts[0, 0] = sq(3.6, 0.0, math.pi / 4, 0.9), 4           # the diamond below the end (5, 1.5) of piece 2
    boxes[1, 0, :4], boxes[1, 1, :4], counts[1, :2] = sq(3.6, 0.0, math.pi / 4, 0.9)[::-1], sq(-0.2, 3.4, 0.5, 0.8), 4
    for e in range(2, E):
        for b in range(e // 2):
            boxes[e, b, :4], counts[e, b] = sq(rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, math.pi / 2), rng.uniform(0.6, 1.0)), 4
    box = [tuple(v) for v in boxes[0, 0, :4].tolist()]
    poly = R.shrink(box, 0.4)
    bp, gp, deg = R.nearest_pair(box, poly, (5.0, 5.0), (5.0, 1.5))
    assert not deg and gp == (5.0, 1.5) and min(math.hypot(bp[0] - v[0], bp[1] - v[1]) for v in poly) > 0.2      # the end, and the inside of an edge
    cfg = GTSPConfig(max_boxes=4)
    plan = env.gtsp_plan(dev(poses), dev(boxes), dev(counts), dev(goals.reshape(-1, 4)), config=cfg, return_weights=True)
    host = {k: getattr(plan, k).cpu().numpy() for k in plan._fields}
    ref = [R.plan(poses[e], boxes[e], counts[e], goals, BD, cfg=dict(max_boxes=4)) for e in range(E)]
    ends = 0
    for e in range(E):
        _check(host, ref, e, 4)
        for b in ref[e]["clusters"]:
            box = [tuple(v) for v in boxes[e, b, :4].tolist()]
            poly = R.shrink(box, 0.4)
            for g in goals.tolist():
                bp, gp, deg = R.nearest_pair(box, poly, tuple(g[0]), tuple(g[1]))
                ends += not deg and list(gp) in g and bp not in poly
    print("routes that start inside a box edge, opposite a piece's end: %d" % ends)
    assert [r["n_push"] for r in ref] == [1, 2, 1, 1, 2, 2, 3, 3] and ends >= 2          # the diamond in either winding, at the least
