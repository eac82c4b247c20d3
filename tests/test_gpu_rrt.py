"""bp_rrt_plan on the device (-m gpu): the kernel against the scalar restatement (tests/rrt_ref.py), ``==`` on every output; properties of found
plans that do not lean on the restatement; refusals before launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rrt_ref as R

pytestmark = pytest.mark.gpu

V = 6
SMALL = dict(step=0.25, max_nodes=2000, max_waypoints=64)
# a 4 x 3 room, a divider with a door at y in (1.2, 1.8), and a closed chamber in the upper right corner that no path enters
ROOM = [[0, 0, 4, 0], [4, 0, 4, 3], [4, 3, 0, 3], [0, 3, 0, 0], [2, 0, 2, 1.2], [2, 1.8, 2, 3], [3.2, 3, 3.2, 2.2], [3.2, 2.2, 4, 2.2]]
RADIUS = 0.1


def square(cx, cy, h):
    return [(cx - h, cy - h), (cx + h, cy - h), (cx + h, cy + h), (cx - h, cy + h)]


def env_spec(e):
    """Start, goal and boxes of env e: ten kinds, so that a batch of 70 holds every status several times."""
    rng = np.random.RandomState(1000 + e)
    kind = e % 10
    start, goal = [0.5 + 0.8 * rng.rand(), 0.5 + 2.0 * rng.rand()], [2.6 + 0.4 * rng.rand(), 0.5 + 1.2 * rng.rand()]
    boxes = []
    if kind in (1, 4, 7):        # boxes in the way, clockwise and anticlockwise, a triangle and a hexagon
        boxes = [square(1.2, 0.8 + rng.rand(), 0.2)[::-1], [(2.6, 2.0), (3.0, 2.4), (2.5, 2.6)],
                 [(2.9 + 0.15 * math.cos(a), 0.4 + 0.15 * math.sin(a)) for a in np.arange(6) * math.pi / 3]]
    if kind == 2:                # a box closes the door: pass 0 uses up max_nodes, pass 1 goes through the box
        boxes = [[(1.9, 1.0), (2.1, 1.0), (2.1, 2.0), (1.9, 2.0)]]
    if kind == 3 and e % 20 == 3:   # the goal inside the chamber: both passes use up max_nodes
        goal = [3.6, 2.6]
    if kind == 5:                # within the inflated wall
        start = [0.05, 1.0] if e % 20 == 5 else start
        goal = goal if e % 20 == 5 else [2.05, 0.5]
    if kind == 6:                # on the other side of the room, start on the right
        start, goal = goal, start
    if kind == 8:                # start inside a box: every segment from it meets the box, pass 1 finds
        boxes = [square(start[0], start[1], 0.15)]
    if kind == 9:                # a short hop
        goal = [start[0] + 0.3, start[1] + 0.1]
    return start, goal, boxes


def pack(specs, nbox=3):
    E = len(specs)
    boxes, counts = np.zeros((E, nbox, V, 2)), np.zeros((E, nbox), np.int32)
    for e, (_, _, bx) in enumerate(specs):
        for b, poly in enumerate(bx):
            if len(poly):
                boxes[e, b, :len(poly)], counts[e, b] = poly, len(poly)
    return (np.array([s[0] for s in specs], np.float64), np.array([s[1] for s in specs], np.float64), boxes, counts)


_envs = {}


def maze_env(E):
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    if E not in _envs:
        _envs[E] = BatchedMazeEnv(E, num_layouts=1, device="cuda:0")
        _envs[E].reset()
    return _envs[E]


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype)


def launch(env, starts, goals, walls, boxes, counts, streams, cfg, active=None, inflate=RADIUS, **kw):
    from benchpush_amd.planning import RRTConfig
    config = RRTConfig(inflate_radius=inflate, **cfg)
    out = env.rrt_plan(dev(starts), dev(goals), dev(np.asarray(walls, np.float64).reshape(-1, 4)), dev(boxes), dev(counts), dev(np.asarray(streams, np.int64)),
                       None if active is None else dev(np.asarray(active, np.uint8)), config=config, **kw)
    torch.cuda.synchronize()
    env.check_errors()
    return out


def assert_equal(out, want, E):
    status, nn, it, paths, lengths, _ = want
    got = [t.cpu().numpy() for t in out]
    assert np.array_equal(got[0], status[:E]), (got[0], status[:E])
    assert np.array_equal(got[1], nn[:E]) and np.array_equal(got[2], it[:E]), (got[1], nn[:E], got[2], it[:E])
    assert np.array_equal(got[4], lengths[:E])
    assert np.array_equal(got[3], paths[:E])           # ==, rows past the length untouched zeros included


@pytest.fixture(scope="module")
def batch70():
    """70 envs' inputs and what the restatement plans for them, computed once."""
    specs = [env_spec(e) for e in range(70)]
    specs[11] = specs[10]                               # equal scenes ...
    starts, goals, boxes, counts = pack(specs)
    starts[1, 0] = math.nan                             # a non-finite start
    streams = 7_000_000_000 + np.arange(70) * 3
    streams[11] = streams[10]                           # ... and equal streams
    active = np.ones(70, np.uint8)
    active[2] = 0
    cfg = dict(SMALL)
    want = R.rrt_plan_batch(starts, goals, ROOM, boxes, counts, streams, dict(cfg, inflate_radius=RADIUS), active)
    return starts, goals, boxes, counts, streams, active, cfg, want


def test_the_batch_holds_every_case(batch70):
    status, nn = batch70[7][0], batch70[7][1]
    for s in (R.FOUND, R.FOUND_IGNORING_BOXES, R.FALLBACK, R.BLOCKED, R.BAD_INPUT, R.SKIPPED):
        assert (status == s).sum() >= 1, s
    found = status == R.FOUND
    assert nn[found, 0].min() < 64 and ((nn[found, 0] > 64) & (nn[found, 0] < 128)).any() and nn[found, 0].max() > 128      # below one lane round, two, more
    two = status == R.FOUND_IGNORING_BOXES
    assert (batch70[7][2][two, 0] == SMALL["max_nodes"]).all()      # pass 0 used up its iterations
    assert status[1] == R.BAD_INPUT and status[2] == R.SKIPPED


@pytest.mark.parametrize("E", [1, 3, 70])
def test_kernel_equals_restatement(batch70, E):
    """A plan depends on the env's own inputs and its stream only: the first E envs of the batch of 70, planned as a batch of E, give the same rows."""
    starts, goals, boxes, counts, streams, active, cfg, want = batch70
    out = launch(maze_env(E), starts[:E], goals[:E], ROOM, boxes[:E], counts[:E], streams[:E], cfg, active[:E])
    assert_equal(out, want, E)
    if E == 70:
        got = [t.cpu().numpy() for t in out]
        assert got[0][10] in (R.FOUND, R.FOUND_IGNORING_BOXES) and all(np.array_equal(g[10], g[11]) for g in got)     # equal streams, equal scenes
        assert not np.array_equal(got[3][10], got[3][20])


@pytest.mark.parametrize("lds_nodes", [0, 64, 512, 2048])
def test_nodes_in_lds_change_nothing(batch70, lds_nodes, monkeypatch):
    """BP_RRT_LDS_NODES: the nearest search reads the first nodes of the tree from LDS.  64: most trees of the batch outgrow the prefix; 2048: none does."""
    monkeypatch.setenv("BP_RRT_LDS_NODES", str(lds_nodes))
    starts, goals, boxes, counts, streams, active, cfg, want = batch70
    assert_equal(launch(maze_env(70), starts, goals, ROOM, boxes, counts, streams, cfg, active), want, 70)


def test_env_alone_and_elsewhere_in_a_batch(batch70):
    """Env 14 of the batch planned alone, and as env 0 and env 2 of a batch of 3."""
    starts, goals, boxes, counts, streams, active, cfg, want = batch70
    pick = np.array([14, 33, 14])
    out = launch(maze_env(3), starts[pick], goals[pick], ROOM, boxes[pick], counts[pick], streams[pick], cfg)
    one = launch(maze_env(1), starts[14:15], goals[14:15], ROOM, boxes[14:15], counts[14:15], streams[14:15], cfg)
    for g3, g1, w in zip(out, one, want[:5]):
        g3, g1 = g3.cpu().numpy(), g1.cpu().numpy()
        assert np.array_equal(g3[0], w[14]) and np.array_equal(g3[2], w[14]) and np.array_equal(g1[0], w[14]) and np.array_equal(g3[1], w[33])


@pytest.mark.parametrize("segments", [5, 64, 65])
def test_segment_counts_around_one_lane_round(segments):
    """Walls plus box edges of 5, 64 and 65: below, at and one past the 64 segments that the lanes test per round."""
    if segments == 5:
        walls, nsq = [[0, 0, 4, 0], [0, 3, 4, 3]], 0
    else:
        walls, nsq = ROOM[:4] + ([[2, 0, 2, 1.2]] if segments == 65 else []), 15
    sq = [square(0.9 + 0.55 * (i % 5), 0.6 + 0.8 * (i // 5), 0.08) for i in range(nsq)]
    specs = [([0.4, 0.4 + 0.3 * e], [3.6, 2.5 - 0.2 * e], sq + ([[(2.0, 1.3), (2.3, 1.5), (1.9, 1.7)]] if segments == 5 else [])) for e in range(3)]
    if segments != 5:
        specs[2] = (specs[2][0], specs[2][1], sq[:14] + [[]])     # a skipped polygon in the last slot
    starts, goals, boxes, counts = pack(specs, nbox=max(1, nsq))
    assert len(walls) + counts[0].sum() == segments
    streams = [5, 6, 7]
    want = R.rrt_plan_batch(starts, goals, walls, boxes, counts, streams, dict(SMALL, inflate_radius=RADIUS))
    assert (want[0] == R.FOUND).all()
    assert_equal(launch(maze_env(3), starts, goals, walls, boxes, counts, streams, SMALL), want, 3)


def test_small_trees_cap_and_single_pass():
    specs = [env_spec(e) for e in (0, 1, 2)]
    starts, goals, boxes, counts = pack(specs)
    streams = [11, 12, 13]
    # a goal bias of one half: trees of a few nodes
    cfg = dict(SMALL, goal_bias=0.5)
    want = R.rrt_plan_batch(starts, goals, ROOM, boxes, counts, streams, dict(cfg, inflate_radius=RADIUS))
    assert want[1][0, 0] < 64
    assert_equal(launch(maze_env(3), starts, goals, ROOM, boxes, counts, streams, cfg), want, 3)
    # four rows for paths of nine and more waypoints: CAP, length 0, the first four waypoints written
    cfg = dict(SMALL, max_waypoints=4)
    want = R.rrt_plan_batch(starts, goals, ROOM, boxes, counts, streams, dict(cfg, inflate_radius=RADIUS))
    assert (want[0] == R.CAP).any() and (want[4][want[0] == R.CAP] == 0).all()
    assert_equal(launch(maze_env(3), starts, goals, ROOM, boxes, counts, streams, cfg), want, 3)
    # passes = 1: the env whose door a box closes falls back instead of going through the box
    cfg = dict(SMALL, passes=1)
    want = R.rrt_plan_batch(starts, goals, ROOM, boxes, counts, streams, dict(cfg, inflate_radius=RADIUS))
    assert want[0][2] == R.FALLBACK and want[4][2] == 2
    assert_equal(launch(maze_env(3), starts, goals, ROOM, boxes, counts, streams, cfg), want, 3)
    # a count outside 0, 3 .. V is a bad input
    counts2 = counts.copy()
    counts2[0, 0], counts2[1, 0] = 2, V + 1
    want = R.rrt_plan_batch(starts, goals, ROOM, boxes, counts2, streams, dict(SMALL, inflate_radius=RADIUS))
    assert want[0][0] == R.BAD_INPUT and want[0][1] == R.BAD_INPUT
    assert_equal(launch(maze_env(3), starts, goals, ROOM, boxes, counts2, streams, SMALL), want, 3)


@pytest.mark.parametrize("version", [1, 2])
def test_reference_parameters_on_the_maze(version):
    """The reference's parameters (step 0.05, 26000 nodes, inflate radius 2.25 * min_r) on the env's own layout, all defaults of rrt_plan, E = 2."""
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    env = BatchedMazeEnv(2, cfg={"maze_version": version}, num_layouts=1, device="cuda:0")
    env.reset()
    out = env.rrt_plan()
    boxes, counts = env.box_polys()
    torch.cuda.synchronize()
    starts = env.info[:, :2].cpu().numpy()
    goals = np.array([[env.cfg.env.goal_x, env.cfg.env.goal_y]] * 2, np.float64)
    want = R.rrt_plan_batch(starts, goals, env.walls, boxes.cpu().numpy(), counts.cpu().numpy(), [0, 1],
                            dict(inflate_radius=2.25 * env.cfg.robot.min_r))
    print("maze version %d: status %s, nodes %s, iterations %s, waypoints %s" % (version, want[0], want[1].tolist(), want[2].tolist(), want[4]))
    assert (want[0] <= R.FOUND_IGNORING_BOXES).all() and want[2].max() > 1000
    assert_equal(out, want, 2)
    env.close()


def _wall_distance(p, walls):
    best = math.inf
    for ax, ay, bx, by in walls:
        abx, aby = bx - ax, by - ay
        t = min(1.0, max(0.0, ((p[0] - ax) * abx + (p[1] - ay) * aby) / (abx * abx + aby * aby)))
        best = min(best, math.hypot(p[0] - ax - t * abx, p[1] - ay - t * aby))
    return best


def test_found_plans_are_paths(batch70):
    """Independent of the restatement, from the tree that the kernel leaves in the workspace: every found plan starts at the start and ends at the goal
    (start + 1.0 * (goal - start) rounds to the goal here: the coordinates are within a factor of two of each other), no tree edge is longer than
    step * (1 + 1e-12), and the path through the tree, sampled every 0.002, keeps inflate_radius - 1e-9 from every wall."""
    starts, goals, boxes, counts, streams, active, cfg, _ = batch70
    env = maze_env(70)
    ws = torch.zeros(env.rrt_workspace_bytes(__import__("benchpush_amd.planning", fromlist=["RRTConfig"]).RRTConfig(**cfg)), dtype=torch.uint8, device="cuda:0")
    out = launch(env, starts, goals, ROOM, boxes, counts, streams, cfg, active, workspace=ws)
    status, nn, _, paths, lengths = [t.cpu().numpy() for t in out]
    per = ws.numel() // 70
    raw = ws.cpu().numpy()
    cap = cfg["max_nodes"] + 2
    checked = 0
    for e in np.flatnonzero(status <= R.FOUND_IGNORING_BOXES):
        n = nn[e, status[e]]
        nodes = raw[e * per: e * per + cap * 16].view(np.float64).reshape(cap, 2)[:n]
        parents = raw[e * per + cap * 16: e * per + cap * 20].view(np.int32)[:n]
        assert parents[0] == -1 and (parents[1:] >= 0).all() and (parents[1:] < np.arange(1, n)).all()
        assert np.array_equal(paths[e, 0], starts[e]) and np.array_equal(paths[e, lengths[e] - 1], goals[e])
        assert np.array_equal(nodes[0], starts[e]) and np.array_equal(nodes[n - 1], goals[e])
        edge = np.hypot(*(nodes[1:] - nodes[parents[1:]]).T)
        assert edge.max() <= cfg["step"] * (1 + 1e-12)
        idx, chain = n - 1, []
        while idx != -1:
            chain.append(nodes[idx])
            idx = parents[idx]
        for a, b in zip(chain[:-1], chain[1:]):
            for t in np.linspace(0.0, 1.0, int(np.hypot(*(b - a)) / 0.002) + 2):
                assert _wall_distance(a + t * (b - a), ROOM) > RADIUS - 1e-9
        checked += 1
    assert checked >= 40


def test_refusals_come_before_any_launch():
    from benchpush_amd import _lib
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from benchpush_amd.planning import RRTConfig, RRTPlan
    env = maze_env(3)
    starts, goals, boxes, counts = pack([env_spec(e) for e in range(3)])
    args = lambda: (dev(starts), dev(goals), dev(np.asarray(ROOM, np.float64)), dev(boxes), dev(counts), dev(np.arange(3, dtype=np.int64)))   # noqa: E731
    fresh = lambda P=64: RRTPlan(*(torch.full(s, -7, dtype=d, device="cuda:0") for s, d in                                                 # noqa: E731
                                   [((3,), torch.int32), ((3, 2), torch.int32), ((3, 2), torch.int32), ((3, P, 2), torch.float64), ((3,), torch.int32)]))

    def refused(exc, *a, config=None, P=64, **kw):
        out = fresh(P)
        with pytest.raises(exc):
            env.rrt_plan(*a, config=config or RRTConfig(inflate_radius=RADIUS, **SMALL), out=out, **kw)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in out)

    small = torch.zeros(env.rrt_workspace_bytes(RRTConfig(**SMALL)) - 16, dtype=torch.uint8, device="cuda:0")
    refused(_lib.BpError, *args(), workspace=small)
    for bad in (dict(step=0.0), dict(step=-1.0), dict(max_nodes=0), dict(passes=3), dict(goal_radius=math.nan)):
        refused(_lib.BpError, *args(), config=RRTConfig(inflate_radius=RADIUS, **dict(SMALL, **bad)), workspace=torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0"))
    refused(_lib.BpError, *args(), config=RRTConfig(inflate_radius=RADIUS, **dict(SMALL, max_waypoints=1)), P=1)
    a = list(args())
    a[2] = torch.zeros((_lib.RRT_MAX_WALLS + 1, 4), dtype=torch.float64, device="cuda:0")
    refused(_lib.BpError, *a)
    a = list(args())
    a[3], a[4] = torch.zeros((3, 65, 20, 2), dtype=torch.float64, device="cuda:0"), torch.zeros((3, 65), dtype=torch.int32, device="cuda:0")
    refused(_lib.BpError, *a)
    a = list(args())
    a[0] = a[0].float()
    refused(ValueError, *a)
    a = list(args())
    a[1] = a[1].cpu()
    refused(ValueError, *a)
    a = list(args())
    a[5] = a[5][:2]
    refused(ValueError, *a)
    a = list(args())
    a[3] = a[3].transpose(1, 2)
    refused(ValueError, *a)
    with pytest.raises(_lib.BpError):
        env.rrt_workspace_bytes(RRTConfig(step=0.0))
    ship = BatchedShipIceEnv(2, cfg={"concentration": 0.1}, num_trials=1, device="cuda:0")
    ship.reset()
    cfgs = RRTConfig(inflate_radius=RADIUS, **SMALL).as_struct()
    z = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    rc = ship.L.bp_rrt_plan(ship.h, C.byref(cfgs), z.data_ptr(), z.data_ptr(), None, 0, None, None, 0, 0, z.data_ptr(), None, z.data_ptr(), z.numel(),
                            z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None)
    assert rc != 0 and b"maze handles only" in ship.L.bp_last_error(ship.h)
    ship.close()


def test_uniform_on_the_host_is_the_restatement():
    from benchpush_amd import _lib
    L = _lib.load()
    for seed, stream, p, k, j in [(42, 0, 0, 0, 0), (42, 7_000_000_003, 1, 25999, 2), (2 ** 64 - 1, -5, 0, 12345, 1), (0, 2 ** 40 + 17, 1, 1, 0)]:
        assert L.bp_rrt_uniform(seed, stream, p, k, j) == R.rrt_uniform(seed, stream, p, k, j)
