"""bp_lattice_search / BatchedShipIceEnv.lattice_search on the GPU: == the numpy + heapq restatement (tests/lattice_ref.py) on status, g, expanded,
n_nodes, nodes and edges; the reference-generated goldens; NO_PATH, CAP, SKIPPED; refusals; no side effect; lattice_full_paths; the example planner.

Observed with the restatement on the shapes below (defaults: max_expansions 8192, node and queue capacity 16384, max_path_nodes 128), maxima over
the found cases: the batch (8 headings) 132 expansions, 311 nodes seen, 260 queue entries, 8 path nodes; the 16-heading case 99 / 413 / 608 / 7; the
golden cases 634 / 1126 / 713 / 19.  Every one stays below a quarter of its default cap.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

import lattice_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 6
H, W = 120, 40
THETA0 = [math.pi / 2, 0.0, 1.2, 2.0, math.pi / 2, 1.7]          # exactly pi / 2 and 0, generic ones
START_X = [20.0, 14.0, 9.5, 30.5, 32.0, 8.0]                      # the last four hug a side wall: edges leave the window and cost +inf
START_Y = [20.0, 18.0, 22.3, 16.9, 19.4, 21.2]
AHEAD = [60.0, 45.0, 6.0, 50.0, 55.0, 7.5]                        # 6.0 and 7.5 lie within the turning radius: the acos branch of the heuristic runs


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@pytest.fixture(scope="module")
def golden():
    return LR.load_golden()


@pytest.fixture(scope="module")
def env():
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    e = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, trials=default_trials(0.3, 2, base_seed=21), device=DEV)
    e.reset()
    yield e
    e.check_errors()
    e.close()


@pytest.fixture(scope="module")
def ship_fp():
    from benchpush_amd.planning import LATTICE_SHIP_VERTICES, ship_footprint
    return ship_footprint(LATTICE_SHIP_VERTICES, 5, 0.25)


def make_prims(M, nh):
    from benchpush_amd.planning import LatticePrimitives
    s = M["set_%d" % nh]
    return LatticePrimitives(s["edges"], nh, M["scale"], s["turning_radius"], M["step_size"])


@pytest.fixture(scope="module")
def prims8(golden):
    return make_prims(golden[1], 8)


def sparse_maps(seed, n):
    """Maps with large zero regions: g ties, and a node that is already queued is reached again more cheaply."""
    rs = np.random.RandomState(seed)
    return rs.uniform(0.0, 10.0, (n, H, W)) * (rs.uniform(0.0, 1.0, (n, H, W)) < 0.15)


@pytest.fixture(scope="module")
def batch(env, prims8, ship_fp):
    """Starts, goals, per-env masks rasterised on the device (and read back for the restatement) and the maps of the batch test."""
    from benchpush_amd.planning import lattice_max_val, lattice_swath_masks
    masks = lattice_swath_masks(env, prims8, ship_fp, dev(np.array(THETA0)))
    torch.cuda.synchronize()
    T = LR.tables_from_prims(prims8, lattice_max_val(prims8, ship_fp))
    assert tuple(masks.shape) == (E, 8 * prims8.ne_max, T.S) and masks.dtype == torch.int64
    starts = np.stack([START_X, START_Y, THETA0], 1)
    goal_y = np.array(START_Y) + np.array(AHEAD)
    return {"T": T, "masks": masks, "masks_np": masks.cpu().numpy(), "starts": starts, "goal_y": goal_y, "maps": sparse_maps(5, E)}


def run(env, prims, maps, starts, goal_y, masks, **kw):
    active = kw.pop("active", None)
    r = env.lattice_search(maps if isinstance(maps, torch.Tensor) else dev(maps), dev(starts), dev(goal_y), prims,
                           masks if isinstance(masks, torch.Tensor) else dev(masks), active=None if active is None else dev(np.asarray(active)), **kw)
    torch.cuda.synchronize()
    return r


def restate(T, maps, starts, goal_y, masks, margin=25, **kw):
    kw.setdefault("max_expansions", 8192)                      # the defaults of BatchedShipIceEnv.lattice_search
    kw.setdefault("max_path_nodes", 128)
    kw.setdefault("node_capacity", 2 * kw["max_expansions"])
    kw.setdefault("queue_capacity", 2 * kw["max_expansions"])
    out = []
    for e in range(len(starts)):
        cm = maps[e] if maps.ndim == 3 else maps
        mk = masks[e] if masks.ndim == 3 else masks
        out.append(LR.lattice_search(cm, starts[e], goal_y[e], T, mk, margin=margin, **kw))
    return out


def assert_equal(res, want, what=""):
    st, g, ex, nn = (t.cpu().numpy() for t in (res.status, res.g, res.expanded, res.n_nodes))
    nodes, edges = res.nodes.cpu().numpy(), res.edges.cpu().numpy()
    for e, w in enumerate(want):
        tag = "%s env %d" % (what, e)
        assert st[e] == w.status, (tag, st[e], w.status)
        assert g[e] == w.g, (tag, g[e], w.g)
        assert ex[e] == w.expanded, (tag, ex[e], w.expanded)
        assert nn[e] == w.n_nodes, (tag, nn[e], w.n_nodes)
        assert np.array_equal(nodes[e, :w.n_nodes], w.nodes), tag
        assert np.array_equal(edges[e, :w.n_nodes], w.edges), tag


@pytest.mark.parametrize("weight,h_baseline,shared", [(1.0, False, False), (0.0, False, True), (2.5, False, False), (1.0, True, False)])
def test_device_equals_restatement_on_the_batch(env, prims8, batch, weight, h_baseline, shared):
    maps = batch["maps"][3] if shared else batch["maps"]
    goal_y = batch["goal_y"] if weight else np.minimum(batch["goal_y"], batch["starts"][:, 1] + 30.0)   # f = g expands far more: nearer goals
    res = run(env, prims8, maps, batch["starts"], goal_y, batch["masks"], weight=weight, h_baseline=h_baseline)
    want = restate(batch["T"], maps, batch["starts"], goal_y, batch["masks_np"], weight=weight, h_baseline=h_baseline)
    assert_equal(res, want, "w=%s base=%s" % (weight, h_baseline))
    assert sum(w.status == LR.FOUND for w in want) >= 3
    if weight == 1.0 and not h_baseline:
        assert any(w.improved > 0 for w in want) and max(w.max_queue for w in want) > 64
        # the acos branch ran: a near goal with the turning circle's centre beyond it
        assert any(batch["starts"][e, 1] + 10.0 * abs(math.sin(THETA0[e])) >= batch["goal_y"][e] > batch["starts"][e, 1] for e in range(E))


def test_sixteen_headings(env, golden, ship_fp):
    from benchpush_amd.planning import lattice_max_val, lattice_swath_masks
    p16 = make_prims(golden[1], 16)
    assert max(len(es) for es in p16.edges) > 9
    th0 = np.array([math.pi / 2, 1.45, math.pi / 2, 1.7, 1.3, math.pi / 2])
    masks = lattice_swath_masks(env, p16, ship_fp, dev(th0))
    T = LR.tables_from_prims(p16, lattice_max_val(p16, ship_fp))
    starts = np.stack([[20.0, 15.5, 24.0, 18.2, 21.7, 19.1], [30.0, 31.2, 29.5, 33.3, 30.8, 32.1], th0], 1)
    goal_y = starts[:, 1] + np.array([25.0, 30.0, 3.0, 28.0, 22.0, 35.0])
    maps = sparse_maps(9, E)
    res = run(env, p16, maps, starts, goal_y, masks)
    want = restate(T, maps, starts, goal_y, masks.cpu().numpy())
    assert_equal(res, want, "16 headings")
    assert sum(w.status == LR.FOUND for w in want) >= 4


def test_golden_cases_with_the_references_own_masks(env, prims8, golden):
    G, M = golden
    kept = [n for n, c in enumerate(M["cases"]) if c["kept"]]
    assert len(kept) >= 10
    nem, u = M["ne_max"], M["scale"] / 2
    for lot in (kept[:E], kept[E:2 * E]):
        ids = (lot + lot[:E])[:E]                                  # a short lot is filled up with repeats
        cases = [M["cases"][n] for n in ids]
        maps = np.stack([LR.golden_map(c["seed"], M["H"], M["W"]) for c in cases])
        masks = np.stack([G["masks_%d" % n] for n in ids])
        starts = np.array([c["start"] for c in cases])
        res = run(env, prims8, maps, starts, np.array([c["goal_y"] for c in cases]), masks, margin=cases[0]["margin"])
        st, g, ex, nn = (t.cpu().numpy() for t in (res.status, res.g, res.expanded, res.n_nodes))
        nodes, edges = res.nodes.cpu().numpy(), res.edges.cpu().numpy()
        for e, (n, c) in enumerate(zip(ids, cases)):
            assert st[e] == LR.FOUND and nn[e] == c["n_nodes"] and ex[e] == c["expanded_restated"] and g[e] == c["g_restated"], (n, st[e], g[e], ex[e])
            assert abs(g[e] - c["g_ref"]) <= LR.golden_rtol(M["S"] * M["S"] * c["n_nodes"]) * c["g_ref"]
            ref = G["node_path_%d" % n]
            assert np.abs(nodes[e, :nn[e], :2] - ref[:, :2]).max() < 1e-6      # the reference accumulates its float nodes
            dth = np.abs(np.remainder(nodes[e, :nn[e], 2] - ref[:, 2] + math.pi, 2 * math.pi) - math.pi)
            assert dth.max() < 1e-9
            walk = [(0, 0, 0)]                                     # the integer node path that the device's edges spell == the reference's
            for eid in edges[e, 1:nn[e]]:
                i, j, h = walk[-1]
                ex_, ey_, eh = prims8.edges[eid // nem][eid % nem]
                rx, ry = LR.rot_edge(int(ex_ * 2), int(ey_ * 2), h // 2)
                walk.append((i + rx, j + ry, LR.succ_heading(h, eh, 2, 8)))
            assert walk == [tuple(v) for v in G["inodes_%d" % n].tolist()], n
            assert edges[e, 0] == -1 and u == 2.5


def test_no_path_two_kinds(env, prims8, batch):
    narrow = np.random.RandomState(2).uniform(0.0, 1.0, (H, 12))   # 12 cells wide and the ship lies across it: every edge's swath leaves the map
    starts = np.stack([[6.0] * E, START_Y, [0.0] * E], 1)
    across, across_np = batch["masks"][1].contiguous(), batch["masks_np"][1]      # the masks of theta0 = 0, shared by all envs
    res = run(env, prims8, narrow, starts, starts[:, 1] + 40.0, across)
    want = restate(batch["T"], narrow, starts, starts[:, 1] + 40.0, across_np)
    assert_equal(res, want, "narrow")
    assert all(w.status == LR.NO_PATH and w.expanded == 1 for w in want)
    goal_y = batch["starts"][:, 1] - np.array([0.0, 1.0, 5.0, 0.0, 30.0, 2.5])      # at or behind the start: the goal is the start node
    res = run(env, prims8, batch["maps"], batch["starts"], goal_y, batch["masks"])
    assert (res.status.cpu().numpy() == LR.NO_PATH).all() and (res.expanded.cpu().numpy() == 0).all() and (res.n_nodes.cpu().numpy() == 0).all()
    assert torch.isinf(res.g).all()


def test_caps_return_a_status(env, prims8, batch):
    for kw in ({"max_expansions": 5}, {"max_path_nodes": 2}, {"node_capacity": 40}, {"queue_capacity": 30}):
        res = run(env, prims8, batch["maps"], batch["starts"], batch["goal_y"], batch["masks"], **kw)
        want = restate(batch["T"], batch["maps"], batch["starts"], batch["goal_y"], batch["masks_np"], **kw)
        assert_equal(res, want, str(kw))
        assert sum(w.status == LR.CAP for w in want) >= 3, kw


def test_active_mask_skips_and_leaves_rows_untouched(env, prims8, batch):
    from benchpush_amd.envs.ship_ice import LatticeResult
    N = 128
    out = LatticeResult(torch.full((E,), -7, dtype=torch.int32, device=DEV), torch.full((E,), -7.0, dtype=torch.float64, device=DEV),
                        torch.full((E,), -7, dtype=torch.int32, device=DEV), torch.full((E,), -7, dtype=torch.int32, device=DEV),
                        torch.full((E, N, 3), -7.0, dtype=torch.float64, device=DEV), torch.full((E, N), -7, dtype=torch.int32, device=DEV))
    active = np.array([1, 0, 1, 0, 0, 1], bool)
    res = run(env, prims8, batch["maps"], batch["starts"], batch["goal_y"], batch["masks"], active=active, out=out)
    assert res is out
    want = restate(batch["T"], batch["maps"], batch["starts"], batch["goal_y"], batch["masks_np"])
    st = res.status.cpu().numpy()
    for e in range(E):
        if active[e]:
            assert st[e] == want[e].status and float(res.g[e]) == want[e].g and int(res.n_nodes[e]) == want[e].n_nodes
            assert np.array_equal(res.nodes[e, :want[e].n_nodes].cpu().numpy(), want[e].nodes)
            assert (res.nodes[e, want[e].n_nodes:] == -7.0).all() and (res.edges[e, want[e].n_nodes:] == -7).all()
        else:
            assert st[e] == LR.SKIPPED and float(res.g[e]) == -7.0 and int(res.expanded[e]) == -7 and int(res.n_nodes[e]) == -7
            assert (res.nodes[e] == -7.0).all() and (res.edges[e] == -7).all()


def test_refusals_write_nothing(env, prims8, batch, golden):
    from benchpush_amd._lib import BpError
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    from benchpush_amd.envs.ship_ice import LatticeResult
    from benchpush_amd.planning import LatticePrimitives
    N = 128
    out = LatticeResult(torch.full((E,), -7, dtype=torch.int32, device=DEV), torch.full((E,), -7.0, dtype=torch.float64, device=DEV),
                        torch.full((E,), -7, dtype=torch.int32, device=DEV), torch.full((E,), -7, dtype=torch.int32, device=DEV),
                        torch.full((E, N, 3), -7.0, dtype=torch.float64, device=DEV), torch.full((E, N), -7, dtype=torch.int32, device=DEV))

    def unchanged():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (out.status, out.g, out.expanded, out.n_nodes, out.nodes, out.edges))

    maps, starts, goal_y, masks = dev(batch["maps"]), dev(batch["starts"]), dev(batch["goal_y"]), batch["masks"]
    wide = torch.zeros((8 * prims8.ne_max, 65), dtype=torch.int64, device=DEV)
    with pytest.raises(BpError):
        env.lattice_search(maps, starts, goal_y, prims8, wide, out=out)                       # S = 65
    assert unchanged()
    maze = BatchedMazeEnv(E, cfg={"num_obstacles": 20}, num_layouts=2, device=DEV)
    maze.reset()
    with pytest.raises(BpError):
        maze.lattice_search(maps, starts, goal_y, prims8, masks, out=out)                     # a handle of another task
    maze.close()
    assert unchanged()
    bad = make_prims(golden[1], 8)
    bad.edges[1][2] = (1.25, 1.5, 1)                                                          # not a multiple of the sub-unit 1 / 2
    with pytest.raises(BpError):
        env.lattice_search(maps, starts, goal_y, bad, masks, out=out)
    assert unchanged()
    L, cfg = env.L, None
    import ctypes as C
    from benchpush_amd import _lib
    e, hd, ln, cnt = prims8.tables()
    S = int(masks.shape[-1])
    cfg = _lib.BpLatticeConfig(H=H, W=W, S=S, nh=8, nb=2, ne_max=prims8.ne_max, den=2, margin=25, h_baseline=0, max_expansions=100, node_capacity=400,
                               queue_capacity=400, max_path_nodes=N, pad_=0, map_stride=H * W, mask_stride=8 * prims8.ne_max * S, unit=5.0, weight=1.0,
                               turning_radius=10.0)
    need = int(L.bp_lattice_workspace_bytes(C.byref(cfg), E))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())        # noqa: E731
    call = lambda nbytes: L.bp_lattice_search(env.h, C.byref(cfg), p(maps), p(starts), p(goal_y), None, hp(e), hp(hd), hp(ln), hp(cnt), p(masks), p(ws),   # noqa: E731
                                              nbytes, p(out.status), p(out.g), p(out.expanded), p(out.n_nodes), p(out.nodes), p(out.edges), env._stream())
    assert call(need - 1) == -1 and unchanged()                                               # a short workspace
    cfg.max_expansions = 0
    assert call(need) == -1 and unchanged()
    cfg.max_expansions, cfg.nh = 100, 12
    assert call(need) == -1 and unchanged()
    cfg.nh = 8
    assert call(need) == 0
    torch.cuda.synchronize()
    assert not unchanged()
    for args in ((maps.float(), starts, goal_y, prims8, masks), (maps, starts.cpu(), goal_y, prims8, masks), (maps, starts[:, :2].contiguous(), goal_y, prims8, masks),
                 (maps, starts, goal_y[:3].contiguous(), prims8, masks), (maps, starts, goal_y, prims8, masks.int()), (maps, starts, goal_y, prims8, masks[:, :5].contiguous())):
        with pytest.raises(ValueError):
            env.lattice_search(*args)


def test_planning_leaves_the_envs_alone(prims8, batch):
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    envs = [BatchedShipIceEnv(E, cfg={"concentration": 0.3}, trials=default_trials(0.3, 2, base_seed=33), device=DEV) for _ in range(2)]
    obs = [e.reset()[0] for e in envs]
    assert torch.equal(obs[0], obs[1])
    rng = np.random.RandomState(4)
    for t in range(3):
        a = dev(rng.uniform(-1, 1, E))
        if t:
            run(envs[1], prims8, batch["maps"], batch["starts"], batch["goal_y"], batch["masks"])
        outs = [e.step(a) for e in envs]
        for x, y in zip(outs[0][:4], outs[1][:4]):
            assert torch.equal(x, y)
        assert torch.equal(envs[0].info, envs[1].info)
    for e in envs:
        e.check_errors()
        e.close()


def test_full_paths_against_a_numpy_assembly(env, prims8, batch):
    from benchpush_amd.planning import lattice_full_paths
    res = run(env, prims8, batch["maps"], batch["starts"], batch["goal_y"], batch["masks"])
    paths, lengths = lattice_full_paths(prims8, res, dev(batch["starts"]))
    torch.cuda.synchronize()
    paths, lengths = paths.cpu().numpy(), lengths.cpu().numpy()
    nodes, edges, nn = res.nodes.cpu().numpy(), res.edges.cpu().numpy(), res.n_nodes.cpu().numpy()
    assert (nn > 1).any()
    for e in range(E):
        parts = []
        for a in range(max(nn[e] - 1, 0)):
            b, k = divmod(int(edges[e, a + 1]), prims8.ne_max)
            sm = prims8.samples(b, k)
            th = nodes[e, a, 2] - b * prims8.spacing
            c, s = np.cos(th), np.sin(th)
            parts.append(np.stack([c * sm[0] - s * sm[1] + nodes[e, a, 0], s * sm[0] + c * sm[1] + nodes[e, a, 1], np.remainder(sm[2] + th, 2 * np.pi)], 1))
        want = np.concatenate(parts) if parts else np.zeros((0, 3))
        assert lengths[e] == len(want)
        got = paths[e, :lengths[e]]
        assert np.abs(got[:, :2] - want[:, :2]).max(initial=0.0) < 1e-9
        assert np.abs(np.remainder(got[:, 2] - want[:, 2] + np.pi, 2 * np.pi) - np.pi).max(initial=0.0) < 1e-9
        assert (paths[e, lengths[e]:] == 0).all()


def test_example_lattice_planner_runs_three_steps():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import lattice_planner
    finished, found = lattice_planner.run(envs=4, steps=3, every=1)
    assert found > 0
