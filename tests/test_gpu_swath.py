"""bp_swath_cost / BatchedShipIceEnv.swath_costs on the GPU: bit-exact against the numpy restatement (tests/swath_ref.py), the reference-generated goldens,
structure, guards, refusals, no side effect, the CostMap adapter and the example planner."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from swath_ref import golden_cost_map, golden_mask, golden_rtol, load_golden, random_arcs, swath_ref, swath_ref_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 4


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@pytest.fixture(scope="module")
def env():
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    e = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, trials=default_trials(0.3, 2, base_seed=21), device=DEV)
    e.reset()
    rng = np.random.RandomState(3)
    for _ in range(3):
        e.step(dev(rng.uniform(-1, 1, E)))
    yield e
    e.check_errors()
    e.close()


@pytest.fixture(scope="module")
def ship_fp():
    from benchpush_amd.planning import LATTICE_SHIP_VERTICES, ship_footprint
    return ship_footprint(LATTICE_SHIP_VERTICES, 5, 0.25)


@pytest.fixture(scope="module")
def map96():
    """Random non-negative 40 x 96 maps (two words per row, the last one partial), one per env, and arcs over them."""
    rng = np.random.RandomState(17)
    maps = rng.uniform(0.0, 5.0, (E, 40, 96)) * (rng.uniform(0, 1, (E, 40, 96)) < 0.6)
    return maps, random_arcs(rng, E, 5, 24, 40, 96)


def run(env, maps, paths, fp, **kw):
    rows = kw.pop("rows", None)
    lengths = kw.pop("lengths", None)
    out = env.swath_costs(dev(paths), dev(fp), dev(maps), lengths=None if lengths is None else dev(np.asarray(lengths), torch.int32),
                          rows=None if rows is None else dev(np.asarray(rows), torch.int32), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


def check_against_restatement(env, maps, paths, fp, **kw):
    for outside in ("clip", "reject"):
        costs, masks = run(env, maps, paths, fp, outside=outside, return_swaths=True, **kw)
        wc, wm = swath_ref_batch(maps, paths, fp, kw.get("lengths"), kw.get("rows"), outside)
        assert np.array_equal(masks, wm), outside
        assert np.array_equal(costs, wc, equal_nan=True), (outside, costs, wc)
    return wc, wm


def test_device_equals_restatement_on_the_envs_own_cost_maps(env, ship_fp):
    maps = env.cost_maps(5, 76, 12, vs=0.3 * 5 + 1e-8)   # 380 x 60: one word per row
    torch.cuda.synchronize()
    maps = maps.cpu().numpy()
    assert maps.shape == (E, 380, 60) and (maps[:, :, 1:-1] > 0).any()
    rng = np.random.RandomState(5)
    paths = random_arcs(rng, E, 4, 32, 380, 60)
    x, y = paths[..., 0], paths[..., 1]
    assert x.min() < 0 and x.max() > 59 and y.min() < 0 and y.max() > 379      # arcs leave the map on each side
    wc, wm = check_against_restatement(env, maps, paths, ship_fp)
    assert np.isinf(wc).any() and np.isfinite(wc).any() and wm.any()


def test_device_equals_restatement_on_two_and_three_word_rows(env, ship_fp, map96):
    maps, paths = map96
    wc, wm = check_against_restatement(env, maps, paths, ship_fp)
    assert wm[..., 64:].any() and wm[..., :64].any() and np.isfinite(wc).any()
    rng = np.random.RandomState(23)                    # 7 x 130: three words per row, fewer rows than the footprint is high
    thin = rng.uniform(0.0, 3.0, (E, 7, 130))
    p = random_arcs(rng, E, 3, 20, 7, 130)
    p[:, 0, :, 1] = 3.0 + 0.37 * np.arange(E)[:, None]   # one candidate per env crosses the strip broadside: its footprint is higher than the map
    p[:, 0, :, 2] = 1.583
    p[:, 0, :, 0] = np.linspace(-5, 140, 20)
    wc, wm = check_against_restatement(env, thin, p, ship_fp)
    assert wm[..., 128:].any() and wm[:, 0].all(axis=1).any()


def test_ties_on_pixel_centres(env, map96):
    """theta exactly 0, pi/2, pi, 3pi/2; x and y at integers and half-integers: footprint edges run through pixel centres and the nose vertex sits on a pixel."""
    maps = map96[0]
    fp = np.array([[4.0, 0.0], [2.0, 1.5], [-3.0, 1.5], [-3.0, -1.5], [2.0, -1.5]])
    thetas = [0.0, math.pi / 2, math.pi, 3 * math.pi / 2]
    paths = np.zeros((E, 4, 4, 3))
    for e in range(E):
        for k in range(4):
            for i in range(4):
                half = 0.5 * ((e + k + i) % 2)
                paths[e, k, i] = (20.0 + 7 * k + i + half, 10.0 + 5 * e + 0.5 * (k % 2) + (i // 2), thetas[(k + e) % 4])
    paths[0, 0, :, :2] = [[5.0, 1.5], [90.0, 38.5], [95.0, 20.0], [0.0, 0.0]]   # ties on the map's own border too
    check_against_restatement(env, maps, paths, fp)
    m, _ = swath_ref(maps[0], np.array([[20.0, 15.5, 0.0]]), fp)   # the ties are ties: nose vertex on pixel (row 15.5 -> none), edges through rows 14 and 17
    assert m[14, 17:23].all() and m[17, 17:23].all() and not m[13].any() and not m[18].any()
    m, _ = swath_ref(maps[0], np.array([[20.0, 15.0, 0.0]]), fp)   # nose vertex exactly on pixel (15, 24), stern edge through column 17
    assert m[15, 24] and m[15, 17] and not m[15, 25] and not m[15, 16]


def test_structure(env, ship_fp, map96):
    maps, paths = map96
    K, P = paths.shape[1:3]
    base_c, base_m = run(env, maps, paths, ship_fp, return_swaths=True)
    # every sample repeated: same swath, same cost
    c, m = run(env, maps, np.repeat(paths, 2, axis=2), ship_fp, return_swaths=True)
    assert np.array_equal(c, base_c) and np.array_equal(m, base_m)
    # permuting the candidates permutes the outputs
    perm = np.array([3, 0, 4, 1, 2])
    c, m = run(env, maps, paths[:, perm], ship_fp, return_swaths=True)
    assert np.array_equal(c, base_c[:, perm]) and np.array_equal(m, base_m[:, perm])
    # lengths 0, 1, P and P + 5 (clamped), and a negative one
    lengths = np.array([[0, 1, P, P + 5, -3]] * E, np.int32)
    wc, wm = check_against_restatement(env, maps, paths, ship_fp, lengths=lengths)
    assert (wc[:, 0] == 0).all() and not wm[:, 0].any() and not wm[:, 4].any() and np.array_equal(wm[:, 2], base_m[:, 2]) and np.array_equal(wm[:, 3], base_m[:, 3])
    # row windows: per candidate (empty, reversed, beyond the map, negative start, a proper one) and per environment
    rows = np.array([[[5, 5], [30, 10], [35, 400], [-7, 12], [8, 31]]] * E, np.int32)
    wc, wm = check_against_restatement(env, maps, paths, ship_fp, rows=rows)
    assert not wm[:, 0].any() and not wm[:, 1].any() and not wm[:, 4, :8].any() and not wm[:, 4, 31:].any() and np.array_equal(wm[:, 4, 8:31], base_m[:, 4, 8:31])
    check_against_restatement(env, maps, paths, ship_fp, rows=np.array([[0, 40], [10, 20], [39, 40], [3, 2]], np.int32))
    # one shared [H, W] map equals its E-fold copy
    shared = run(env, maps[2], paths, ship_fp)
    assert np.array_equal(shared, run(env, np.repeat(maps[2:3], E, axis=0), paths, ship_fp))
    # masks on and off: equal costs; out= buffers are used
    assert np.array_equal(run(env, maps, paths, ship_fp), base_c)
    oc, om = torch.zeros((E, K), dtype=torch.float64, device=DEV), torch.zeros((E, K, 40, 96), dtype=torch.uint8, device=DEV)
    r = env.swath_costs(dev(paths), dev(ship_fp), dev(maps), return_swaths=True, out=(oc, om))
    torch.cuda.synchronize()
    assert r[0] is oc and r[1] is om and np.array_equal(oc.cpu().numpy(), base_c) and np.array_equal(om.cpu().numpy(), base_m)
    # a mask buffer whose rows are not 4-byte aligned (39 x 95 cells) takes the byte path
    check_against_restatement(env, maps[:, :39, :95].copy(), paths, ship_fp)


def test_guards(env, ship_fp, map96):
    maps, paths = map96
    paths = np.concatenate([paths, paths[:, :1]], axis=1)   # K = 6
    bad = paths.copy()
    bad[:, 1, 7, 0] = np.nan
    bad[:, 3, 0, 2] = np.inf
    bad[:, 4, :, :] = 1e300
    good = run(env, maps, paths, ship_fp, return_swaths=True)
    for outside in ("clip", "reject"):
        ref_c, _ = run(env, maps, paths, ship_fp, outside=outside, return_swaths=True)
        c, m = run(env, maps, bad, ship_fp, outside=outside, return_swaths=True)
        wc, wm = swath_ref_batch(maps, bad, ship_fp, outside=outside)
        assert np.array_equal(c, wc, equal_nan=True) and np.array_equal(m, wm)
        assert np.isnan(c[:, 1]).all() and np.isnan(c[:, 3]).all() and not m[:, [1, 3, 4]].any()
        assert (c[:, 4] == (0.0 if outside == "clip" else np.inf)).all()
        for k in (0, 2, 5):                                  # the neighbours are unaffected
            assert np.array_equal(c[:, k], ref_c[:, k]) and np.array_equal(m[:, k], good[1][:, k])
    # a NaN behind the counted samples does not count; a single huge sample among good ones drops out (clip) or rejects
    lengths = np.full((E, 6), 24, np.int32)
    lengths[:, 1] = 7
    mixed = paths.copy()
    mixed[:, 1, 7, 0] = np.nan
    mixed[:, 2, 3, 1] = -4e18
    mixed[:, 0, 5, 2] = 1e22
    check_against_restatement(env, maps, mixed, ship_fp, lengths=lengths)
    env.check_errors()


def test_golden_masks_and_costs(env):
    G, M = load_golden()
    H, W = M["H"], M["W"]
    cm = golden_cost_map(M["map_seed"], H, W)
    n = M["cases"]
    assert n == 24
    paths = G["paths"].reshape(E, n // E, M["P"], 3)
    costs, masks = run(env, cm, paths, G["footprint"], return_swaths=True)
    costs, masks = costs.reshape(n), masks.reshape(n, H, W)
    rtol = golden_rtol(H, W)
    for i in range(n):
        assert np.array_equal(masks[i].astype(bool), golden_mask(G, M, i)), i
        ref = float(G["costs"][i])
        print(i, costs[i], ref, abs(costs[i] - ref) / ref)
        assert abs(costs[i] - ref) <= rtol * ref, i


def test_refusals_write_nothing(env, ship_fp, map96):
    from benchpush_amd._lib import BpError
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    maps, paths = map96
    K = paths.shape[1]
    P, F, M = dev(paths), dev(ship_fp), dev(maps)
    oc = torch.full((E, K), -7.25, dtype=torch.float64, device=DEV)
    om = torch.full((E, K, 40, 96), 9, dtype=torch.uint8, device=DEV)

    def unchanged():
        torch.cuda.synchronize()
        return bool((oc == -7.25).all()) and bool((om == 9).all())

    with pytest.raises(BpError):                              # 21 vertices
        env.swath_costs(P, dev(np.concatenate([ship_fp, ship_fp[:4]])), M, return_swaths=True, out=(oc, om))
    with pytest.raises(BpError):                              # 2 vertices
        env.swath_costs(P, F[:2].contiguous(), M, return_swaths=True, out=(oc, om))
    assert unchanged()
    big = torch.zeros((4097, 8), dtype=torch.float64, device=DEV)   # 4097 words: one above the documented LDS limit
    with pytest.raises(BpError):
        env.swath_costs(P, F, big, out=oc)
    ok = torch.zeros((4096, 8), dtype=torch.float64, device=DEV)    # the limit itself is accepted
    assert bool((env.swath_costs(P, F, ok) == 0).all())
    maze = BatchedMazeEnv(E, cfg={"num_obstacles": 20}, num_layouts=2, device=DEV)
    maze.reset()
    with pytest.raises(BpError):
        maze.swath_costs(P, F, M, return_swaths=True, out=(oc, om))
    maze.close()
    assert unchanged()
    for args in ((P.float(), F, M), (P.cpu(), F, M), (P, F, M.cpu()), (P, F.float(), M), (P.transpose(1, 2), F, M), (P, F, M.transpose(1, 2)),
                 (P[:, :, :, :2].contiguous(), F, M), (P[:2].contiguous(), F, M), (P, F, M[:2].contiguous())):
        with pytest.raises(ValueError):
            env.swath_costs(*args, return_swaths=True, out=(oc, om))
    with pytest.raises(ValueError):
        env.swath_costs(P, F, M, lengths=torch.zeros((E, K), dtype=torch.int64, device=DEV), out=oc)
    with pytest.raises(ValueError):
        env.swath_costs(P, F, M, rows=torch.zeros((E, 3), dtype=torch.int32, device=DEV), out=oc)
    with pytest.raises(ValueError):
        env.swath_costs(P, F, M, outside="ignore", out=oc)
    with pytest.raises(ValueError):
        env.swath_costs(P, F, M, out=torch.zeros((E, K + 1), dtype=torch.float64, device=DEV))
    assert unchanged()
    env.check_errors()


def test_swath_costs_leave_the_environments_alone(ship_fp, map96):
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    maps, paths = map96
    trials = default_trials(0.3, 2, base_seed=21)
    a, b = (BatchedShipIceEnv(2, cfg={"concentration": 0.3}, trials=trials, device=DEV) for _ in range(2))
    acts = [dev(np.array([0.4, -0.8])), dev(np.array([-0.3, 0.9]))]
    for e in (a, b):
        e.reset()
        e.step(acts[0])
    b.swath_costs(dev(paths[:2]), dev(ship_fp), dev(maps[:2]), outside="reject", return_swaths=True)
    b.swath_costs(dev(paths[:2]), dev(ship_fp), b.cost_maps(5, 76, 12))
    outs = [e.step(acts[1]) for e in (a, b)]
    torch.cuda.synchronize()
    assert torch.equal(a.body_state(), b.body_state())
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.check_errors()
        e.close()


def test_costmap_adapter_and_example_planner(env, ship_fp):
    from benchpush_amd.cost_map import CostMap
    cm = CostMap(scale=5, m=76, n=12, alpha=10, ship_mass=1, horizon=None, margin=1, env=env)
    with pytest.raises(ValueError):
        cm.swath_cost(np.zeros((3, 3)), ship_fp)
    cm.update(None, 0.0, vs=0.3 * 5 + 1e-8)
    path = random_arcs(np.random.RandomState(9), 1, 1, 32, 300, 40)[0, 0] + [10.0, 40.0, 0.0]
    swath, cost = cm.swath_cost(path, ship_fp)
    wm, wc = swath_ref(cm.cost_map, path, ship_fp)
    assert swath.dtype == bool and swath.shape == (380, 60) and isinstance(cost, float)
    assert np.array_equal(swath, wm) and cost == wc and swath.any()

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import sampling_planner
    actions = sampling_planner.plan(env, 5)
    torch.cuda.synchronize()
    assert actions.shape == (E,) and actions.dtype == torch.float64 and actions.device.type == "cuda"
    assert bool(torch.isfinite(actions).all()) and bool((actions.abs() <= 1).all())
    env.check_errors()
