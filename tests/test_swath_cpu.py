"""Swath costs without a GPU: the numpy restatement (tests/swath_ref.py) against the goldens written by the reference's own compute_swath_cost and Ship
(tests/golden/make_golden_swath.py), the planning helpers and the ctypes layout of bp_swath_config."""
import ctypes as C

import numpy as np
import pytest
import torch

from swath_ref import golden_cost_map, golden_mask, golden_rtol, load_golden, swath_ref


@pytest.fixture(scope="module")
def gold():
    G, M = load_golden()
    cm = golden_cost_map(M["map_seed"], M["H"], M["W"])
    got = [swath_ref(cm, G["paths"][i], G["footprint"]) for i in range(M["cases"])]
    return G, M, got


def test_restatement_reproduces_every_golden_mask(gold):
    G, M, got = gold
    assert M["cases"] >= 20
    for i, (mask, _) in enumerate(got):
        ref = golden_mask(G, M, i)
        assert ref.any() and np.array_equal(mask, ref), i
    P = G["paths"]   # the cases leave the map on all four sides
    assert (P[..., 0].min() < 0) and (P[..., 0].max() > M["W"] - 1) and (P[..., 1].min() < 0) and (P[..., 1].max() > M["H"] - 1)


def test_restatement_reproduces_every_golden_cost(gold):
    G, M, got = gold
    rtol = golden_rtol(M["H"], M["W"])
    for i, (_, cost) in enumerate(got):
        ref = float(G["costs"][i])
        print(i, cost, ref, abs(cost - ref) / max(ref, 1e-300))
        assert ref > 0 and abs(cost - ref) <= rtol * ref, i


def test_ship_footprint_is_the_reference_ships(gold):
    from benchpush_amd.planning import LATTICE_SHIP_VERTICES, ship_footprint
    G, M, _ = gold
    assert M["vertices"] == LATTICE_SHIP_VERTICES
    fp = ship_footprint(M["vertices"], M["scale"], M["padding"])
    assert fp.dtype == np.float64 and np.array_equal(fp, G["footprint"])
    assert fp.shape == (17, 2) and fp[0, 1] == 0.0 and fp[4, 0] == 0.0   # a zero coordinate stays zero
    assert np.array_equal(ship_footprint([[1, -2], [0, 3], [-1, 0]], 2.0), [[2, -4], [0, 6], [-2, 0]])


def test_arc_paths_properties():
    from benchpush_amd.planning import arc_paths
    pose = torch.tensor([[10.0, 20.0, 0.3], [5.5, 7.25, -2.0], [0.0, 0.0, np.pi / 2]], dtype=torch.float64)
    k = torch.tensor([-0.1, 0.0, 1e-12, 0.05], dtype=torch.float64)
    p = arc_paths(pose, k, 12.0, 0.5)
    assert p.shape == (3, 4, 25, 3) and p.dtype == torch.float64 and p.is_contiguous()
    s = torch.arange(25, dtype=torch.float64) * 0.5
    assert torch.equal(p[:, :, 0, :], pose[:, None, :].expand(3, 4, 3))                       # start pose
    assert torch.allclose(p[..., 2], pose[:, 2, None, None] + k[None, :, None] * s, rtol=0, atol=1e-14)   # heading th0 + k * s
    chord = (p[:, :, 1:, :2] - p[:, :, :-1, :2]).norm(dim=-1)                                  # spacing: chord of an arc of length step
    kk = k[None, :, None].abs().clamp_min(1e-9)
    want = torch.where(k[None, :, None].abs() < 1e-9, torch.full_like(chord, 0.5), 2 * torch.sin(kk * 0.25) / kk)
    assert torch.allclose(chord, want, rtol=0, atol=1e-12)
    for j in (1, 2):                                                                           # the straight limit
        assert torch.allclose(p[:, j, :, 0], pose[:, 0, None] + s * torch.cos(pose[:, 2, None]), rtol=0, atol=1e-12)
        assert torch.allclose(p[:, j, :, 1], pose[:, 1, None] + s * torch.sin(pose[:, 2, None]), rtol=0, atol=1e-12)
    assert torch.allclose(p[:, 3], arc_paths(pose, k[3:].repeat(3, 1), 12.0, 0.5)[:, 0], rtol=0, atol=0)   # [E, K] curvature
    ek = torch.tensor([[0.1, -0.1], [0.0, 0.2], [0.3, 0.0]], dtype=torch.float64)
    q = arc_paths(pose, ek, 3.0, 1.0)
    assert q.shape == (3, 2, 4, 3) and torch.allclose(q[..., 2], pose[:, 2, None, None] + ek[:, :, None] * torch.arange(4.0, dtype=torch.float64), atol=1e-14)
    # a quarter turn of radius 10 to the left from heading 0 ends at (10, 10)
    quarter = arc_paths(torch.zeros(1, 3, dtype=torch.float64), torch.tensor([0.1], dtype=torch.float64), 5 * np.pi, 5 * np.pi)
    assert torch.allclose(quarter[0, 0, 1], torch.tensor([10.0, 10.0, np.pi / 2], dtype=torch.float64), atol=1e-12)
    with pytest.raises(ValueError):
        arc_paths(torch.zeros(3, dtype=torch.float64), k, 1.0, 0.5)
    with pytest.raises(ValueError):
        arc_paths(pose, torch.zeros(2, 4, dtype=torch.float64), 1.0, 0.5)


def test_replan_mask_is_the_comparison_of_path_update():
    from benchpush_amd.planning import replan_mask
    new, old = torch.tensor([9.4, 9.5, 9.6, 0.0]), torch.tensor([10.0, 10.0, 10.0, 0.0])
    assert replan_mask(new, old).tolist() == [True, False, False, False]
    assert replan_mask(np.array([4.0]), np.array([5.0]), threshold_cost=0.5).tolist() == [False]


def test_swath_config_layout_matches_the_library():
    from benchpush_amd import _lib
    from benchpush_amd.build import build_hip
    build_hip()
    L = _lib.load()
    assert L.bp_sizeof_swath_config() == C.sizeof(_lib.BpSwathConfig) == 32
    assert [(n, getattr(_lib.BpSwathConfig, n).offset) for n, _ in _lib.BpSwathConfig._fields_] == \
        [("H", 0), ("W", 4), ("K", 8), ("P", 12), ("nv", 16), ("outside", 20), ("map_stride", 24)]
    assert "bp_swath_cost" in _lib.EXPORTS and L.bp_abi_version() == 11


def test_restatement_guards_and_window():
    """The restatement's own edge rules, as the device is held to them: non-finite -> NaN and an empty mask, huge -> nothing / +inf, window clamps."""
    cm = np.ones((12, 70))
    fp = np.array([[2.0, 0.0], [-2.0, 1.5], [-2.0, -1.5]])
    ok = np.array([[30.0, 6.0, 0.3], [31.0, 6.2, 0.3]])
    m, c = swath_ref(cm, ok, fp)
    assert m.sum() == c > 0 and swath_ref(cm, ok, fp, outside="reject")[1] == c
    assert swath_ref(cm, ok, fp, rows=(9, 3))[1] == 0.0 and swath_ref(cm, ok, fp, rows=(-5, 99))[1] == c
    assert swath_ref(cm, ok, fp, length=0)[1] == 0.0 and swath_ref(cm, ok, fp, length=7)[1] == c
    m, c = swath_ref(cm, np.array([[30.0, 6.0, 0.3], [np.nan, 6.2, 0.3]]), fp)
    assert np.isnan(c) and not m.any()
    assert swath_ref(cm, np.array([[30.0, 6.0, 0.3], [np.nan, 6.2, 0.3]]), fp, length=1)[1] > 0
    far = np.array([[1e300, 6.0, 0.3]])
    assert swath_ref(cm, far, fp)[1] == 0.0 and swath_ref(cm, far, fp, outside="reject")[1] == np.inf
    edge = np.array([[1.0, 6.0, 0.0]])    # a vertex at column -1: clipped, or rejected
    assert swath_ref(cm, edge, fp)[1] > 0 and swath_ref(cm, edge, fp, outside="reject")[1] == np.inf
