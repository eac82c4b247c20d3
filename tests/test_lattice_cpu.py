"""The lattice search without a GPU: the Dubins paths, bp_acos in Python, the restatement (tests/lattice_ref.py) against the reference-generated
goldens, the integer heading rule, and the C ABI's layout and export list."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import lattice_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_dubins():
    """By file path, as an interpreter without torch would: the module imports neither torch nor the package."""
    spec = importlib.util.spec_from_file_location("bp_dubins_standalone", os.path.join(ROOT, "benchpush_amd", "dubins.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


dubins = _load_dubins()


@pytest.fixture(scope="module")
def golden():
    return LR.load_golden()


def _end(p):
    return p.sample(p.path_length())


def test_dubins_reaches_the_end_pose_and_respects_the_turning_radius():
    rng = np.random.RandomState(0)
    for _ in range(200):
        q0 = (rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(0, 2 * math.pi))
        q1 = (rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(0, 2 * math.pi))
        r, step = rng.uniform(0.3, 3.0), 0.05
        p = dubins.shortest_path(q0, q1, r)
        x, y, t = _end(p)
        assert abs(x - q1[0]) < 1e-9 and abs(y - q1[1]) < 1e-9
        assert abs((t - q1[2] + math.pi) % (2 * math.pi) - math.pi) < 1e-9
        assert p.path_length() >= math.hypot(q1[0] - q0[0], q1[1] - q0[1]) - 1e-12
        qs, ts = p.sample_many(step)
        assert ts[0] == 0.0 and ts[-1] < p.path_length() <= ts[-1] + step and len(qs) == len(ts)
        th = np.array([q[2] for q in qs])
        turn = np.abs((np.diff(th) + math.pi) % (2 * math.pi) - math.pi)
        assert turn.max(initial=0.0) <= step / r + 1e-9
        for word in range(6):                                    # the shortest path is the shortest of the words that exist
            try:
                assert dubins.path(q0, q1, r, word).path_length() >= p.path_length()
            except ValueError:
                pass


def test_dubins_closed_forms():
    p = dubins.shortest_path((0, 0, 0), (4, 0, 0), 1.0)          # straight line
    assert abs(p.path_length() - 4.0) < 1e-12 and all(abs(q[1]) < 1e-12 and abs(q[2]) < 1e-12 for q in p.sample_many(0.5)[0])
    # quarter circle to the left; the radius is taken 1e-10 short, as the reference's primitives do (eps of get_points_on_dubins_path), because the
    # exactly degenerate case rounds an angle of 0 to 2 pi in the published construction
    p = dubins.shortest_path((0, 0, 0), (2, 2, math.pi / 2), 2.0 - 1e-10)
    assert abs(p.path_length() - math.pi) < 1e-8
    for (x, y, t), s in zip(*p.sample_many(0.25)):
        assert abs(x - 2 * math.sin(s / 2)) < 1e-8 and abs(y - 2 * (1 - math.cos(s / 2))) < 1e-8 and abs(t - s / 2) < 1e-8
    # the symmetric S-curve: a left arc of angle a, a straight of length s, a right arc of angle a; the heading returns to 0
    r, a, st = 1.5, 0.7, 2.0
    p = dubins.shortest_path((0, 0, 0), (2 * r * math.sin(a) + st * math.cos(a), 2 * r * (1 - math.cos(a)) + st * math.sin(a), 0), r)
    assert abs(p.path_length() - (2 * r * a + st)) < 1e-9 and dubins.WORDS[p.path_type()] == "LSR"
    assert all(abs(p.segment_length(i) - v) < 1e-9 for i, v in enumerate((r * a, st, r * a)))
    assert len(dubins.shortest_path((0, 0, 0), (1, 0, 0), 1.0).sample_many(0.25)[0]) == 4       # 0, .25, .5, .75: the end point is not included


def test_recorded_control_sets_have_finite_primitives_without_a_loop(golden):
    from benchpush_amd.planning import LatticePrimitives
    M = golden[1]
    total = 0
    for nh, count in ((8, 18), (16, 109)):
        s = M["set_%d" % nh]
        p = LatticePrimitives(s["edges"], nh, M["scale"], s["turning_radius"], M["step_size"])
        assert sum(len(es) for es in p.edges) == count and p.max_prim == s["max_prim"] and p.den == (2 if nh == 8 else 1)
        for b in range(p.num_base_h):
            for k, (ex, ey, eh) in enumerate(p.edges[b]):
                ln, sm = p.length(b, k), p.samples(b, k)
                assert math.isfinite(ln) and ln == s["lengths"][b][k]                # the maker ran the same module under the reference's Primitives
                assert ln < 2 * math.pi * p.turning_radius                           # no full loop
                th = np.unwrap(sm[2])
                assert abs(th[-1] - th[0]) < 2 * math.pi and abs(sm.shape[1] - ln / p.step_size) <= 1
                assert ln >= math.hypot(ex, ey) * p.scale - 1e-9
                total += 1
    assert total == 127
    q = LatticePrimitives.from_reference(p)
    assert q.edges == p.edges and q.max_prim == p.max_prim and all(np.array_equal(q.samples(b, k), p.samples(b, k)) and q.length(b, k) == p.length(b, k)
                                                                 for b in range(p.num_base_h) for k in range(len(p.edges[b])))


def _ulps(a, b):
    ia, ib = (np.array([v], np.float64).view(np.int64)[0] for v in (a, b))
    return abs(int(ia) - int(ib))


def test_bp_acos_within_two_ulp_of_libm():
    xs = list(np.linspace(-1.0, 1.0, 4001)) + [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 5e-324, -5e-324, 2.2e-308, 1e-300, 1e-17, -1e-17, 2.0 ** -57, 1 - 2.0 ** -53,
                                                  -1 + 2.0 ** -53, 0.4999999999999999, 0.5000000000000001]
    xs += list(1.0 - np.logspace(-16, -1, 200)) + list(-1.0 + np.logspace(-16, -1, 200))
    worst = max(_ulps(LR.bp_acos(float(x)), math.acos(float(x))) for x in xs)
    assert worst <= 2, worst
    assert LR.bp_acos(1.0) == 0.0 and LR.bp_acos(-1.0) == math.pi and math.isnan(LR.bp_acos(1.0000000000000002)) and math.isnan(LR.bp_acos(math.nan))


def test_restatement_reproduces_the_kept_golden_searches(golden):
    G, M = golden
    assert M["kept"] >= 10 and M["kept"] + M["dropped"] == len(M["cases"]) >= 12 and len(M["unrotated_masks_differing"]) <= 4
    s = M["set_8"]
    T = LR.Tables(s["edges"], s["lengths"], 8, M["scale"], 2, M["max_val"], s["turning_radius"] * M["scale"])
    generic = 0
    for n, c in enumerate(M["cases"]):
        if not c["kept"]:
            continue
        generic += c["start"][2] != math.pi / 2
        r = LR.lattice_search(LR.golden_map(c["seed"], M["H"], M["W"]), c["start"], c["goal_y"], T, G["masks_%d" % n], weight=c["weight"], margin=c["margin"])
        assert r.status == LR.FOUND and [tuple(v) for v in r.inodes] == [tuple(v) for v in G["inodes_%d" % n].tolist()], n
        assert r.g == c["g_restated"] and r.expanded == c["expanded_restated"]
        assert abs(r.g - c["g_ref"]) <= LR.golden_rtol(M["S"] * M["S"] * r.n_nodes) * c["g_ref"], (n, r.g, c["g_ref"])
        assert np.abs(r.nodes[:, :2] - G["node_path_%d" % n][:, :2]).max() < 1e-6
        assert 70 <= c["goal_y"] - c["start"][1] <= 90
    assert generic >= 4


def test_restated_rasterisation_reproduces_the_recorded_masks(golden):
    from benchpush_amd.planning import LatticePrimitives, lattice_max_val, ship_footprint, ship_halves
    G, M = golden
    s = M["set_8"]
    p = LatticePrimitives(s["edges"], 8, M["scale"], s["turning_radius"], M["step_size"])
    fp = ship_footprint(M["ship_vertices"], M["scale"], M["padding"])
    assert np.array_equal(fp, np.array(M["footprint"])) and lattice_max_val(p, fp) == M["max_val"]
    for mine, theirs in zip(ship_halves(fp), M["halves"]):
        assert sorted(map(tuple, mine.tolist())) == sorted(map(tuple, theirs))
    masks = LR.restated_masks(p.samples, [len(es) for es in p.edges], 8, p.ne_max, fp, ship_halves(fp), 0.0, M["max_val"])
    recorded = LR.unpack_masks(G["unrotated_masks"], M["S"])
    differ = [i for i in range(len(masks)) if not np.array_equal(masks[i], recorded[i])]
    assert differ == M["unrotated_masks_differing"] and recorded.any(axis=(1, 2)).sum() == 72
    assert np.array_equal(LR.pack_masks(recorded), G["unrotated_masks"])


def test_integer_heading_rule_differs_from_the_float_rule_where_listed():
    diff8 = {(h, eh) for h in range(8) for eh in range(8) if LR.float_heading(h, eh, 2, 8) != LR.succ_heading(h, eh, 2, 8)}
    assert diff8 == {(4, 7), (5, 6), (5, 7), (6, 5), (7, 4), (7, 5)}
    assert all(LR.float_heading(h, eh, 2, 8) == (LR.succ_heading(h, eh, 2, 8) - 1) % 8 for h, eh in diff8)
    diff16 = [(h, eh) for h in range(16) for eh in range(16) if LR.float_heading(h, eh, 4, 16) != LR.succ_heading(h, eh, 4, 16)]
    assert len(diff16) == 78


def test_config_layout_and_exports():
    from benchpush_amd import _lib
    c = _lib.BpLatticeConfig
    assert C.sizeof(c) == 96 and c.map_stride.offset == 56 and c.mask_stride.offset == 64 and c.unit.offset == 72 and c.turning_radius.offset == 88
    assert [f[0] for f in c._fields_[:9]] == ["H", "W", "S", "nh", "nb", "ne_max", "den", "margin", "h_baseline"]
    for name in ("bp_sizeof_lattice_config", "bp_lattice_workspace_bytes", "bp_lattice_search"):
        assert name in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "benchpush_amd.h")) as f:
        header = f.read()
    assert "#define BP_ABI_VERSION 11" in header and "bp_lattice_search(" in header and "bp_lattice_workspace_bytes(" in header
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.load()
        assert L.bp_abi_version() == 11 and L.bp_sizeof_lattice_config() == 96
        cfg = c(H=380, W=60, S=49, nh=8, nb=2, ne_max=9, den=2, margin=25, max_expansions=10, node_capacity=1000, queue_capacity=500, max_path_nodes=8,
                unit=5.0, weight=1.0, turning_radius=10.0)
        per_env = 2048 * 4 + 1000 * 24 + 500 * 16
        assert L.bp_lattice_workspace_bytes(C.byref(cfg), 1) == per_env and L.bp_lattice_workspace_bytes(C.byref(cfg), 4096) == 4096 * per_env
        cfg.node_capacity = 0
        assert L.bp_lattice_workspace_bytes(C.byref(cfg), 1) < 0
