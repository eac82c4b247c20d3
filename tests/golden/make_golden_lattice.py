"""Writes tests/golden/lattice_golden.{json,npz}: recorded output of the reference's own lattice planner (Primitives, Ship, generate_swath, AStar),
next to which the restatement of tests/lattice_ref.py is run case by case.

Run once, from the repository root, with an interpreter that has numpy, scipy and scikit-image (torch is not needed), after the oracle library is built:

    python tests/golden/make_golden_lattice.py /path/to/reference/checkout

The reference is imported as it is, with three stand-ins: ``numba.jit`` is the identity (and ``numba.boolean = bool``), ``dubins`` is this repository's
benchpush_amd/dubins.py loaded by file path, and any module that is absent (matplotlib, the simulator's dependencies) is mocked.  The ``cmap`` argument
of AStar is a stand-in with ``cost_map``, ``shape`` and ``scale``.  Only data is recorded: the two control sets as ``get_primitives`` returns them, the
path lengths, the unrotated ``generate_swath`` masks, and for each search the rotated swath table that the search used, the reference's node path,
its goal node's g score and whether the restatement reproduces the node path (also with its f-tie rule reversed)."""
import contextlib
import importlib.abc
import importlib.machinery
import importlib.util
import io
import json
import math
import os
import sys
import types
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class _MockModule(types.ModuleType):
    __all__ = []
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return mock.MagicMock(name="%s.%s" % (self.__name__, name))


class _MockFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: whatever no real finder knows becomes a mock."""
    mocked = []

    def __init__(self, only=None):
        self.only = only

    def find_spec(self, name, path=None, target=None):
        top = name.split(".")[0]
        if top in ("benchpush", "lattice_ref", "swath_ref", "oracle") or (self.only is not None and top not in self.only):
            return None
        self.mocked.append(name)
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _MockModule(spec.name)

    def exec_module(self, module):
        pass


# what the reference's modules import on the way to AStar and this job never calls; mocked only where no real module is found
ABSENT_OK = {"yaml", "gym", "gymnasium", "pymunk", "pygame", "shapely", "cv2", "torch", "tqdm", "seaborn", "pandas", "networkx", "stable_baselines3",
             "sb3_contrib", "tensorboard", "PIL", "imageio", "spfa"}


def install_stubs():
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: a[0] if (a and callable(a[0]) and not k) else (lambda f: f)
    nb.boolean = bool
    sys.modules["numba"] = nb
    _load("dubins", os.path.join(ROOT, "benchpush_amd", "dubins.py"))
    broken = []
    for name in ("matplotlib.pyplot", "matplotlib.ticker"):      # present but unusable counts as absent
        try:
            importlib.import_module(name)
        except Exception:
            broken.append(name.split(".")[0])
            for m in [m for m in sys.modules if m.split(".")[0] in ("matplotlib", "dateutil")]:
                del sys.modules[m]
    if broken:
        sys.meta_path.insert(0, _MockFinder(only=set(broken)))
    sys.meta_path.append(_MockFinder(only=ABSENT_OK))


class CMap:
    def __init__(self, cost_map, scale):
        self.cost_map, self.shape, self.scale = cost_map, cost_map.shape, scale


SCALE, H, W = 5, 120, 40
SHIP_VERTICES = [[1., -0.], [0.9, 0.10], [0.5, 0.25], [0.25, 0.25], [0, 0.25], [-0.25, 0.25], [-0.5, 0.25], [-0.75, 0.25], [-1., 0.25],
                 [-1., -0.25], [-0.75, -0.25], [-0.5, -0.25], [-0.25, -0.25], [0, -0.25], [0.25, -0.25], [0.5, -0.25], [0.9, -0.10]]
# (seed, x0, y0, theta0, rows to the goal, weight): the start heading is pi / 2 in most and generic in five
CASES = [(101, 20.0, 20.0, math.pi / 2, 80, 1.0), (102, 14.3, 18.6, math.pi / 2, 75, 1.0), (103, 25.7, 22.2, math.pi / 2, 90, 1.0),
         (104, 19.2, 15.9, math.pi / 2, 70, 1.0), (105, 21.4, 24.1, math.pi / 2, 85, 1.0), (106, 17.8, 19.5, math.pi / 2, 78, 1.0),
         (107, 22.9, 17.3, math.pi / 2, 88, 1.0), (108, 20.6, 21.7, 1.3312, 80, 1.0), (109, 18.4, 20.3, 1.8127, 76, 1.0),
         (110, 21.1, 18.8, 1.4946, 84, 1.0), (111, 19.7, 23.4, 1.7011, 72, 1.0), (112, 20.2, 16.6, 1.6203, 82, 1.0)]


def main(ref_root):
    sys.path.insert(0, ref_root)
    install_stubs()
    import lattice_ref as LR
    from benchpush.baselines.ship_ice_nav.planning_based.utils.a_star_search import AStar
    from benchpush.common.primitives import Primitives
    from benchpush.common.ship import Ship
    from benchpush.common.swath import generate_swath, rotate_swath

    meta = {"H": H, "W": W, "scale": SCALE, "ship_vertices": SHIP_VERTICES, "padding": 0.25, "step_size": 0.1}
    arrays = {}
    sets = {}
    for nh, radius in ((8, 2.0), (16, 1.0)):
        raw = Primitives.get_primitives(nh)
        prim = Primitives(scale=SCALE, turning_radius=radius, num_headings=nh, step_size=0.1, cache=False)
        sets[nh] = prim
        meta["set_%d" % nh] = {"turning_radius": radius, "edges": [[list(e) for e in raw[(0, 0, b)]] for b in range(len(raw))],
                               "lengths": [[prim.path_lengths[((0, 0, b), e)] for e in prim.edge_set_dict[(0, 0, b)]] for b in range(len(raw))],
                               "max_prim": prim.max_prim}
    prim = sets[8]
    ship = Ship(scale=SCALE, vertices=SHIP_VERTICES, padding=0.25, mass=1)
    swath_dict = generate_swath(ship, prim, cache=False, model_inference=False)
    max_val = int(prim.max_prim + ship.max_ship_length // 2)
    S = 2 * max_val + 1
    nb, nem = prim.num_base_h, max(len(v) for v in prim.edge_set_dict.values())
    meta.update(max_val=max_val, S=S, ne_max=nem, footprint=ship.vertices.tolist(), max_ship_length=int(ship.max_ship_length))
    big = [np.asarray([[a, np.sign(b) * (abs(b) + ship.width / 2)] for a, b in half]) for half in (ship.right_half, ship.left_half)]
    meta["halves"] = [h.tolist() for h in big]

    def table(fn):
        out = np.zeros((8 * nem, S, S), bool)
        for h in range(8):
            for k, e in enumerate(prim.edge_set_dict[(0, 0, h % nb)]):
                out[h * nem + k] = fn((e, h))
        return out

    unrot = table(lambda key: swath_dict[key])
    arrays["unrotated_masks"] = LR.pack_masks(unrot)
    samples = lambda b, k: prim.paths[((0, 0, b), prim.edge_set_dict[(0, 0, b)][k])]   # noqa: E731
    counts = [len(prim.edge_set_dict[(0, 0, b)]) for b in range(nb)]
    restated = LR.restated_masks(samples, counts, 8, nem, ship.vertices, big, 0.0, max_val)
    differ = [int(i) for i in range(8 * nem) if not np.array_equal(unrot[i], restated[i])]
    meta["unrotated_masks_differing"] = differ
    meta["unrotated_masks_differing_pixels"] = [int((unrot[i] != restated[i]).sum()) for i in differ]
    assert len(differ) <= 4, "more than 4 of the 72 unrotated masks differ from the restated rasterisation: %s" % differ

    T = LR.Tables(meta["set_8"]["edges"], meta["set_8"]["lengths"], 8, SCALE, 2, max_val, prim.turning_radius)
    u = SCALE / 2
    cases, kept = [], 0
    for n, (seed, x0, y0, th0, ahead, weight) in enumerate(CASES):
        cm = LR.golden_map(seed, H, W)
        goal_y = y0 + ahead
        a_star = AStar(weight=weight, cmap=CMap(cm, SCALE), prim=prim, ship=ship, swath_dict=swath_dict, swath_dict_no_padding=swath_dict,
                       ship_no_padding=ship)
        with contextlib.redirect_stdout(io.StringIO()):
            res = a_star.search(start=(x0, y0, th0), goal_y=goal_y)
        assert res, "the reference found no path in case %d" % n
        node_path = np.asarray(res[1][0]).T                      # [n, 3] = (x, y, world heading)
        g_ref = float(res[3][1])
        theta0 = th0 % (2 * math.pi)
        used = a_star.swath_dict
        full = table(lambda key: (used[key] if key in used else rotate_swath(swath_dict[key], theta0)) == 1)
        for key in used:                                         # the table is what the search used, where it used any
            assert np.array_equal(used[key] == 1, rotate_swath(swath_dict[key], theta0) == 1)
        words = LR.pack_masks(full)
        c0, s0 = math.cos(theta0), math.sin(theta0)
        inodes = []
        for x, y, t in node_path:
            a, b = ((x - x0) * c0 + (y - y0) * s0) / u, (-(x - x0) * s0 + (y - y0) * c0) / u
            hh = ((t - theta0) % (2 * math.pi)) / (2 * math.pi / 8)
            assert abs(a - round(a)) < 1e-6 and abs(b - round(b)) < 1e-6 and abs(hh - round(hh)) < 1e-6
            inodes.append((int(round(a)), int(round(b)), int(round(hh)) % 8))
        runs = [LR.lattice_search(cm, (x0, y0, th0), goal_y, T, words, weight=weight, margin=a_star.margin, reverse_ties=rv) for rv in (False, True)]
        same = [r.status == LR.FOUND and [tuple(v) for v in r.inodes] == inodes for r in runs]
        reason = None
        if not all(same):
            reason = "float heading index" if _float_rule_in(inodes, LR, nb) else "tie"
        case = {"seed": seed, "start": [x0, y0, th0], "goal_y": goal_y, "weight": weight, "margin": int(a_star.margin), "kept": reason is None,
                "dropped_because": reason, "g_ref": g_ref, "expanded_ref": len(res[3][0]), "n_nodes": len(inodes),
                "g_restated": runs[0].g, "expanded_restated": runs[0].expanded}
        cases.append(case)
        kept += reason is None
        arrays["masks_%d" % n] = words
        arrays["node_path_%d" % n] = node_path
        arrays["inodes_%d" % n] = np.asarray(inodes, np.int32)
        print("case %2d: kept %s  ref g %.6f  restated g %.6f  expanded %d / %d  nodes %d" %
              (n, reason is None, g_ref, runs[0].g, case["expanded_ref"], runs[0].expanded, len(inodes)), file=sys.stderr)
    meta["cases"] = cases
    meta["kept"], meta["dropped"] = kept, len(CASES) - kept
    meta["mocked_modules"] = sorted(set(_MockFinder.mocked))
    assert kept >= 10, "fewer than 10 of %d searches kept" % len(CASES)
    np.savez_compressed(os.path.join(HERE, "lattice_golden.npz"), **arrays)
    with open(os.path.join(HERE, "lattice_golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("kept %d of %d; %d unrotated masks differ" % (kept, len(CASES), len(differ)), file=sys.stderr)


def _float_rule_in(inodes, LR, nb):
    """Does the reference's own path pass a (node heading, edge heading) pair on which the float rule and the integer rule differ?"""
    for (_, _, h), (_, _, h2) in zip(inodes[:-1], inodes[1:]):
        for eh in range(8):
            if LR.float_heading(h, eh, nb, 8) == h2 and LR.succ_heading(h, eh, nb, 8) != h2:
                return True
    return False


if __name__ == "__main__":
    main(sys.argv[1])
