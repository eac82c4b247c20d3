"""Golden swath masks and costs from the reference's own compute_swath_cost (common/swath.py:114-163) and Ship (common/ship.py) on random arcs
(run ONLY in the build container, after `make -C oracle`):

    PYTHONPATH=<reference checkout>:.:tests PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_swath.py

skimage is absent: skimage.draw's polygon is this repository's restatement (oracle hook) and skimage.transform, which compute_swath_cost does not use,
is mocked.  The reference takes sin / cos from libm and the rotation from a BLAS product, so a pixel centre within ~1e-15 of an edge could fall on
the other side than in the restatement (tests/swath_ref.py): the poses are generic, and a case whose mask differs from the restatement's is dropped
(none is, with these seeds).  Exact ties are tested against the restatement only.  The cost map is not stored: golden_cost_map(seed) rebuilds it.
Data only.
"""
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

from oracle import oracle as orc
from swath_ref import arc, golden_cost_map, swath_ref

draw_mod = types.ModuleType("skimage.draw.draw")
draw_mod.polygon = lambda r, c, shape=None: orc.draw_polygon(np.asarray(r, np.float64), np.asarray(c, np.float64), shape)
draw_pkg = types.ModuleType("skimage.draw"); draw_pkg.draw = draw_mod; draw_pkg.polygon = draw_mod.polygon
sk = types.ModuleType("skimage"); sk.draw = draw_pkg; sk.transform = MagicMock()
sys.modules.update({"skimage": sk, "skimage.draw": draw_pkg, "skimage.draw.draw": draw_mod, "skimage.transform": sk.transform})
for m in ["shapely", "shapely.geometry", "pymunk"]:
    sys.modules[m] = MagicMock()

from benchpush.common.ship import Ship  # noqa: E402
from benchpush.common.swath import compute_swath_cost  # noqa: E402

from benchpush_amd.planning import LATTICE_SHIP_VERTICES  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, P, STEP, SCALE, PADDING, MAP_SEED = 380, 60, 32, 0.75, 5, 0.25, 5


if __name__ == "__main__":
    ship = Ship(scale=SCALE, vertices=LATTICE_SHIP_VERTICES, padding=PADDING)
    cm = golden_cost_map(MAP_SEED, H, W)
    rng = np.random.RandomState(11)
    paths, costs, arrays, dropped = [], [], {}, 0
    for i in range(28):
        side = i % 6   # 0 .. 3: starts near the left / right / bottom / top side, so part of the swath is off the map; 4, 5: inside
        x0, y0 = rng.uniform(8, W - 8), rng.uniform(10, H - 10)
        if side == 0: x0 = rng.uniform(-6, 5)
        if side == 1: x0 = rng.uniform(W - 6, W + 5)
        if side == 2: y0 = rng.uniform(-6, 5)
        if side == 3: y0 = rng.uniform(H - 6, H + 5)
        path = arc(x0, y0, rng.uniform(0, 2 * np.pi), rng.uniform(-0.12, 0.12), (P - 1) * STEP, STEP)
        swath, cost = compute_swath_cost(cm, path, ship.vertices)
        mine, _ = swath_ref(cm, path, ship.vertices)
        if not np.array_equal(mine, swath):
            dropped += 1
            continue
        if len(paths) == 24:
            break
        arrays["mask_%d" % len(paths)] = np.packbits(swath)
        paths.append(path); costs.append(float(cost))
    assert len(paths) == 24, (len(paths), dropped)
    sides = np.array([[p[:, 0].min() < 0, p[:, 0].max() > W - 1, p[:, 1].min() < 0, p[:, 1].max() > H - 1] for p in paths])
    assert sides.any(0).all(), "the cases must leave the map on all four sides"
    arrays.update(paths=np.asarray(paths), costs=np.asarray(costs), footprint=np.asarray(ship.vertices, np.float64))
    np.savez_compressed(os.path.join(HERE, "swath_golden.npz"), **arrays)
    with open(os.path.join(HERE, "swath_golden.json"), "w") as f:
        json.dump({"H": H, "W": W, "P": P, "step": STEP, "scale": SCALE, "padding": PADDING, "map_seed": MAP_SEED, "vertices": LATTICE_SHIP_VERTICES,
                   "cases": len(paths), "dropped": dropped}, f)
    print("wrote", len(paths), "cases; dropped", dropped, "; costs", min(costs), max(costs))
