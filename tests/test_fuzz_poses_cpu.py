"""What the pose fuzz of the observation and cost-map rasterisers (tests/fuzz_poses.py, tests/test_gpu_fuzz_obs.py) covers, asserted with the oracle alone:
the GPU comparison cannot pass for want of inputs.  Every condition is computed after reset (one settle sub-step) from the oracle's info(), world_polys()
and its own observation, for the default batch of the GPU test; a condition must hold in at least 5 % of the scenes (and in at least 8).

A floe is a *candidate* when it passes k_observe's pre-test (its AABB, grown by the shape radius and a pixel, meets the window): that count decides the
number of passes over OBS_CHUNK candidates and the capacity flag.  Raster rows, pixel centres and crossings are looked at only inside the part of the
window that lies on the map, and only for candidates within the range cull."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_poses as F  # noqa: E402
from benchpush_amd.config import default_cfg, merge_user_cfg, ship_ice_physics_params  # noqa: E402
from oracle import oracle as orc  # noqa: E402

SNAP = 1e-6           # OBS_SNAP_Y / OBS_SNAP_X of csrc/bp_kernels.hpp
MAXCAND, CHUNK = 96, 32
KEYS = ("cols_lt0", "cols_geW", "rows_lt0", "rows_geH", "foot_partial", "ht_lt0", "ht_ge", "vtx_near_row", "vtx_on_row", "cross_on_centre",
        "cand_33_64", "cand_65_96", "neg_centroid_paints")


def _setup():
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1})
    params = F.fuzz_params(ship_ice_physics_params(cfg), 0.02, 4)
    return cfg, params, orc.OracleShipIce(params, cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)


def _signed_centroid(v):
    x, y = v[:, 0], v[:, 1]
    xp, yp = np.roll(x, 1), np.roll(y, 1)
    u = x * yp - xp * y
    a = u.sum() / 2
    return np.array([((x + xp) * u).sum(), ((y + yp) * u).sum()]) / (6 * a)


def scene_coverage(o, cfg, params, obs):
    """The conditions of one scene the oracle `o` has just reset to; `obs` is its observation."""
    P = params
    pix, Wg, Hg = P["m_to_pix"], int(P["map_w"] * P["m_to_pix"]), int(P["map_h"] * P["m_to_pix"])
    LW, LH = int(P["local_w"] * pix), int(P["local_h"] * pix)
    info = o.info()
    x, y, th = info["x"], info["y"], info["theta"]
    gj0, gi0 = int(x * pix) - LW // 2, int((y + P["vshift"]) * pix) - LH // 2
    gj1, gi1 = gj0 + LW - 1, gi0 + LH - 1
    cov = dict.fromkeys(KEYS, False)
    cov.update(cols_lt0=gj0 < 0, cols_geW=gj1 >= Wg, rows_lt0=gi0 < 0, rows_geH=gi1 >= Hg)
    s, c = orc.sincos(th)
    rot = lambda p: (np.array([p[0] * c - p[1] * s + x, p[0] * s + p[1] * c + y]) * pix)   # noqa: E731
    g = np.array([rot(p) for p in cfg.ship.vertices])
    out = (g[:, 0] < 0) | (g[:, 0] >= Wg) | (g[:, 1] < 0) | (g[:, 1] >= Hg)
    cov["foot_partial"] = 0 < out.sum() < len(out)
    ht = [int(v) for p in (cfg.ship.head, cfg.ship.tail) for v in rot(p)]      # truncated like the cast to uint16, before it wraps
    cov["ht_lt0"] = min(ht) < 0
    cov["ht_ge"] = ht[0] >= Wg or ht[2] >= Wg or ht[1] >= Hg or ht[3] >= Hg
    wp, cnt = o.world_polys()
    r0, r1, c0, c1 = max(gi0, 0), min(gi1, Hg - 1), max(gj0, 0), min(gj1, Wg - 1)   # the window on the map
    ncand = 0
    for k in range(1, len(cnt)):
        v = wp[k, : cnt[k]]
        lo, hi = v.min(0) - P["poly_radius"], v.max(0) + P["poly_radius"]
        if math.floor(lo[1] * pix) - 1 > gi1 or math.ceil(hi[1] * pix) + 1 < gi0 or math.floor(lo[0] * pix) - 1 > gj1 or math.ceil(hi[0] * pix) + 1 < gj0:
            continue
        ncand += 1
        cen = _signed_centroid(v)
        if abs(x - abs(cen[0])) > P["obs_range"] or abs(y - abs(cen[1])) > P["obs_range"]:
            continue
        col, row = v[:, 0] * pix, v[:, 1] * pix
        near = np.abs(row - np.rint(row)) < SNAP
        inwin = (np.rint(row) >= r0) & (np.rint(row) <= r1) & (col.max() >= c0) & (col.min() <= c1)
        cov["vtx_on_row"] |= bool((near & inwin & (row == np.rint(row))).any())
        cov["vtx_near_row"] |= bool((near & inwin & (row != np.rint(row))).any())
        # crossings of the floe's edges with the window's raster rows that hold no vertex within SNAP, the abscissa computed like raster_row_convex's
        R = np.arange(max(r0, math.ceil(row.min())), min(r1, math.floor(row.max())) + 1, dtype=np.float64)
        R = R[(np.abs(row[None, :] - R[:, None]) >= SNAP).all(1)] if len(R) else R
        if len(R):
            y0, y1 = row[None, :] - R[:, None], np.roll(row, 1)[None, :] - R[:, None]
            x0, x1 = np.broadcast_to(col, y0.shape), np.broadcast_to(np.roll(col, 1), y0.shape)
            st = (y0 > 0) != (y1 > 0)
            X = x0[st] - y0[st] * ((x1[st] - x0[st]) / (y1[st] - y0[st]))
            cov["cross_on_centre"] |= bool(((np.abs(X - np.rint(X)) < SNAP) & (np.rint(X) >= c0) & (np.rint(X) <= c1)).any())
        if cen.min() < 0 and not cov["neg_centroid_paints"]:
            rr, cc = orc.draw_polygon(row, col, shape=(Hg, Wg))
            m = (rr >= r0) & (rr <= r1) & (cc >= c0) & (cc <= c1)
            cov["neg_centroid_paints"] = bool(m.any()) and bool((obs[3, rr[m] - gi0, cc[m] - gj0] == 255).all())
    cov["cand_33_64"], cov["cand_65_96"] = CHUNK < ncand <= 2 * CHUNK, 2 * CHUNK < ncand <= MAXCAND
    return cov, ncand, info


@pytest.fixture(scope="module")
def batch():
    cfg, params, o = _setup()
    scenes = F.make_obs_scenes(F.OBS_SCENES, F.OBS_BASE_SEED)
    rows = []
    for sc in scenes:
        obs, _ = o.reset(sc)
        cov, ncand, info = scene_coverage(o, cfg, params, obs)
        cm = None
        if sc["fuzz"]["family"] == 5:
            cm = [o.costmap(sc_, m, n, al, sm, hz, mg, info["y"] * sc_ - 1, vs) for sc_, m, n, al, sm, hz, mg, vs in F.COSTMAP_CONFIGS]
        wp, cnt = o.world_polys()
        rnd = [np.rint(wp[k, : cnt[k]]) for k in range(1, len(cnt))]          # resample_vertices(decimals=0) at scale 1
        kept = [len(np.unique(q, axis=0)) for q in rnd]
        rows.append(dict(cov=cov, ncand=ncand, cm=cm, dropped=any(k < len(q) for k, q in zip(kept, rnd)), kmin=min(kept, default=99)))
    return scenes, rows


def test_generator_is_deterministic_and_names_its_families():
    a, b = F.make_obs_scenes(24, 5), F.make_obs_scenes(24, 5)
    for p, q in zip(a, b):
        assert p["ship_state"] == q["ship_state"] and p["fuzz"] == q["fuzz"] and len(p["obstacles"]) == len(q["obstacles"])
        assert all(np.array_equal(u["vertices"], w["vertices"]) for u, w in zip(p["obstacles"], q["obstacles"]))
    assert [s["fuzz"]["family"] for s in a] == [(5 + i) % 6 for i in range(24)]
    assert F.make_obs_scenes(3, 7)[1]["ship_state"] == F.make_obs_scenes(3, 8)[0]["ship_state"]     # scene = f(seed)
    for version in (1, 2):
        la, lb = F.make_maze_layouts(9, version), F.make_maze_layouts(9, version)
        assert all(np.array_equal(p[k], q[k]) for p, q in zip(la, lb) for k in ("centres", "walls", "start"))
    o1, o2 = F.make_overflow_scenes(), F.make_overflow_scenes()
    assert [len(s["obstacles"]) for s in o1] == [90, 140] and all(np.array_equal(u["vertices"], w["vertices"]) for u, w in zip(o1[1]["obstacles"], o2[1]["obstacles"]))


def test_scenes_keep_to_the_stated_families(batch):
    scenes, _ = batch
    for sc in scenes:
        fam, (x, y, th) = sc["fuzz"]["family"], sc["ship_state"]
        assert -math.pi <= th <= math.pi and len(sc["obstacles"]) <= 96
        if fam != 4:
            assert len(sc["obstacles"]) <= 60
        if fam == 0:
            assert 0.05 < x < 2.9
        elif fam == 1:
            assert 9.1 < x < 11.95
        elif fam == 2:
            assert 0.05 < y < 0.95 or 35.1 < y < 39.95
        elif fam == 3:
            assert min(abs(x), abs(x - F.MAP_W), abs(y), abs(y - F.MAP_H)) <= 1.0
        else:
            assert 3.5 <= x <= 8.5 and 2.0 <= y <= 30.0
    outside = [s for s in scenes if s["fuzz"]["family"] == 3 and not (0 <= s["ship_state"][0] <= F.MAP_W and 0 <= s["ship_state"][1] <= F.MAP_H)]
    assert len(outside) >= 8          # one family-3 scene in four has its centre outside the map
    exact = [s for s in scenes if s["ship_state"][2] in (0.0, math.pi / 2, -math.pi / 2, math.pi)]
    assert len(exact) >= len(scenes) // 8


@pytest.mark.parametrize("key", KEYS)
def test_default_batch_reaches(batch, key):
    _, rows = batch
    need = max(8, math.ceil(0.05 * len(rows)))
    got = sum(bool(r["cov"][key]) for r in rows)
    assert got >= need, "%s: %d scenes of %d, need %d" % (key, got, len(rows), need)


def test_no_scene_exceeds_the_candidate_capacity(batch):
    scenes, rows = batch
    assert max(r["ncand"] for r in rows) <= MAXCAND
    assert all(r["ncand"] > CHUNK for s, r in zip(scenes, rows) if s["fuzz"]["family"] == 4)


def test_overflow_scenes_have_90_and_about_140_candidates():
    cfg, params, o = _setup()
    n = []
    for sc in F.make_overflow_scenes():
        obs, _ = o.reset(sc)
        n.append(scene_coverage(o, cfg, params, obs)[1])
    assert 80 <= n[0] <= MAXCAND and n[1] >= 120


def test_costmap_configs_cost_cells_and_resampling_drops_vertices(batch):
    scenes, rows = batch
    fam5 = [r for s, r in zip(scenes, rows) if s["fuzz"]["family"] == 5]
    assert len(fam5) >= 8
    for k, c in enumerate(F.COSTMAP_CONFIGS):
        costed = [int(((r["cm"][k] > 0) & (r["cm"][k] < 1e10)).sum()) for r in fam5]
        assert sum(n >= 20 for n in costed) * 2 >= len(fam5), (c, costed)
    assert sum(r["dropped"] for r in rows) * 10 >= len(rows)
    assert sum(r["kmin"] <= 2 for r in rows) >= 8       # floes that resample to one or two vertices (k_costmap's degenerate polygons)


def test_maze_layouts_are_what_they_say():
    for version in (1, 2):
        L = F.make_maze_layouts(F.MAZE_LAYOUTS, version)
        W = L[0]["walls"][:, [0, 2]].max()
        H = L[0]["walls"][:, [1, 3]].max()
        assert len(L) == F.MAZE_LAYOUTS
        st = np.array([l["start"] for l in L])
        assert (st[:, 0] >= 0.3).all() and (st[:, 0] <= W - 0.3).all() and (st[:, 1] >= 0.3).all() and (st[:, 1] <= H - 0.3).all()
        assert st[:, 0].min() < 1.0 and st[:, 0].max() > W - 1.0 and st[:, 1].min() < 1.0 and st[:, 1].max() > H - 1.0     # robots next to the border
        quarter = np.isin(st[:, 2], (0.0, math.pi / 2, math.pi, -math.pi / 2))
        assert quarter.sum() == (F.MAZE_LAYOUTS + 2) // 3
        for l in L:
            c = l["centres"]
            assert c.shape == (F.MAZE_BOXES, 2) and np.array_equal(c[F.MAZE_BOXES // 2:] * 16, np.rint(c[F.MAZE_BOXES // 2:] * 16))
