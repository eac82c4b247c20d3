"""rgb_array frames without a GPU: palettes and frame sizes against the reference's values, the per-slot tables, the painter's primitives,
the RGB PNG codec and the new C ABI names (tests/test_gpu_render.py compares k_render's frames with the painter)."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest

from benchpush_amd import render as R
from benchpush_amd.config import default_cfg


def _cfg(name):
    c = default_cfg(name)
    if name == "maze_namo":
        c.env = c.env1          # maze_version 1 (maze_NAMO_env.py:68-73)
    return c


def test_palettes_are_the_references():
    assert R.PALETTES["ship_ice"]["background"] == (28, 107, 160)       # ship_ice_env.py:487
    assert R.PALETTES["ship_ice"]["ice"] == (173, 216, 230)             # ship_ice_env.py:210
    assert R.PALETTES["ship_ice"]["ship"] == (64, 64, 64)               # ship_ice_env.py:214
    assert R.PALETTES["maze"]["background"] == (200, 200, 200)          # maze_NAMO_env.py:602
    assert R.PALETTES["maze"]["box"] == (204, 153, 102)                 # maze_NAMO_env.py:256
    assert R.PALETTES["maze"]["robot"] == (100, 100, 100)               # maze_NAMO_env.py:260
    assert R.PALETTES["maze"]["wheel"] == (0, 0, 0)                     # sim_utils.py:50
    assert R.PALETTES["box_delivery"]["background"] == (234, 234, 234)  # box_delivery_env.py:235
    assert R.PALETTES["box_delivery"]["boundary"] == (140, 155, 155)    # sim_utils.py:14 BOUNDARY
    assert R.PALETTES["box_delivery"]["receptacle"] == (144, 238, 144)  # sim_utils.py:11 GREEN
    assert R.PALETTES["box_delivery"]["box"] == (204, 153, 102)         # sim_utils.py:12 BOX
    assert R.PALETTES["box_delivery"]["robot"] == (100, 100, 100)       # sim_utils.py:13 AGENT
    assert R.PALETTES["area_clearing"]["background"] == (245, 245, 245) # area_clearing.py:353-357
    assert R.PALETTES["area_clearing"]["box"] == (204, 153, 102)        # area_clearing.py:393
    assert R.PALETTES["area_clearing"]["robot"] == (100, 100, 100)      # area_clearing.py:376
    assert R.PATH_RGB == (255, 0, 0)                                    # renderer.py:83-92


def test_frame_sizes():
    c = _cfg("ship_ice")
    assert R.frame_size("ship_ice", c) == (1600, 480)                   # map 12 x 40 m at render_scale 40 (config.yaml:63)
    assert R.frame_size("ship_ice", c, 10) == (400, 120)
    assert R.frame_size("maze", _cfg("maze_namo")) == (15 * 80, 15 * 80)  # env1 15 x 15 m at render_scale 80
    bd = _cfg("box_delivery")                                           # (room_length + wall_thickness / 2) x (room_width + wall_thickness / 2), s = 30
    assert R.frame_size("box_delivery", bd) == (int((5 + 7) * 30), int((10 + 7) * 30))
    assert R.frame_size("area_clearing", _cfg("area_clearing")) == (540, 540)   # (16 + 2) m at render_scale 30
    assert R.transform("area_clearing", _cfg("area_clearing")) == (9.0, 9.0, 0.0, 540.0)   # both axes shifted by env_width / 2
    assert R.transform("box_delivery", bd) == (0.0, 0.0, 255.0, 180.0)
    with pytest.raises(ValueError):
        R.frame_size("ship_ice", c, 0)


def _fake_env(task, nbcap, **kw):
    e = types.SimpleNamespace(nb_cap=nbcap, trials=[None, None], **kw)
    return e


def test_slot_tables():
    t = R.render_table("ship_ice", _fake_env("ship_ice", 16))
    assert t["labels"][0] == "ship" and t["rank"][0, 0] == t["rank"].max() and t["order"][0, -1] == 0
    assert tuple(t["rgb"][1, 0]) == (64, 64, 64) and tuple(t["rgb"][1, 5]) == (173, 216, 230)
    mc = _cfg("maze_namo")
    t = R.render_table("maze", _fake_env("maze", 16, cfg=mc, layouts=[{"centres": [0] * 4}]))
    nw = len(mc.robot.wheel_vertices)
    assert t["labels"][: 1 + nw] == ["robot"] + ["wheel"] * nw
    assert all(tuple(t["rgb"][0, 1 + k]) == (0, 0, 0) for k in range(nw))
    assert t["rank"][0, : 1 + nw].min() > t["rank"][0, 1 + nw:].max()          # the agent's shapes are on top
    assert t["labels"][-1] == "wall" and t["rank"][0, -1] < t["rank"][0, 1 + nw]  # walls under the boxes
    from benchpush_amd.box_delivery_scenario import generate_trials
    bc = _cfg("box_delivery")
    trials = generate_trials(bc, 2)
    env = _fake_env("box_delivery", 32, cfg=bc, nbox=len(trials[0]["boxes"]))
    env.trials = trials
    t = R.render_table("box_delivery", env)
    assert t["rank"][0, 0] == t["rank"][0, :6].min() and t["rank"][0, :6].min() > t["rank"][0, 6:].max()
    pr = R.overlay_prims("box_delivery", env)
    assert len(pr) == 1 and pr[0]["kind"] == "poly" and pr[0]["layer"] == 0 and pr[0]["rgb"] == (144, 238, 144)   # receptacle: static layer, green
    ac = _cfg("area_clearing")
    pr = R.overlay_prims("area_clearing", _fake_env("area_clearing", 32, cfg=ac))
    assert all(p["kind"] == "capsule" and p["half_px"] == 1.5 and p["layer"] == 1 for p in pr)


def test_painter_polygon_equals_oracle_fill():
    from oracle.oracle import draw_polygon
    from render_painter import polygon_mask
    rng = np.random.default_rng(0)
    H, W = 90, 130
    for _ in range(60):
        n = int(rng.integers(3, 12))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = rng.uniform(2, 30)
        r0, c0 = rng.uniform(-10, H + 10), rng.uniform(-10, W + 10)
        rows, cols = r0 + rad * np.sin(ang), c0 + rad * np.cos(ang)
        if rng.random() < 0.3:
            rows, cols = np.round(rows), np.round(cols)        # vertices on pixel centres: the vertex / edge rules
        full = np.zeros((H, W), bool)
        rr, cc = draw_polygon(rows, cols, (H, W))
        full[rr, cc] = True
        assert np.array_equal(polygon_mask(rows, cols, H, W), full)


def test_painter_capsule_rule():
    from render_painter import capsule_mask
    # goal line of ship-ice: row H - goal_y * s, half-width 3, across the frame
    m = capsule_mask((0.0, 1240.0), (480.0, 1240.0), 3.0, 1600, 480)           # integral row: 1237..1243 (dist2 = 9 <= 9 at the ends)
    assert np.array_equal(np.nonzero(m.any(1))[0], np.arange(1237, 1244)) and m[1237:1244].all()
    m = capsule_mask((0.0, 1239.5), (480.0, 1239.5), 3.0, 1600, 480)           # fractional row: 1237..1242 (|dy| <= 2.5)
    assert np.array_equal(np.nonzero(m.any(1))[0], np.arange(1237, 1243))
    m = capsule_mask((5.0, 5.0), (5.0, 5.0), 2.0, 11, 11)                      # a disc: a == b
    yy, xx = np.mgrid[0:11, 0:11]
    assert np.array_equal(m, (xx - 5.0) ** 2 + (yy - 5.0) ** 2 <= 4.0)
    m = capsule_mask((1.0, 1.0), (8.0, 1.0), 0.5, 4, 12)                       # a 1-px path: one row, clamped at the ends
    assert np.array_equal(np.argwhere(m), [[1, c] for c in range(1, 9)])


def test_tile_images():
    f = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    m = R.tile_images(f)
    assert m.shape == (2 * 2, 3 * 3, 3)
    assert np.array_equal(m[0:2, 3:6], f[1]) and np.array_equal(m[2:4, 3:6], f[4]) and not m[2:4, 6:9].any()


def test_rgb_png_roundtrip_and_grey_unchanged(tmp_path):
    import struct
    import zlib
    from benchpush_amd.obs_log import read_gray_png, read_png, write_gray_png, write_rgb_png
    f = np.random.default_rng(1).integers(0, 256, (17, 23, 3)).astype(np.uint8)
    write_rgb_png(str(tmp_path / "c.png"), f)
    assert np.array_equal(read_png(str(tmp_path / "c.png")), f)
    g = np.random.default_rng(2).integers(0, 256, (9, 14)).astype(np.uint8)
    write_gray_png(str(tmp_path / "g.png"), g)
    raw = np.concatenate([np.zeros((9, 1), np.uint8), g], 1).tobytes()
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    want = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 14, 9, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    assert open(str(tmp_path / "g.png"), "rb").read() == want
    assert np.array_equal(read_gray_png(str(tmp_path / "g.png")), g)


def test_render_abi_declared_and_exported():
    from benchpush_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "benchpush_amd.h")).read()
    for n in ("bp_render", "bp_set_render_table", "bp_sizeof_render_args", "bp_sizeof_render_prim"):
        assert n in _lib.EXPORTS and (n + "(") in hdr
    L = _lib.load()
    for n in _lib.EXPORTS:
        getattr(L, n)
    assert L.bp_abi_version() == 11
    assert L.bp_sizeof_render_args() == C.sizeof(R.RenderArgs) and L.bp_sizeof_render_prim() == C.sizeof(R.RenderPrim)
