"""CPU AddressSanitizer + UndefinedBehaviorSanitizer pass over the host-side product code, which is otherwise compiled only inside the .hip translation
unit: bp_host_scene.hpp (the scene builders that bp_load_scenarios / bp_load_maze / bp_bd_load call before their first HIP call, and pack_trials) over
bp_host_geom.hpp and bp_host_bd.hpp (hulls and mass properties, fillPoly, disk dilation, EDT indices, spfa, maze maps).
tools/host_sanitize/host_sanitize.cpp calls those same builders -- the library's code, not a copy of it -- on the arrays the Python envs hand to the
entry points, for every shipped layout family: 100 ship-ice trials at 10-50 %, both maze versions, the four box-delivery obstacle configurations and the
four area-clearing layouts; and, in its --refuse mode, on the smallest records that reach each of the builders' refusal messages.
GPU sanitizers are not available on the pool; this is the CPU build only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "host_sanitize", "host_sanitize.cpp")


def _b(a, dt):
    return np.ascontiguousarray(a, dt).tobytes()


def _ship_records():
    from benchpush_amd import _lib
    from benchpush_amd.config import default_cfg, merge_user_cfg, ship_ice_physics_params
    from benchpush_amd.envs.ship_ice import default_trials
    from benchpush_amd.scenario import pack_trials
    out = []
    for conc in (0.1, 0.2, 0.3, 0.4, 0.5):
        cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": conc})
        bc = _lib.make_config(ship_ice_physics_params(cfg), cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)
        pk = pack_trials(default_trials(conc, 20, base_seed=int(conc * 100)), max_verts=_lib.MAXV)
        T, F, V = pk["verts"].shape[:3]
        out.append(struct.pack("<i", 1) + bytes(bc) + struct.pack("<iii", T, F, V) + _b(pk["verts"], np.float64) + _b(pk["counts"], np.int32) +
                   _b(pk["centres"], np.float64) + _b(pk["starts"], np.float64) + _b(pk["nfloes"], np.int32))
    return out


def _maze_records():
    from benchpush_amd import _lib
    from benchpush_amd.config import default_cfg, maze_physics_params, maze_walls, merge_user_cfg
    from benchpush_amd.envs.maze_namo import _maze_cfg
    from benchpush_amd.maze_scenario import generate_layout
    out = []
    for version, nbox, rs in ((1, 20, False), (2, 8, True)):
        cfg = _maze_cfg({"maze_version": version, "num_obstacles": nbox, "random_start": rs})
        P = maze_physics_params(cfg)
        rv = cfg.robot.vertices
        head = ((rv[0][0] + rv[3][0]) / 2, (rv[0][1] + rv[3][1]) / 2)
        tail = ((rv[1][0] + rv[2][0]) / 2, (rv[1][1] + rv[2][1]) / 2)
        bc = _lib.make_config(P, rv, head, tail, env_kind=_lib.ENV_MAZE, wheel_vertices=cfg.robot.wheel_vertices, obstacle_size=cfg.obstacle_size)
        walls = np.ascontiguousarray(maze_walls(cfg), np.float64)
        layouts = [generate_layout(cfg, walls, 3 + t) for t in range(6)]
        centres = np.stack([np.asarray(l["centres"], np.float64).reshape(nbox, 2) for l in layouts])
        start = np.stack([np.asarray(l["start"], np.float64).reshape(3) for l in layouts])
        gh, gw = int(round(bc.map_h * bc.m_to_pix)), int(round(bc.map_w * bc.m_to_pix))
        out.append(struct.pack("<i", 2) + bytes(bc) + struct.pack("<iiiii", len(layouts), nbox, len(walls), gh, gw) + _b(centres, np.float64) +
                   _b(walls, np.float64) + _b(start, np.float64))
    return out


def _bd_record(bcfg, trials, nbox, ns):
    def pad(a, fill=0):
        o = np.full((ns,) + a.shape[1:], fill, a.dtype)
        o[: len(a)] = a
        return o
    starts = np.stack([t["start"] for t in trials])
    boxes = np.stack([t["boxes"] for t in trials])
    sv = np.stack([pad(np.asarray(t["statics"][0])) for t in trials])
    sc = np.stack([pad(np.asarray(t["statics"][1])) for t in trials])
    sp = np.stack([pad(np.asarray(t["statics"][2])) for t in trials])
    sr = np.stack([pad(np.asarray(t["statics"][3])) for t in trials])
    st = np.stack([pad(np.asarray(t["statics"][4]), 3) for t in trials])
    return (struct.pack("<i", 3) + bytes(bcfg) + struct.pack("<iii", len(trials), nbox, ns) + _b(starts, np.float64) + _b(boxes, np.float64) +
            _b(sv, np.float64) + _b(sc, np.int32) + _b(sp, np.float64) + _b(sr, np.float64) + _b(st, np.int32))


def _box_records():
    from benchpush_amd import _lib
    from benchpush_amd.box_delivery_scenario import box_delivery_params, box_delivery_physics_params, generate_trials
    from benchpush_amd.envs.box_delivery import _bd_cfg
    out = []
    for oc in ("small_empty", "small_columns", "large_columns", "large_divider"):
        cfg = _bd_cfg({"env": {"obstacle_config": oc}})
        bd = box_delivery_params(cfg)
        trials = generate_trials(cfg, 4, 5)
        nbox = len(trials[0]["boxes"])
        bd["num_boxes"] = nbox
        bcfg = _lib.make_bd_config(box_delivery_physics_params(cfg), bd, cfg)
        out.append(_bd_record(bcfg, trials, nbox, max(len(t["statics"][1]) for t in trials)))
    return out


def _area_records():
    from benchpush_amd import _lib
    from benchpush_amd.area_clearing_scenario import (area_clearing_params, area_clearing_physics_params, env_layout, generate_trials, goal_points)
    from benchpush_amd.envs.area_clearing import _ac_cfg
    out = []
    for name in ("clear_env", "clear_env_small", "walled_env", "walled_env_with_columns"):
        cfg = _ac_cfg({"env": name})
        bd = area_clearing_params(cfg)
        trials = generate_trials(cfg, 3, 2)
        nbox = len(trials[0]["boxes"])
        bd["num_boxes"] = nbox
        lay = env_layout(cfg)
        bcfg = _lib.make_bd_config(area_clearing_physics_params(cfg), bd, cfg)
        _lib.fill_area_geometry(bcfg, lay.boundary, lay.outer_boundary, cfg.agent.footprint_vertices, goal_points(cfg))
        bcfg.distance_scale_max = bd["distance_scale_max"]
        out.append(_bd_record(bcfg, trials, nbox, max(len(t["statics"][1]) for t in trials)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, compiled once for the module."""
    path = str(tmp_path_factory.mktemp("host_sanitize") / "host_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-Wno-unused-function", "-o", path, SRC])
    return path


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_host_side_loaders_are_clean_under_asan_and_ubsan(exe, tmp_path):
    case = tmp_path / "cases.bin"
    recs = _ship_records() + _maze_records() + _box_records() + _area_records()
    case.write_bytes(b"".join(recs))
    rc, out, err = _run(exe, [str(case)])
    assert rc == 0, (out[-2000:], err[-4000:])
    assert "host-sanitize-ok %d" % len(recs) in out and "runtime error" not in err and "AddressSanitizer" not in err, (out[-2000:], err[-4000:])
    assert out.count("ship-ice:") == 5 and out.count("maze:") == 2 and out.count("box-delivery:") == 4 and out.count("area-clearing:") == 4


def _refusal_records():
    """[(record, the builder's message)]: the smallest records that reach each refusal a builder's input can reach -- at most two trials, one box, at
    most three static slots.  Where two trials can be had the bad one is the second, so the builder has accepted a trial when it refuses.  One trial:
    box_half = 0 makes every box degenerate, and an area-clearing trial is only accepted with its four walls (the small-map window must be sealed), more
    statics than these records hold; its refusals need no accepted trial before them."""
    from benchpush_amd import _lib
    from benchpush_amd.area_clearing_scenario import area_clearing_params, area_clearing_physics_params, env_layout, goal_points
    from benchpush_amd.box_delivery_scenario import box_delivery_params, box_delivery_physics_params, generate_trials
    from benchpush_amd.config import default_cfg, merge_user_cfg, ship_ice_physics_params
    from benchpush_amd.envs.area_clearing import _ac_cfg
    from benchpush_amd.envs.box_delivery import _bd_cfg
    out = []
    # ship-ice: trial 0 holds one triangle
    cfg = merge_user_cfg(default_cfg("ship_ice"), {"concentration": 0.1})
    bc = _lib.make_config(ship_ice_physics_params(cfg), cfg.ship.vertices, cfg.ship.head, cfg.ship.tail)

    def ship(V, counts, nfloes, second):
        verts = np.zeros((2, 1, V, 2))
        verts[0, 0, :3] = [[10.0, 10.0], [14.0, 10.0], [10.0, 14.0]]
        verts[1, 0, : len(second)] = second
        centres = np.array([[[11.0, 11.0]], [[20.0, 20.0]]])
        starts = np.array([[6.0, 2.0, np.pi / 2]] * 2)
        return (struct.pack("<i", 1) + bytes(bc) + struct.pack("<iii", 2, 1, V) + _b(verts, np.float64) + _b(counts, np.int32) + _b(centres, np.float64) +
                _b(starts, np.float64) + _b(nfloes, np.int32))
    tri = [[20.0, 20.0], [24.0, 20.0], [20.0, 24.0]]
    ang = 2 * np.pi * np.arange(_lib.MAXV + 1) / (_lib.MAXV + 1)
    out.append((ship(3, [[3], [3]], [1, 2], tri), "nfloes > F"))
    out.append((ship(3, [[3], [4]], [1, 1], tri), "vertex count > V"))
    out.append((ship(_lib.MAXV + 1, [[3], [_lib.MAXV + 1]], [1, 1], np.stack([20 + 5 * np.cos(ang), 20 + 5 * np.sin(ang)], 1)), "hull exceeds BP_MAXV vertices"))

    # box-delivery: a trial of one box whose only static is the receptacle
    cfg = _bd_cfg({"env": {"obstacle_config": "small_empty"}})
    gen = generate_trials(cfg, 2, 5)

    def bd_config(**fields):
        bd = box_delivery_params(cfg)
        bd["num_boxes"] = 1
        bcfg = _lib.make_bd_config(box_delivery_physics_params(cfg), bd, cfg)
        for k, v in fields.items():
            setattr(bcfg, k, v)
        return bcfg

    def statics(rows):   # rows of (vertices, count, pose, radius, type)
        v = np.zeros((len(rows), 4, 2))
        for i, r in enumerate(rows):
            v[i, : len(r[0])] = r[0]
        return (v, np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.float64), np.array([r[3] for r in rows], np.float64),
                np.array([r[4] for r in rows], np.int32))

    def trial(t, rows):
        return {"start": gen[t]["start"], "boxes": gen[t]["boxes"][:1], "statics": statics(rows)}
    k = list(gen[0]["statics"][4]).index(4)
    rv = np.asarray(gen[0]["statics"][0][k], np.float64)
    recept = (rv, 4, gen[0]["statics"][2][k], 0.0, 4)
    column = (rv * 0.1, 4, (0.0, 0.0, 0.3), 0.0, 3)
    good = trial(0, [recept])

    def bd(second, ns, bcfg=None):
        return _bd_record(bcfg or bd_config(), [good, trial(1, second)], 1, ns)
    out.append((_bd_record(bd_config(box_half=0.0), [good], 1, 1), "degenerate box"))
    out.append((bd([recept, (rv, 5, (0.0, 0.0, 0.0), 0.0, 3)], 2), "static polygons have 3 or 4 vertices"))
    collinear = np.array([rv[0], (rv[0] + rv[1]) / 2, rv[1], rv[3]])
    out.append((bd([(collinear, 4, recept[2], 0.0, 4)], 1), "the receptacle must be a quadrilateral"))
    out.append((bd([column], 1), "exactly one receptacle polygon per trial is required"))
    out.append((bd([recept, recept], 2), "exactly one receptacle polygon per trial is required"))

    # area-clearing
    cfg = _ac_cfg({"env": "clear_env"})
    ac = area_clearing_params(cfg)
    ac["num_boxes"] = 1
    lay = env_layout(cfg)
    acfg = _lib.make_bd_config(area_clearing_physics_params(cfg), ac, cfg)
    _lib.fill_area_geometry(acfg, lay.boundary, lay.outer_boundary, cfg.agent.footprint_vertices, goal_points(cfg))
    acfg.distance_scale_max = ac["distance_scale_max"]
    out.append((_bd_record(acfg, [trial(0, [recept])], 1, 1), "area-clearing has no receptacle polygon"))
    out.append((_bd_record(acfg, [trial(0, [column])], 1, 1), "free space does not fit the small-map window"))
    return out


def test_every_refusal_of_the_scene_builders_is_clean_under_asan_and_ubsan(exe, tmp_path):
    recs = _refusal_records()
    case = tmp_path / "refusals.bin"
    case.write_bytes(b"".join(r for r, _ in recs))
    rc, out, err = _run(exe, ["--refuse", str(case)])
    assert rc == 0, (out[-2000:], err[-4000:])
    assert out.splitlines() == ["refused: " + m for _, m in recs] + ["host-sanitize-refused %d" % len(recs)]
    assert "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    # the same records are not accepted by the ordinary mode either: it stops at the first, with the message
    rc, out, err = _run(exe, [str(case)])
    assert rc == 1 and "refused: " + recs[0][1] in err and "Sanitizer" not in err, (out, err[-4000:])
