"""Scalar restatement of the path-tracking semantics (DESIGN.md "Path tracking"; include/benchpush_amd.h: bp_track_path) in Python floats, built on the
oracle's deterministic sin / cos and atan2.  Helper of test_track_cpu.py and test_gpu_track.py; tests/golden/make_golden_track.py checks it call by call
against the reference's own ``PlanningBasedPolicy.act`` (there with libm's functions: ``track_ref(..., fns=LIBM)``)."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE, GENTLE, PID, NEAR = 0, 1, 2, 3

# the tunables of policy.py:63-81 and dt (policy.py:82), the reference's values
DEFAULTS = dict(thresh=10.0, look_car=50.0, d_back=15.0, d_ahead=25.0, kp=0.10, ki=0.15, kd=2.0, i_cap=10.0, dead=0.02, straight_ang=0.100, yaw_big=0.50,
                omega_small=0.002, kp_v=0.50, ki_v=0.05, v_max=2.5, omega_max=0.02, dt=0.005)


def _oracle_fns():
    from oracle import oracle as orc
    from oracle import oracle_bd
    return orc.sincos, oracle_bd.atan2


LIBM = (lambda x: (math.sin(x), math.cos(x)), math.atan2)


def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _walk(px, py, start, step, limit, n):
    """dist, j = 0.0, start; while dist < limit and a next sample exists: dist += |p[next] - p[j]|; j = next."""
    dist, j = 0.0, start
    while dist < limit and (j + 1 < n if step > 0 else j > 0):
        hi = j + 1 if step > 0 else j
        ddx, ddy = px[hi] - px[hi - 1], py[hi] - py[hi - 1]
        dist += math.sqrt(ddx * ddx + ddy * ddy)
        j += step
    return j


def track_ref(path, pose, state, action_scale, length=None, cfg=None, fns=None):
    """One call for one env.  path [P, 3], pose (x, y, yaw), state (int_yaw, prev_yaw, int_v, has_yaw).  Returns None where nothing is written (length
    below 1), else (actions (yaw, surge), ct_err, diag (i_near, branch, forward index, backward index), new state)."""
    c = dict(DEFAULTS, **(cfg or {}))
    sincos, atan2 = fns or _oracle_fns()
    path = np.asarray(path, np.float64).reshape(-1, 3)
    n = len(path) if length is None else min(int(length), len(path))
    if n < 1:
        return None
    sx, sy, syaw = (float(v) for v in pose)
    state = tuple(float(v) for v in state)
    if not (np.isfinite(path[:n]).all() and math.isfinite(sx) and math.isfinite(sy) and math.isfinite(syaw)):
        return (math.nan, math.nan), math.nan, (-1, NONE, -1, -1), state
    px, py = path[:n, 0].tolist(), path[:n, 1].tolist()
    int_yaw, prev_yaw, int_v, has_yaw = state
    best, i_near = None, 0
    for i in range(n):
        dx, dy = px[i] - sx, py[i] - sy
        d2 = dx * dx + dy * dy
        if best is None or d2 < best:
            best, i_near = d2, i
    ct = math.sqrt(best)
    dt = c["dt"]
    k = _walk(px, py, i_near, -1, c["d_back"], n)
    j2 = _walk(px, py, i_near, +1, c["d_ahead"], n)
    if ct > c["thresh"]:
        jt = _walk(px, py, i_near, +1, c["look_car"], n)
        yaw_ref = atan2(py[jt] - sy, px[jt] - sx)
        s, co = sincos(yaw_ref - syaw)
        yaw_err = atan2(s, co)
        vbx, vby = px[i_near] - px[k], py[i_near] - py[k]
        vfx, vfy = px[j2] - px[i_near], py[j2] - py[i_near]
        ang_seg = abs(atan2(vbx * vfy - vby * vfx, vbx * vfx + vby * vfy))
        if ang_seg < c["straight_ang"] and abs(yaw_err) > c["yaw_big"]:
            branch = GENTLE
            omega = (1.0 if yaw_err > 0.0 else (-1.0 if yaw_err < 0.0 else 0.0)) * c["omega_small"]
        else:
            branch = PID
            if has_yaw == 0.0:
                int_yaw, prev_yaw, has_yaw = 0.0, yaw_err, 1.0
            if abs(yaw_err) > c["dead"]:
                int_yaw = _clip(int_yaw + yaw_err * dt, -c["i_cap"], c["i_cap"])
            else:
                int_yaw = int_yaw * 0.8
            d_yaw = (yaw_err - prev_yaw) / dt
            prev_yaw = yaw_err
            omega = _clip(c["kp"] * yaw_err + c["ki"] * int_yaw + c["kd"] * d_yaw, -c["omega_max"], c["omega_max"])
    else:
        branch, jt = NEAR, j2
        yaw_ref = atan2(py[j2] - py[k], px[j2] - px[k])
        s, co = sincos(yaw_ref - syaw)
        yaw_err = atan2(s, co)
        omega = _clip(yaw_err / dt, -c["omega_max"], c["omega_max"])
    int_v = _clip(int_v + c["ki_v"] * ct * dt, 0.0, c["v_max"])
    pv = c["kp_v"] * ct + int_v
    v_cmd = pv if pv < c["v_max"] else c["v_max"]
    return (omega / action_scale, 20.0 * v_cmd), ct, (i_near, branch, jt, k), (int_yaw, prev_yaw, int_v, has_yaw)


def track_ref_batch(paths, poses, state, action_scale, lengths=None, active=None, cfg=None, out=None):
    """The restatement over a batch.  paths [E, P, 3] or one shared [P, 3]; state [E, 4] is updated in place.  out = (actions [E, 2], ct_err [E],
    diag [E, 4]) is overwritten where the device would write and returned (fresh zero arrays if None)."""
    paths, poses = np.asarray(paths, np.float64), np.asarray(poses, np.float64)
    E = len(poses)
    actions, ct, diag = out if out is not None else (np.zeros((E, 2)), np.zeros(E), np.zeros((E, 4), np.int32))
    for e in range(E):
        if active is not None and not active[e]:
            continue
        r = track_ref(paths[e] if paths.ndim == 3 else paths, poses[e], state[e], action_scale, None if lengths is None else lengths[e], cfg)
        if r is None:
            continue
        actions[e], ct[e], diag[e], state[e] = r
    return actions, ct, diag


def load_golden():
    with open(os.path.join(GOLDEN, "track_golden.json")) as f:
        return json.load(f)


def golden_straight(G, pose, goal_y, dy=10):
    """The path [n, 3] that the reference's straight_planner gave for (pose, goal_y, dy), as recorded in the golden."""
    for s in G["straight"]:
        if tuple(s["pose"]) == tuple(pose) and s["goal_y"] == goal_y and s["dy"] == dy:
            return np.asarray(s["path"], np.float64).reshape(-1, 3)
    raise KeyError((pose, goal_y, dy))
