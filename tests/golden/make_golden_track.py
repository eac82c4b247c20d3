"""Writes tests/golden/track_golden.json: recorded output of the reference's own ``PlanningBasedPolicy.act`` and ``straight_planner``
(baselines/ship_ice_nav/planning_based/policy.py), next to which the restatement of tests/track_ref.py is run call by call.

Run once, from the repository root, with an interpreter that has numpy (torch is not needed):

    python tests/golden/make_golden_track.py /path/to/reference/checkout

The reference is imported as it is, with the stand-ins of make_golden_lattice.py plus mocks for skimage and torchvision (its planners' imports; this
job calls neither planner).  The policy is built with ``__new__`` and its ``path`` is set by hand.  Only data is recorded: per path the samples, the
poses of 25 consecutive calls, what each call returned and the integrators after it.  Every call is also made with the restatement -- with libm's
functions, from the reference's state before the call -- and a call where the nearest index or the branch differs from the reference is marked
``keep: false`` and counted; the largest differences seen over the kept calls are written next to the data."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

import make_golden_lattice as mgl   # noqa: E402
import track_ref as T               # noqa: E402

ACTION_SCALE = (math.pi / 2) / 7
CALLS = 25
LENGTHS = [2, 3, 5, 8, 13, 21, 34, 55, 64, 65, 89, 97, 128, 129, 160, 200, 233, 300, 350, 399, 144]
SPACINGS = [0.02, 0.5, 2.0]
NPATHS = 42


def make_path(rng, n, ds, straight):
    s = np.arange(n) * ds
    amp = rng.uniform(0.0, 0.02) if straight else rng.uniform(0.2, 0.7)
    head = math.pi / 2 + rng.uniform(-0.2, 0.2) + amp * np.sin(s / rng.uniform(8.0, 30.0) + rng.uniform(0, 2 * math.pi))
    x = rng.uniform(20.0, 40.0) + np.concatenate(([0.0], np.cumsum(ds * np.cos(head[:-1]))))
    y = rng.uniform(0.0, 20.0) + np.concatenate(([0.0], np.cumsum(ds * np.sin(head[:-1]))))
    return np.round(np.stack([x, y, head], 1), 5)


def make_pose(rng, path, idx, far, state):
    n = len(path)
    idx = min(max(idx, 0), n - 1)
    x, y, h = path[idx]
    off = (rng.choice([-1.0, 1.0]) * 14.0 + rng.normal(0, 1.0)) if far else rng.normal(0, 2.0)
    along = rng.normal(0, 0.5)
    px = x - off * math.sin(h) + along * math.cos(h)
    py = y + off * math.cos(h) + along * math.sin(h)
    yaw = h + rng.normal(0, 0.2)
    u = rng.uniform()
    if far and u < 0.4:
        yaw += rng.choice([-1.0, 1.0]) * rng.uniform(0.6, 1.5)
    elif far and u < 0.6:      # aimed at the carrot: the PID's dead zone
        r = T.track_ref(path, (px, py, yaw), state, ACTION_SCALE, fns=T.LIBM)
        jt = r[2][2]
        yaw = math.atan2(path[jt, 1] - py, path[jt, 0] - px) + rng.uniform(-0.015, 0.015)
    return [round(float(px), 6), round(float(py), 6), round(float(yaw), 6)]


def ref_state(p):
    has = hasattr(p, "_int_yaw")
    return [float(p._int_yaw) if has else 0.0, float(p._prev_yaw) if has else 0.0, float(getattr(p, "_int_v", 0.0)), 1.0 if has else 0.0]


def main(ref_root):
    mgl.install_stubs()
    sys.meta_path.append(mgl._MockFinder(only={"skimage", "torchvision"}))
    sys.path.insert(0, ref_root)
    from benchpush.baselines.ship_ice_nav.planning_based.policy import PlanningBasedPolicy

    rng = np.random.RandomState(20240611)
    cases, dropped = [], 0
    kept_by_branch = {T.GENTLE: 0, T.PID: 0, T.NEAR: 0}
    max_yaw = max_surge = max_state = 0.0
    for c in range(NPATHS):
        n, ds = LENGTHS[c % len(LENGTHS)], SPACINGS[c % 3]
        path = make_path(rng, n, ds, straight=(c % 3 == 0) or (c % 7 == 0))
        far = c % 2 == 1
        pol = PlanningBasedPolicy.__new__(PlanningBasedPolicy)
        pol.path = path
        i0 = rng.randint(-3, max(1, n // 2))
        stride = max(1, int(round(rng.uniform(0.2, 1.5) / ds))) if n > 30 else 1
        poses, outs, states, keep, diags = [], [], [], [], []
        for t in range(CALLS):
            before = ref_state(pol)
            pose = make_pose(rng, path, i0 + t * stride, far, before)
            yaw, surge = pol.act(None, ship_pos=tuple(pose), action_scale=ACTION_SCALE)
            after = ref_state(pol)
            # what the reference did, from its own expressions and its state
            d2 = (path[:, 0] - pose[0]) ** 2 + (path[:, 1] - pose[1]) ** 2
            ri = int(np.argmin(d2))
            if float(np.sqrt(d2[ri])) <= 10.0:
                rb = T.NEAR
            else:
                rb = T.PID if (after[3] == 1.0 and (before[3] == 0.0 or after[1] != before[1] or after[0] != before[0])) else T.GENTLE
            (myaw, msurge), _, diag, mstate = T.track_ref(path, pose, before, ACTION_SCALE, fns=T.LIBM)
            ok = diag[0] == ri and diag[1] == rb
            if ok:
                kept_by_branch[rb] += 1
                max_yaw = max(max_yaw, abs(myaw - float(yaw)))
                max_surge = max(max_surge, abs(msurge - float(surge)))
                max_state = max(max_state, max(abs(a - b) for a, b in zip(mstate, after)))
            else:
                dropped += 1
            poses.append(pose)
            outs.append([float(yaw), float(surge)])
            states.append(after)
            keep.append(bool(ok))
            diags.append([ri, rb])
        cases.append({"path": path.tolist(), "spacing": ds, "poses": poses, "out": outs, "state_after": states, "keep": keep, "near_branch": diags})
    total = NPATHS * CALLS
    assert dropped <= 0.02 * total, "more than 2 %% of the calls dropped: %d of %d" % (dropped, total)
    assert min(kept_by_branch.values()) >= 30, kept_by_branch

    straight = []
    for pose, goal_y, dy in [((1.0, 2.0, 1.5), 32.0, 10), ((1.0, 2.0, 1.5), 30.0, 10), ((6.13, 0.37, 1.5707963267948966), 76.0, 10),
                             ((3.0, 71.0, 1.2), 76.0, 10), ((5.5, 75.9, 1.6), 76.0, 10), ((2.25, 6.0, 1.4), 76.0, 10), ((4.0, 0.1, 1.7), 40.1, 2.5),
                             ((4.0, 80.0, 1.7), 76.0, 10), ((4.0, 90.0, 1.7), 76.0, 10), ((7.7, 3.3, 1.0), 76.0, 7)]:
        straight.append({"pose": list(pose), "goal_y": goal_y, "dy": dy, "path": pol.straight_planner(pose, (0, goal_y), dy).tolist()})

    out = {"action_scale": ACTION_SCALE, "dt": 0.005, "calls": total, "dropped": dropped,
           "kept_by_branch": {str(k): v for k, v in kept_by_branch.items()}, "max_yaw_diff": max_yaw, "max_surge_diff": max_surge,
           "max_state_diff": max_state, "cases": cases, "straight": straight}
    dst = os.path.join(HERE, "track_golden.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s: %d bytes, %d calls, %d dropped, kept by branch %s, max yaw / surge / state difference %.3g / %.3g / %.3g"
          % (dst, os.path.getsize(dst), total, dropped, kept_by_branch, max_yaw, max_surge, max_state))


if __name__ == "__main__":
    main(sys.argv[1])
