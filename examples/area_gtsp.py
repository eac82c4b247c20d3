"""The planning-based area-clearing baseline on the device: plan the pushes of every env (one push path per box and boundary edge, the optimal tour
by an exact set DP), steer along the plan with the reference's controller, and write frames with the plan drawn.

    python examples/area_gtsp.py [--envs 4] [--steps 40] [--out area_gtsp_frames]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default="area_gtsp_frames")
    a = ap.parse_args()
    from benchpush_amd import _lib
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    env = BatchedAreaClearingEnv(a.envs, cfg={"agent": {"action_type": "velocity"}})
    env.reset()
    plan = env.gtsp_plan()                       # from the env's own poses and boxes; nothing is copied to the host
    tracker = plan.tracker()
    status, n_push, cost, lengths = (t.cpu().numpy() for t in (plan.status, plan.n_push, plan.cost, plan.lengths))
    for e in range(a.envs):
        print("env %d: status %d flags %#x, %d boxes to push, tour cost %d (= 100 * (0.5 m + pi / 4 rad)), tour %s"
              % (e, status[e] & _lib.GTSP_STATUS_MASK, status[e] & ~_lib.GTSP_STATUS_MASK, n_push[e], cost[e], plan.tour[e, :n_push[e]].tolist()))
    paths = [p[:n] for p, n in zip(plan.paths.cpu().numpy(), lengths)]
    os.makedirs(a.out, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for k in range(a.steps):
        actions, ids = env.track_pushes(plan, tracker)
        env.step(actions)
        if k % 10 == 0 or k == a.steps - 1:
            frames = env.render_frames(paths=paths).cpu().numpy()
            for e in range(a.envs):
                name = os.path.join(a.out, "env%d_step%03d" % (e, k))
                Image.fromarray(frames[e]).save(name + ".png") if Image else np.save(name + ".npy", frames[e])
            print("step %d: waypoint ids %s, boxes cleared %s" % (k, ids.tolist(), env.info[:, 7].int().tolist()))
    env.check_errors()
    env.close()


if __name__ == "__main__":
    main()
