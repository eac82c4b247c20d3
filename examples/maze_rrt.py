"""The planning-based maze-NAMO baseline step by step: plan a path for every env with the batched RRT, steer along it with the waypoint controller,
and write frames with the path drawn in.

    python examples/maze_rrt.py [--envs 4] [--steps 20] [--out frames_maze_rrt] [--maze-version 1] [--quick]

--quick plans with step 0.25 and 2000 nodes per pass instead of the reference's 0.05 and 26000.  Frames go to <out>/env<e>_<t>.png for the first two
envs (benchpush_amd.obs_log.write_rgb_png); nothing is shown on a screen.  At the end the reference-shaped single env (``MazeNAMO``) is given env 0's
first plan through ``update_path`` and writes <out>/single.png from ``render('rgb_array')``."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="frames_maze_rrt")
    ap.add_argument("--maze-version", type=int, default=1)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    from benchpush_amd import _lib
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv, MazeNAMO
    from benchpush_amd.planning import RRTConfig
    from benchpush_amd.obs_log import write_rgb_png
    env = BatchedMazeEnv(a.envs, cfg={"maze_version": a.maze_version}, num_layouts=8)
    env.reset()
    cfg = RRTConfig(step=0.25, max_nodes=2000) if a.quick else RRTConfig()
    plan = env.rrt_plan(config=cfg)
    names = ["found", "found ignoring boxes", "fallback", "blocked", "cap", "bad input", "skipped"]
    for e in range(a.envs):
        print("env %d: %s, %d waypoints, tree %s nodes after %s iterations" % (e, names[int(plan.status[e])], int(plan.lengths[e]),
                                                                               plan.n_nodes[e].tolist(), plan.iterations[e].tolist()))
    os.makedirs(a.out, exist_ok=True)
    shown = list(range(min(2, a.envs)))
    paths = [plan.paths[e, :int(plan.lengths[e])].cpu().numpy() for e in shown]
    first_path = paths[0]
    for t in range(a.steps):
        actions, _ = env.track_waypoints(plan.paths, plan.lengths, Lfc=cfg.Lfc, dt=cfg.dt)
        actions = torch.where(plan.lengths > 0, actions, torch.zeros_like(actions))
        _, _, term, _, _ = env.step(actions)
        frames = env.render_frames(env_ids=shown, paths=paths).cpu().numpy()
        for i, e in enumerate(shown):
            write_rgb_png(os.path.join(a.out, "env%d_%03d.png" % (e, t)), frames[i])
        if bool(term.any()):                # a finished env starts its next episode with a new plan, from the next RNG stream
            env.reset(term)
            gid = env.env_id_offset + torch.arange(a.envs, dtype=torch.int64, device=env.device)
            plan = env.rrt_plan(streams=gid * (1 << 32) + t + 1, active=term, config=cfg, out=plan)
            paths = [plan.paths[e, :int(plan.lengths[e])].cpu().numpy() for e in shown]
    env.check_errors()
    assert int(plan.status.max()) <= _lib.RRT_SKIPPED
    env.close()
    single = MazeNAMO(cfg={"maze_version": a.maze_version}, num_layouts=8)     # env 0 of the batch played the same layout
    single.reset()
    single.update_path(first_path)
    write_rgb_png(os.path.join(a.out, "single.png"), single.render("rgb_array"))
    single.close()
    print("wrote %d frames to %s" % (a.steps * len(shown), a.out))


if __name__ == "__main__":
    main()
