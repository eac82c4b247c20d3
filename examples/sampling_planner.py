"""A sampling planner for ship-ice that never leaves the device: python examples/sampling_planner.py [--envs 64] [--steps 60] (on an MI355X box).

Every `--every` steps each env builds its planner cost map (cost_maps), fans K constant-curvature arcs out of its ship's pose (planning.arc_paths),
scores them with the swath cost of the padded ship footprint (swath_costs, outside="reject": an arc that leaves the channel costs +inf) plus a progress
term, and steers along the cheapest one.  cost maps, arcs, swath costs, argmin and the action are device tensors from start to end: the loop has no
host synchronisation.  The script prints the episode metrics beside a run that always steers straight (action 0); it demonstrates the calls and makes
no claim that this planner beats anything.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
from benchpush_amd.planning import LATTICE_SHIP_VERTICES, arc_paths, ship_footprint

SCALE, PADDING = 5, 0.25          # cells per metre and footprint padding of the reference's lattice planner configuration
HORIZON_M, STEP_CELLS = 6.0, 1.0  # arc length in metres, sample spacing in cells
PROGRESS_WEIGHT = 1.0             # cost per cell that the arc's end stays short of the goal line


def plan(env, num_candidates=5, footprint=None):
    """Yaw actions [E] in [-1, 1] for the envs' current states (device tensor; nothing is copied to the host)."""
    cfg, dev = env.cfg, env.device
    m, n = int(cfg.occ.map_height), int(cfg.occ.map_width)
    speed = float(cfg.target_speed)
    if footprint is None:
        footprint = torch.from_numpy(ship_footprint(LATTICE_SHIP_VERTICES, SCALE, PADDING)).to(dev)
    pose = env.info[:, :3] * torch.tensor([SCALE, SCALE, 1.0], dtype=torch.float64, device=dev)     # metres -> cells
    maps = env.cost_maps(SCALE, m, n, vs=speed * SCALE + 1e-8)
    # a constant action a turns the ship by a * max_yaw_rate_step per second at target_speed: curvature a * max_yaw_rate_step / target_speed per metre
    kmax = env.max_yaw_rate_step / (SCALE * speed)
    curvature = torch.linspace(-kmax, kmax, num_candidates, dtype=torch.float64, device=dev)
    paths = arc_paths(pose, curvature, HORIZON_M * SCALE, STEP_CELLS)
    cost = env.swath_costs(paths, footprint, maps, outside="reject")
    short = (float(cfg.goal_y) * SCALE - paths[:, :, -1, 1]).clamp_min(0.0)
    score = cost + PROGRESS_WEIGHT * short
    best = torch.argmin(score, dim=1)
    # every arc rejected (the ship is at the channel's edge): steer back towards the middle of the channel
    middle = torch.sign(pose[:, 0] - 0.5 * n * SCALE) * torch.sign(torch.sin(pose[:, 2])) * kmax
    k = torch.where(torch.isinf(score).all(dim=1), middle, curvature[best])
    return (k * SCALE * speed / env.max_yaw_rate_step).clamp(-1.0, 1.0)


def run(envs, steps, every, planner, candidates):
    env = BatchedShipIceEnv(envs, cfg={"concentration": 0.3}, num_trials=8)
    env.reset()
    actions = torch.zeros(envs, dtype=torch.float64, device=env.device)
    for t in range(steps):
        if planner and t % every == 0:
            actions = plan(env, candidates)
        _, _, terminated, truncated, _ = env.step(actions)
        env.reset((terminated | truncated))
    rows, counts = env.episode_metrics()
    done = counts > 0
    mean = rows[done].mean(dim=0).tolist() if bool(done.any()) else [float("nan")] * 6
    env.check_errors()
    env.close()
    return int(done.sum()), mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--every", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=9)
    a = ap.parse_args()
    names = ["efficiency", "effort", "reward", "success", "length", "total_work"]
    for label, planner in (("sampling planner", True), ("action 0", False)):
        finished, mean = run(a.envs, a.steps, a.every, planner, a.candidates)
        print("%-17s %3d envs finished an episode; means: %s" % (label, finished, "  ".join("%s %.4g" % (k, v) for k, v in zip(names, mean))))


if __name__ == "__main__":
    main()
