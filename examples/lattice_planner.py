"""The reference's lattice planner over a batch, on the device: python examples/lattice_planner.py [--envs 64] [--steps 30] (on an MI355X box).

The loop of ``LatticePlanner.plan`` (baselines/ship_ice_nav/planning_based/planners/lattice.py) for every env at once and with no host synchronisation:
cost maps (cost_maps) -> lattice A* from each ship's pose to the horizon's goal line (lattice_search) -> the sampled path of each node path
(planning.lattice_full_paths) -> the swath cost of the new and of the kept path over the same row window (swath_costs) -> ``Path.update``'s comparison
(planning.replan_mask).  The control set is data: by default the 8-heading set recorded from the reference in tests/golden/lattice_golden.json.  The ship
is then steered along the kept path by a plain pure-pursuit rule; the tracking controller of the reference's policy is not ported, and the script makes
no claim about how well this steers.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
from benchpush_amd.planning import (LATTICE_SHIP_VERTICES, LatticePrimitives, lattice_full_paths, lattice_swath_masks, replan_mask, ship_footprint)

SCALE, PADDING, HORIZON_M = 5, 0.25, 30          # the reference's lattice_config.yaml: cells per metre, footprint padding, receding horizon in metres
LOOKAHEAD = 15.0                                  # pure pursuit: cells ahead of the ship on the kept path


def load_control_set(path=None, key="set_8"):
    with open(path or os.path.join(ROOT, "tests", "golden", "lattice_golden.json")) as f:
        s = json.load(f)[key]
    return LatticePrimitives(s["edges"], 4 * len(s["edges"]), SCALE, s["turning_radius"], 0.1)


class Planner:
    def __init__(self, env, prims=None):
        self.env, self.prims = env, prims or load_control_set()
        self.fp_np = ship_footprint(LATTICE_SHIP_VERTICES, SCALE, PADDING)
        self.fp = torch.from_numpy(self.fp_np).to(env.device)
        self.path = self.lengths = None
        self.found = torch.zeros((), dtype=torch.int64, device=env.device)

    def plan(self):
        """One planning round; returns the kept paths [E, P, 3] and their lengths [E] (device tensors)."""
        env, dev, cfg = self.env, self.env.device, self.env.cfg
        m, n = int(cfg.occ.map_height), int(cfg.occ.map_width)
        pose = env.info[:, :3] * torch.tensor([SCALE, SCALE, 1.0], dtype=torch.float64, device=dev)
        half = float(self.fp_np[:, 0].max() - self.fp_np[:, 0].min()) / 2
        maps = env.cost_maps(SCALE, m, n, horizon=HORIZON_M, ship_pos_y=pose[:, 1] - half, vs=float(cfg.target_speed) * SCALE + 1e-8)
        goal_y = torch.clamp(pose[:, 1] + HORIZON_M * SCALE, max=float(cfg.goal_y) * SCALE).contiguous()
        masks = lattice_swath_masks(env, self.prims, self.fp_np, pose[:, 2])
        res = env.lattice_search(maps, pose.contiguous(), goal_y, self.prims, masks)
        new, new_len = lattice_full_paths(self.prims, res, pose)
        self.found += (res.status == 0).sum()
        if self.path is None:
            self.path, self.lengths = new, new_len
            return self.path, self.lengths
        # Path.update: both swath costs over the rows from the ship to the goal line
        rows = torch.stack([pose[:, 1].to(torch.int32), goal_y.to(torch.int32)], 1).contiguous()
        both = torch.stack([new, self.path], 1).contiguous()
        cost = env.swath_costs(both, self.fp, maps, lengths=torch.stack([new_len, self.lengths], 1).contiguous(), rows=rows)
        take = (new_len > 0) & (replan_mask(cost[:, 0], cost[:, 1], 0.95) | (self.lengths == 0))
        self.path = torch.where(take[:, None, None], new, self.path)
        self.lengths = torch.where(take, new_len, self.lengths)
        return self.path, self.lengths

    def actions(self):
        """Pure pursuit of the kept path: yaw actions [E] in [-1, 1]."""
        env, dev = self.env, self.env.device
        pose = env.info[:, :3] * torch.tensor([SCALE, SCALE, 1.0], dtype=torch.float64, device=dev)
        P = self.path.shape[1]
        valid = torch.arange(P, device=dev)[None, :] < self.lengths[:, None]
        d = torch.hypot(self.path[:, :, 0] - pose[:, None, 0], self.path[:, :, 1] - pose[:, None, 1])
        ahead = valid & (d >= LOOKAHEAD) & (self.path[:, :, 1] > pose[:, None, 1])
        idx = torch.where(ahead.any(1), ahead.to(torch.int64).argmax(1), (self.lengths.to(torch.int64) - 1).clamp_min(0))
        tgt = self.path[torch.arange(self.path.shape[0], device=dev), idx]
        bearing = torch.atan2(tgt[:, 1] - pose[:, 1], tgt[:, 0] - pose[:, 0])
        err = torch.remainder(bearing - pose[:, 2] + torch.pi, 2 * torch.pi) - torch.pi
        return torch.where(self.lengths > 0, (2.0 * err).clamp(-1.0, 1.0), torch.zeros_like(err))


def run(envs=64, steps=30, every=5):
    env = BatchedShipIceEnv(envs, cfg={"concentration": 0.3}, num_trials=8)
    env.reset()
    planner = Planner(env)
    for t in range(steps):
        if t % every == 0:
            planner.plan()
        _, _, terminated, truncated, _ = env.step(planner.actions())
        env.reset((terminated | truncated))
    _, counts = env.episode_metrics()
    finished, found = int((counts > 0).sum()), int(planner.found)
    env.check_errors()
    env.close()
    return finished, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--every", type=int, default=5)
    a = ap.parse_args()
    finished, found = run(a.envs, a.steps, a.every)
    print("%d envs, %d steps: %d searches found a path, %d envs finished an episode" % (a.envs, a.steps, found, finished))


if __name__ == "__main__":
    main()
