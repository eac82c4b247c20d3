"""The reference's lattice planner over a batch, on the device: python examples/lattice_planner.py [--envs 64] [--steps 30] [--pursuit] (on an MI355X box).

The loop of ``LatticePlanner.plan`` (baselines/ship_ice_nav/planning_based/planners/lattice.py) for every env at once and with no host synchronisation
(benchpush_amd.planning.BatchedLatticePlanner): cost maps (cost_maps) -> lattice A* from each ship's pose to the horizon's goal line (lattice_search) ->
the sampled path of each node path (planning.lattice_full_paths) -> the swath cost of the new and of the kept path over the same row window (swath_costs)
-> ``Path.update``'s comparison (planning.replan_mask).  The control set is data: by default the 8-heading set recorded from the reference in
tests/golden/lattice_golden.json.  The ship is then steered along the kept path by the tracking controller of the reference's policy
(BatchedShipIceEnv.track_paths, one launch per step); --pursuit steers with a plain pure-pursuit rule instead.  The script makes no claim about how
well either steers.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
from benchpush_amd.planning import BatchedLatticePlanner, LatticePrimitives, TrackerState

SCALE, PADDING, HORIZON_M = 5, 0.25, 30          # the reference's lattice_config.yaml: cells per metre, footprint padding, receding horizon in metres
LOOKAHEAD = 15.0                                  # pure pursuit: cells ahead of the ship on the kept path


def load_control_set(path=None, key="set_8"):
    with open(path or os.path.join(ROOT, "tests", "golden", "lattice_golden.json")) as f:
        s = json.load(f)[key]
    return LatticePrimitives(s["edges"], 4 * len(s["edges"]), SCALE, s["turning_radius"], 0.1)


class Planner(BatchedLatticePlanner):
    def __init__(self, env, prims=None):
        super().__init__(env, prims or load_control_set(), SCALE, PADDING, HORIZON_M)

    def actions(self):
        """Pure pursuit of the kept path: yaw actions [E] in [-1, 1]."""
        return self.pursuit_actions(LOOKAHEAD)


def run(envs=64, steps=30, every=5, pursuit=False):
    env = BatchedShipIceEnv(envs, cfg={"concentration": 0.3}, num_trials=8)
    env.reset()
    planner = Planner(env)
    tracker = TrackerState(envs, env.device)
    zero = torch.zeros(envs, dtype=torch.float64, device=env.device)
    for t in range(steps):
        if t % every == 0:
            planner.plan()
        if pursuit:
            act = planner.actions()
        else:   # an env without a path has nothing written: it goes straight on
            actions, _, _ = env.track_paths(planner.paths_metres(), tracker, lengths=planner.lengths)
            act = torch.where(planner.lengths > 0, actions[:, 0], zero)
        _, _, terminated, truncated, _ = env.step(act)
        done = terminated | truncated
        tracker.reset(done)
        env.reset(done)
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
    ap.add_argument("--pursuit", action="store_true", help="steer with the pure-pursuit rule instead of track_paths")
    a = ap.parse_args()
    finished, found = run(a.envs, a.steps, a.every, a.pursuit)
    print("%d envs, %d steps: %d searches found a path, %d envs finished an episode" % (a.envs, a.steps, found, finished))


if __name__ == "__main__":
    main()
