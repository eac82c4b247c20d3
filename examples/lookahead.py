"""One-step look-ahead on ship-ice with forked environments: python examples/lookahead.py [--steps 20] [--branches 7] (on an MI355X box).

Env 0 is the real episode, envs 1..K are branches.  Every step env 0 is fanned out into the branches (clone_envs: one kernel launch), each branch takes
one candidate yaw action, and the real env -- put back by restore_state -- takes the action of the branch with the largest reward.  Restored and cloned
envs continue bit for bit, so the reward the real env then receives is exactly the one its branch predicted; the script checks that.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--branches", type=int, default=7)
    a = ap.parse_args()
    K = a.branches
    env = BatchedShipIceEnv(1 + K, cfg={"concentration": 0.3}, num_trials=4)
    env.reset()
    candidates = torch.linspace(-1, 1, K, dtype=torch.float64, device=env.device)
    branches = list(range(1, K + 1))
    total = 0.0
    for t in range(a.steps):
        s = env.save_state([0])
        env.clone_envs([0] * K, branches)
        actions = torch.zeros(1 + K, dtype=torch.float64, device=env.device)
        actions[1:] = candidates
        _, reward, _, _, _ = env.step(actions)                     # env 0 steps too; it is put back below
        j = int(torch.argmax(reward[1:]).item())
        predicted = float(reward[1 + j])
        env.restore_state(s, [0])
        actions[0] = candidates[j]
        _, reward, terminated, _, info = env.step(actions)
        assert float(reward[0]) == predicted, "a restored env must continue exactly as its branch did"
        total += predicted
        print("step %2d: action %+.2f reward %+.4f  x %.2f y %.2f" % (t, float(candidates[j]), predicted, float(info[0, 0]), float(info[0, 1])))
        if bool(terminated[0]):
            print("goal reached after %d steps" % (t + 1))
            break
    env.check_errors()
    print("return %.4f" % total)
    env.close()


if __name__ == "__main__":
    main()
