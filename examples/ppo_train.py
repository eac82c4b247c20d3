"""A short PPO run, train then evaluate: python examples/ppo_train.py [ship|maze] [envs] [n_steps] [rollouts] [episodes]

The collection loop steps the envs of a BatchedVecEnv(to_numpy=False) with a DeviceRolloutBuffer attached (README "A rollout buffer with GAE, and the PPO
baselines"): begin -> env step -> truncated_rows -> value forward -> end, then finish and the epochs of minibatches.  A timestep is one env transition.
The sizes here are for a look at the loop, not for a trained policy: the reference's schedule is 200000 timesteps.
"""
import logging
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    task = sys.argv[1] if len(sys.argv) > 1 else "ship"
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    n_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    rollouts = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    episodes = int(sys.argv[5]) if len(sys.argv) > 5 else E
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if task == "maze":
        from benchpush_amd.baselines.maze_NAMO.ppo import MazeNAMOPPO as Policy
        cfg, kw = {}, dict(num_layouts=16)
    else:
        from benchpush_amd.baselines.ship_ice_nav.ppo import ShipIcePPO as Policy
        cfg, kw = {"concentration": 0.2}, dict(num_trials=16)
    out = tempfile.mkdtemp(prefix="ppo_")
    cfg["train"] = dict(n_steps=n_steps, batch_size=max(8, E * n_steps // 4), n_epochs=2, total_timesteps=rollouts * n_steps * E,
                        checkpoint_freq=n_steps * E)
    policy = Policy("ppo_example", os.path.join(out, "models"), cfg, num_envs=E, **kw)
    summary = policy.train()
    print("trained: %d timesteps, %d updates, last loss %.4g, buffer %s" % (summary["timesteps"], summary["updates"], summary["loss"], summary["buffer"]))
    print("model: %s\ncheckpoints: %s" % (summary["model"], ", ".join(os.path.basename(c) for c in summary["checkpoints"])))
    efficiency, effort, rewards, name = policy.evaluate(episodes)
    mean = lambda v: sum(v) / max(1, len(v))   # noqa: E731
    print("%s: %d episodes, mean efficiency %.3f, mean reward %.3f" % (name, len(rewards), mean(efficiency), mean(rewards)))


if __name__ == "__main__":
    main()
