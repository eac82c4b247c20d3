"""A short SAC run, train then evaluate: python examples/sac_train.py [ship|maze] [envs] [steps] [episodes]

The loop steps the envs of a BatchedVecEnv(to_numpy=False) in lock step with a DeviceTransitionBuffer attached (README "A transition buffer for lock-step
envs, and the SAC baselines"): actions -> env step -> add -> one update from a sampled batch once past learning_starts.  A timestep is one env transition.
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
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 48
    episodes = int(sys.argv[4]) if len(sys.argv) > 4 else E
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if task == "maze":
        from benchpush_amd.baselines.maze_NAMO.sac import MazeNAMOSAC as Policy
        cfg, kw = {}, dict(num_layouts=16)
    else:
        from benchpush_amd.baselines.ship_ice_nav.sac import ShipIceSAC as Policy
        cfg, kw = {"concentration": 0.2}, dict(num_trials=16)
    out = tempfile.mkdtemp(prefix="sac_")
    cfg["train"] = dict(total_timesteps=steps * E, learning_starts=4 * E, batch_size=32, buffer_size=16 * E, checkpoint_freq=(steps // 3) * E)
    policy = Policy("sac_example", os.path.join(out, "models"), cfg, num_envs=E, **kw)
    summary = policy.train()
    print("trained: %d timesteps in %d steps, %d updates, last losses %s, buffer %s" % (summary["timesteps"], summary["steps"], summary["updates"],
                                                                                       summary["losses"], summary["buffer"]))
    print("model: %s\ncheckpoints: %s" % (summary["model"], ", ".join(os.path.basename(c) for c in summary["checkpoints"])))
    efficiency, effort, rewards, name = policy.evaluate(episodes)
    mean = lambda v: sum(v) / max(1, len(v))   # noqa: E731
    print("%s: %d episodes, mean efficiency %.3f, mean reward %.3f" % (name, len(rewards), mean(efficiency), mean(rewards)))


if __name__ == "__main__":
    main()
