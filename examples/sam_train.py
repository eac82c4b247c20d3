"""A short SAM run, train then evaluate: python examples/sam_train.py [box|area] [envs] [batch] [timesteps] [episodes]

The rollout is the ready queue with a DeviceReplayBuffer attached (README "A replay buffer on the ready queue, and the SAM baseline"): recv ->
predict_batch -> send, then one double-DQN update per recv on a batch sampled on the device.  A timestep is one delivered row slot (recvs * batch).
The sizes here are for a look at the loop, not for a trained policy: the reference's schedule is 60000 timesteps.
"""
import logging
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    task = sys.argv[1] if len(sys.argv) > 1 else "box"
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    M = int(sys.argv[3]) if len(sys.argv) > 3 else max(1, E // 4)
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 40 * M
    episodes = int(sys.argv[5]) if len(sys.argv) > 5 else E
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if task == "area":
        from benchpush_amd.baselines.area_clearing.sam import AreaClearingSAM as Policy
    else:
        from benchpush_amd.baselines.box_delivery.SAM import BoxDeliverySAM as Policy
    out = tempfile.mkdtemp(prefix="sam_")
    train = dict(total_timesteps=steps, learning_starts=4 * M, exploration_timesteps=steps // 2, replay_buffer_size=2000, target_update_freq=10 * M,
                 checkpoint_freq=steps, log_freq=10 * M)
    policy = Policy(cfg={"train": train}, model_name="sam_example", model_path=os.path.join(out, "models"), checkpoint_root=os.path.join(out, "checkpoint"),
                    num_envs=E, queue_batch=M, num_trials=32)
    summary = policy.train("example")
    print("trained: %d timesteps, %d updates, last loss %.4g, buffer %s" % (summary["timesteps"], summary["updates"], summary["loss"], summary["buffer"]))
    print("model: %s\ncheckpoint (with the replay buffer): %s" % (summary["model"], summary["checkpoint"]))
    success, efficiency, effort, rewards, name = policy.evaluate(episodes, max_episode_steps=50)
    mean = lambda v: sum(v) / max(1, len(v))   # noqa: E731
    print("%s: %d episodes, mean success %.3f, mean reward %.3f" % (name, len(rewards), mean(success), mean(rewards)))


if __name__ == "__main__":
    main()
