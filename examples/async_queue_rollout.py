"""Asynchronous rollout through the ready queue: python examples/async_queue_rollout.py [box|area] [envs] [batch] [calls] [budget]

recv() returns exactly `batch` rows -- env ids and their transitions, densely packed, a constant shape for the policy -- and send() gives those envs their
next actions; done envs are reset by the same send and come back as fresh rows (their reset observation, slices == 0).  The queue between the two lives on
the device: this loop reads nothing back, so the host runs ahead of the GPU.  Compare examples/async_rollout.py, which sizes the policy's batch with
``ready.nonzero()`` in every call.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


class RandomPolicy:
    """Stands for a network: maps a batch of observations to heading actions."""

    def __init__(self, device):
        self.g = torch.Generator(device=device)
        self.g.manual_seed(0)

    def __call__(self, obs_rows):
        return torch.rand(obs_rows.shape[0], generator=self.g, device=obs_rows.device, dtype=torch.float64) * 2 - 1


def main():
    task = sys.argv[1] if len(sys.argv) > 1 else "box"
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    M = int(sys.argv[3]) if len(sys.argv) > 3 else max(1, E // 4)
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    if task == "area":
        from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv as Env
    else:
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv as Env
    env = Env(E, num_trials=32)
    budget = int(sys.argv[5]) if len(sys.argv) > 5 else None    # None: the task's default
    policy = RandomPolicy(env.device)
    env.reset()
    q = env.async_queue(batch_size=M, budget=budget)            # every env is queued with its reset observation
    transitions = torch.zeros(E, dtype=torch.int64, device=env.device)
    returns = torch.zeros(E, dtype=torch.float64, device=env.device)
    for _ in range(calls):
        ids, obs, reward, terminated, truncated, info = q.recv()    # [M, ...] device tensors; rows beyond the count have id -1 and zeros
        row = ids.clamp(min=0).long()                               # (rows with id -1 add zeros to env 0)
        transitions.index_add_(0, row, (q.slices > 0).long())       # a learner would store (ids, obs, reward, ...) here
        returns.index_add_(0, row, reward)
        q.send(policy(obs), ids, reset=terminated | truncated)      # rows with id -1 are ignored
    q.close()                                                       # finishes what is in flight; step() / save_state() work again
    env.check_errors()
    t, s = transitions.cpu(), q.stats()
    print("%s: %d envs, batch %d, %d recvs of %d sim steps: %d transitions, mean fill %.2f, %d rejected rows; per env min / median / max = %d / %d / %d"
          % (task, E, M, calls, q.budget, int(t.sum()), s["mean_fill"], s["rejected"], int(t.min()), int(t.median()), int(t.max())))
    env.close()


if __name__ == "__main__":
    main()
