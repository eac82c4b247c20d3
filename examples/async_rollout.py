"""Asynchronous rollout of box-delivery-v0 (or area-clearing-v0): python examples/async_rollout.py [box|area] [envs] [calls] [budget]

step_async() hands back the envs whose env step ended (`ready`) and lets the others carry on, so a launch does not last as long as its slowest env.  The
policy is fed the ready rows only, ready & (terminated | truncated) envs are reset, and transitions are counted per env: envs advance at different rates,
because short env steps come back more often than long ones.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


class RandomPolicy:
    """Stands for a network: maps the observations of the ready envs to their next heading actions."""

    def __init__(self, device):
        self.g = torch.Generator(device=device)
        self.g.manual_seed(0)

    def __call__(self, obs_rows):
        return torch.rand(obs_rows.shape[0], generator=self.g, device=obs_rows.device, dtype=torch.float64) * 2 - 1


def main():
    task = sys.argv[1] if len(sys.argv) > 1 else "box"
    E = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    if task == "area":
        from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv as Env
    else:
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv as Env
    env = Env(E, num_trials=32)
    budget = int(sys.argv[4]) if len(sys.argv) > 4 else env.ASYNC_BUDGET
    policy = RandomPolicy(env.device)
    obs, info = env.reset()
    actions = policy(obs)                                   # every env is idle: every row is accepted by the first call
    transitions = torch.zeros(E, dtype=torch.int64, device=env.device)
    returns = torch.zeros(E, dtype=torch.float64, device=env.device)
    for _ in range(calls):
        obs, reward, terminated, truncated, info, ready = env.step_async(actions, budget)
        idx = ready.nonzero().squeeze(1)                    # (the one host synchronisation of this loop: the policy's batch size)
        if idx.numel():
            transitions[idx] += 1
            returns[idx] += reward[idx]                     # a learner would store (obs[idx], reward[idx], ...) here
            done = ready & (terminated | truncated)
            if bool(done.any()):
                obs, info = env.reset(done)                 # the rows of `done` now hold the first observation of the next episode
            actions[idx] = policy(obs[idx])                 # rows of busy envs are ignored by step_async
    obs, reward, terminated, truncated, info, ready = env.drain()   # finish what is in flight; the handle is closed for step() / save_state() again
    transitions += ready.long()
    env.check_errors()
    t = transitions.cpu()
    print("%s: %d envs, %d calls of %d sim steps: %d transitions; per env min / median / max = %d / %d / %d; calls per transition (last) max %d"
          % (task, E, calls, budget, int(t.sum()), int(t.min()), int(t.median()), int(t.max()), int(env.slices.max())))
    env.close()


if __name__ == "__main__":
    main()
