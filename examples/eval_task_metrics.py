"""Score box-delivery and area-clearing episodes on the device: a random-action box-delivery batch and the GTSP planning baseline on an area-clearing
batch, both scored by the on-device TaskDrivenMetric (episode_history(): no per-step host copies of polygons or info rows).

    python examples/eval_task_metrics.py --envs 64 --episodes 128 --t-max 200
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mean(v):
    v = [x for x in v if x == x and abs(x) != float("inf")]      # an episode without movement has 0 / 0 or x / 0 in its scores
    return sum(v) / len(v) if v else float("nan")


def random_box_delivery(envs, episodes, seed, inactivity_cutoff):
    import torch
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    from benchpush_amd.parallel import summarize_episode_sums
    env = BatchedBoxDeliveryEnv(envs, cfg={"misc": {"inactivity_cutoff": inactivity_cutoff}})
    env.reset()
    gen = torch.Generator().manual_seed(seed)
    while True:
        _, _, term, trunc, _ = env.step((torch.rand(envs, generator=gen, dtype=torch.float64) * 2 - 1).to(env.device))
        done = (term != 0) | (trunc != 0)
        if bool(done.any()):
            env.reset(done)
            _, sums, counts = env.episode_history()
            if int(counts.sum()) >= episodes:
                break
    env.check_errors()
    lists = env.episode_lists()
    env.close()
    rows = [r for rows in lists for r in rows]
    print("box-delivery, random headings: %d episodes finished" % int(counts.sum()))
    print("  means over the last <= 8 episodes of every env: success %.3f  efficiency %.3f  effort %.3f"
          % (mean([r[3] for r in rows]), mean([r[0] for r in rows]), mean([r[1] for r in rows])))
    print("  sums / counts over all of them:", summarize_episode_sums(sums, counts))


def gtsp_area_clearing(envs, episodes, t_max):
    from benchpush_amd.baselines.area_clearing.planning_based.policy import PlanningBasedPolicy
    pol = PlanningBasedPolicy(num_envs=envs, t_max=t_max)
    success, eff, effort, rewards, name = pol.evaluate(episodes)
    pol.close()
    print("area-clearing, %s baseline: %d episodes finished" % (name, len(success)))
    print("  mean success %.3f  efficiency %.3f  effort %.3f  reward %.3f" % (mean(success), mean(eff), mean(effort), mean(rewards)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=128)
    ap.add_argument("--t-max", type=int, default=200, help="sim.t_max of the area-clearing batch (the reference evaluates with 2000)")
    ap.add_argument("--inactivity-cutoff", type=int, default=20, help="misc.inactivity_cutoff of the box-delivery batch")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    random_box_delivery(a.envs, a.episodes, a.seed, a.inactivity_cutoff)
    gtsp_area_clearing(a.envs, a.episodes, a.t_max)
