"""Cost of one gtsp_plan call (k_gtsp_plan) and one track_pushes call (k_gtsp_track) over a batch, in ONE process: device-event time per launch at
the reference's parameters, for the env's own 10 boxes (max_boxes 10) and for 12 boxes per env at the cap (max_boxes 12), with 4 goal segments, next
to the workspace sizes and one env.step of the same run.  Run it under a time limit:

    timeout 600 python tools/bench_gtsp.py [--envs 4096] [--reps 20] [--out profiles/gtsp]

Every env of a launch solves a different instance (its own trial's boxes, or its own random draw); the time of a launch does not depend on the
weights, only on n: the DP visits every set.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3),
                reps=reps, warmup=warmup)               # every entry says how it was timed: env_step takes fewer launches than the rest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/gtsp")
    a = ap.parse_args()
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    from benchpush_amd.planning import GTSPConfig
    E = a.envs
    env = BatchedAreaClearingEnv(E, cfg={"agent": {"action_type": "velocity"}})
    env.reset()
    res = dict(device=torch.cuda.get_device_name(0), E=E)
    rng = np.random.default_rng(0)
    boxes12 = np.zeros((E, 12, 20, 2))
    c, ang = rng.uniform(-4.3, 4.3, (E, 12, 1, 2)), rng.uniform(0, math.pi / 2, (E, 12, 1))
    corners = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float64) * 0.5
    boxes12[:, :, :4, 0] = c[..., 0] + np.cos(ang) * corners[:, 0] - np.sin(ang) * corners[:, 1]
    boxes12[:, :, :4, 1] = c[..., 1] + np.sin(ang) * corners[:, 0] + np.cos(ang) * corners[:, 1]
    cases = (("n10_env_state", GTSPConfig(max_boxes=10), None, None),
             ("n12_at_the_cap", GTSPConfig(max_boxes=12), torch.from_numpy(boxes12).to(env.device),
              torch.full((E, 12), 4, dtype=torch.int32, device=env.device)))
    for name, cfg, boxes, counts in cases:
        plan = None
        ws = torch.empty(env.gtsp_workspace_bytes(cfg), dtype=torch.uint8, device=env.device)

        def call():
            nonlocal plan
            plan = env.gtsp_plan(boxes=boxes, counts=counts, config=cfg, workspace=ws, out=plan)

        t = timed(call, a.reps, 2)
        tr = plan.tracker()
        out = None

        def track():
            nonlocal out
            out = env.track_pushes(plan, tr, config=cfg, out=out)

        st = plan.status.cpu().numpy()
        res[name] = dict(plan=t, track=timed(track, a.reps, 2), workspace_MB=round(ws.numel() / 2 ** 20, 1),
                         workspace_KB_per_env=round(ws.numel() / E / 1024, 1), n_push=dict(min=int(plan.n_push.min()), max=int(plan.n_push.max())),
                         status_codes=np.bincount(st & 0xFF, minlength=5).tolist(), degenerate_envs=int(((st & 0x200) != 0).sum()),
                         cost=dict(mean=float(plan.cost.double().mean()), min=int(plan.cost.min()), max=int(plan.cost.max())))
        del ws
    act = torch.zeros((E, 2), dtype=torch.float64, device=env.device)
    res["env_step"] = timed(lambda: env.step(act), 5, 1)
    env.check_errors()
    os.makedirs(os.path.join(ROOT, a.out), exist_ok=True)
    with open(os.path.join(ROOT, a.out, "bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
