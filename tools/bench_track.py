"""Cost of one track_paths call (k_track_path) over a batch, in ONE process: device-event time per launch, 5 warm-up launches and 20 timed ones at
E = 4096, next to the time of one env.step of the same run.  Two shapes: P of the straight planner (goal_y + dy / 2 over dy samples, + 1) with the
straight planner's own paths, and P = the lattice planner's Pmax ((max_path_nodes - 1) * samples of the longest primitive, spacing 0.1 cell = 0.02 m)
with synthetic gently curved paths -- once with every sample counted (the worst case) and once with the 15 primitives of a typical plan
(profiles/lattice/README.md).  The ships stand at their reset poses, 0 .. 14 m beside the path so that every branch runs.  Run it under a time limit:

    timeout 600 python tools/bench_track.py [--envs 4096] [--out profiles/track]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "examples")]


def timed(fn, reps=20, warmup=5):
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
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(np.min(ts)), 4), max_ms=round(float(np.max(ts)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default="profiles/track")
    a = ap.parse_args()
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from benchpush_amd.planning import TrackerState, straight_paths
    from lattice_planner import load_control_set
    E = a.envs
    env = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, num_trials=100)
    env.reset()
    dev = env.device
    acts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, E)).to(dev)
    for _ in range(3):
        env.step(acts)
    res = dict(device=torch.cuda.get_device_name(0), E=E, reps=20, warmup=5)
    res["env_step"] = timed(lambda: env.step(acts))
    poses = env.info[:, :3].contiguous()
    offs = torch.linspace(0.0, 14.0, E, dtype=torch.float64, device=dev)        # beside the path: near and far envs
    state = TrackerState(E, dev)
    out = None

    def call(paths, lengths):
        nonlocal out
        out = env.track_paths(paths, state, lengths=lengths, poses=poses, out=out)

    # the straight planner's own paths
    dy, goal_y = 10, float(env.cfg.goal_y)
    sp, sl = straight_paths(poses, goal_y, dy, max_len=int(np.ceil((goal_y + dy * 0.5) / dy)) + 1)
    sp[:, :, 0] += offs[:, None]
    res["straight"] = dict(P=int(sp.shape[1]), **timed(lambda: call(sp, sl)))
    res["straight"]["branches"] = torch.bincount(out[2][:, 1].long(), minlength=4).tolist()
    # the lattice planner's shape
    prims = load_control_set()
    pm = max(prims.samples(b, k).shape[1] for b in range(prims.num_base_h) for k in range(len(prims.edges[b])))
    P = 127 * pm
    s = torch.arange(P, dtype=torch.float64, device=dev) * 0.02
    head = torch.pi / 2 + 0.3 * torch.sin(s / 6.0)
    x = torch.cumsum(0.02 * torch.cos(head), 0)[None, :] + poses[:, 0, None] + offs[:, None]
    y = torch.cumsum(0.02 * torch.sin(head), 0)[None, :] + poses[:, 1, None] - 1.0
    lp = torch.stack([x, y, head[None, :].expand(E, P)], -1).contiguous()
    full = torch.full((E,), P, dtype=torch.int32, device=dev)
    typical = torch.full((E,), 15 * pm, dtype=torch.int32, device=dev)
    state.reset()
    res["lattice_all_counted"] = dict(P=P, counted=P, **timed(lambda: call(lp, full)))
    res["lattice_all_counted"]["branches"] = torch.bincount(out[2][:, 1].long(), minlength=4).tolist()
    state.reset()
    res["lattice_typical"] = dict(P=P, counted=15 * pm, **timed(lambda: call(lp, typical)))
    res["lattice_typical"]["branches"] = torch.bincount(out[2][:, 1].long(), minlength=4).tolist()
    env.check_errors()
    env.close()
    print(json.dumps(res))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_track.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
