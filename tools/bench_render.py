"""Cost of rgb_array frames (k_render): device-event time per call after warm-up for k in {1, 16, 256} frames per task at the default scale and at
s / 4, frame bytes per second, and an A/B of a ship-ice step loop with and without rendering 16 frames per step (the two alternated in one process).

    python tools/bench_render.py [--envs 4096] [--steps 20] [--reps 10] [--out profiles/render/bench_render.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(task, E):
    if task == "ship_ice":
        from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
        return BatchedShipIceEnv(E, num_trials=16)
    if task == "maze":
        from benchpush_amd.envs.maze_namo import BatchedMazeEnv
        return BatchedMazeEnv(E, num_layouts=16)
    if task == "box_delivery":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(E, num_trials=16)
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    return BatchedAreaClearingEnv(E, num_trials=16)


def time_render(env, ids, scale, reps):
    out = env.render_frames(ids, scale=scale)          # warm-up (also uploads the table)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        env.render_frames(ids, scale=scale, out=out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out[0].numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/render/bench_render.json")
    ap.add_argument("--skip-ab", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "render": [], "ab": None}
    for task in ("ship_ice", "maze", "box_delivery", "area_clearing"):
        env = make(task, 256)
        env.reset()
        env.step(torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, 256)))
        s0 = float(env.cfg.render_scale)
        for s in (s0, s0 / 4):
            for k in (1, 16, 256):
                ms, fb = time_render(env, list(range(k)), s, a.reps)
                row = dict(task=task, scale=s, k=k, frame_hw=list(env.frame_size(s)), ms=round(ms, 4), frames_per_s=round(k / ms * 1e3, 1),
                           gbytes_per_s=round(k * fb / ms / 1e6, 2))
                res["render"].append(row)
                print(json.dumps(row), flush=True)
        env.close()
    if not a.skip_ab:
        from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
        env = BatchedShipIceEnv(a.envs, num_trials=100)
        env.reset()
        rng = np.random.default_rng(1)
        acts = [torch.from_numpy(rng.uniform(-1, 1, a.envs)).cuda() for _ in range(8)]
        ids = list(range(16))
        out = env.render_frames(ids)
        for i in range(3):
            env.step(acts[i % 8])
        torch.cuda.synchronize()
        t = {"plain": [], "render16": []}
        for rep in range(4):                          # alternate the two loops: same clocks, same thermal state
            for mode in ("plain", "render16") if rep % 2 == 0 else ("render16", "plain"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    env.step(acts[i % 8])
                    if mode == "render16":
                        env.render_frames(ids, out=out)
                torch.cuda.synchronize()
                t[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
        env.check_errors()
        res["ab"] = dict(envs=a.envs, steps_per_rep=a.steps, ms_per_step_plain=[round(x, 3) for x in t["plain"]],
                         ms_per_step_render16=[round(x, 3) for x in t["render16"]],
                         overhead_pct=round((np.median(t["render16"]) / np.median(t["plain"]) - 1) * 100, 2))
        print(json.dumps(res["ab"]), flush=True)
        env.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
