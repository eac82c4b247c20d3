"""Cost of one swath_costs call (k_swath_cost) beside one env.step of the same environments, in ONE process: device-event time per call, 3 warm-up calls
and 20 timed ones, ship-ice at 30 % concentration, the envs' own 380 x 60 cost maps, the 17-vertex padded footprint of the lattice planner, K arcs
fanned out of every ship's pose and sampled every 0.5 cell.  Sizes (E, K, P): (4096, 16, 128), (4096, 64, 32), (256, 16, 128), each with outside="clip"
and "reject", without and with the masks.  Only figures of one run are comparable with each other.  Run it under a time limit:

    timeout 900 python tools/bench_swath.py [--reps 20] [--out profiles/swath]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(4096, 16, 128), (4096, 64, 32), (256, 16, 128)]
SCALE, STEP = 5, 0.5


def timed(fn, reps, warmup=3):
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/swath")
    a = ap.parse_args()
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from benchpush_amd.planning import LATTICE_SHIP_VERTICES, arc_paths, ship_footprint
    rows, step_ms = [], {}
    for E in sorted({s[0] for s in SIZES}, reverse=True):
        env = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, num_trials=100)
        env.reset()
        rng = np.random.default_rng(0)
        acts = torch.from_numpy(rng.uniform(-1, 1, E)).to(env.device)
        for _ in range(2):
            env.step(acts)
        med, lo, hi = timed(lambda: env.step(acts), a.reps)
        step_ms[E] = med
        print(json.dumps(dict(op="env.step", E=E, ms=round(med, 4), ms_min_max=[round(lo, 4), round(hi, 4)])), flush=True)
        rows.append(dict(op="env.step", E=E, ms=round(med, 4), ms_min_max=[round(lo, 4), round(hi, 4)]))
        maps = env.cost_maps(SCALE, 76, 12, vs=0.3 * SCALE + 1e-8)
        med, lo, hi = timed(lambda: env.cost_maps(SCALE, 76, 12, vs=0.3 * SCALE + 1e-8, out=maps), a.reps)
        rows.append(dict(op="cost_maps", E=E, ms=round(med, 4), ms_min_max=[round(lo, 4), round(hi, 4)]))
        fp = torch.from_numpy(ship_footprint(LATTICE_SHIP_VERTICES, SCALE, 0.25)).to(env.device)
        pose = env.info[:, :3] * torch.tensor([SCALE, SCALE, 1.0], dtype=torch.float64, device=env.device)
        for (_, K, P) in [s for s in SIZES if s[0] == E]:
            kmax = env.max_yaw_rate_step / (SCALE * 0.3)
            paths = arc_paths(pose, torch.linspace(-kmax, kmax, K, dtype=torch.float64, device=env.device), (P - 1) * STEP, STEP)
            assert tuple(paths.shape) == (E, K, P, 3)
            costs = torch.empty((E, K), dtype=torch.float64, device=env.device)
            for masks in (False, True):
                sw = torch.empty((E, K, 380, 60), dtype=torch.uint8, device=env.device) if masks else None
                for outside in ("clip", "reject"):
                    med, lo, hi = timed(lambda: env.swath_costs(paths, fp, maps, outside=outside, return_swaths=masks, out=(costs, sw)), a.reps)
                    row = dict(op="swath_costs", E=E, K=K, P=P, outside=outside, masks=masks, ms=round(med, 4), ms_min_max=[round(lo, 4), round(hi, 4)],
                               us_per_candidate=round(1e3 * med / (E * K), 4), ns_per_sample=round(1e6 * med / (E * K * P), 3),
                               share_of_one_step=round(med / step_ms[E], 4), rejected=int(torch.isinf(costs).sum()) if outside == "reject" else None)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del sw
        env.check_errors()
        env.close()
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, warmup=3, map=[380, 60], footprint_vertices=17, sample_step_cells=STEP, rows=rows)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_swath.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
