"""Cost of one lattice_search call (k_lattice_search) over a batch, in ONE process: device-event time per call, 2 warm-up calls and `--reps` timed
ones, ship-ice at 30 % concentration, the envs' own 380 x 60 cost maps (horizon 30 m), the reference's shipped configuration (8 headings, scale 5,
turning radius 2 lattice units, 17-vertex padded footprint, goal line 30 m = 150 rows ahead of each ship, weight 1).  Recorded next to it: the time of the mask generation
(lattice_swath_masks), of one env.step and of cost_maps, the expansions / nodes / queue entries per env (mean, p99, max -- the node and queue figures
come from the restatement on `--cpu-envs` envs), the workspace bytes, and the restatement's wall time for one env on the CPU.  Run it under a time limit:

    timeout 900 python tools/bench_lattice.py [--envs 4096] [--reps 10] [--out profiles/lattice]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "examples")]

SCALE, HORIZON_M = 5, 30


def timed(fn, reps, warmup=2):
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


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(mean=round(float(v.mean()), 1), p99=float(np.percentile(v, 99)), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-envs", type=int, default=8)
    ap.add_argument("--max-expansions", type=int, default=None)
    ap.add_argument("--out", default="profiles/lattice")
    a = ap.parse_args()
    import lattice_ref as LR
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from benchpush_amd.planning import LATTICE_SHIP_VERTICES, lattice_max_val, lattice_swath_masks, ship_footprint
    from lattice_planner import load_control_set
    E = a.envs
    env = BatchedShipIceEnv(E, cfg={"concentration": 0.3}, num_trials=100)
    env.reset()
    acts = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, E)).to(env.device)
    for _ in range(3):
        env.step(acts)
    res = dict(device=torch.cuda.get_device_name(0), E=E, reps=a.reps, map=[380, 60], headings=8, horizon_m=HORIZON_M)
    res["env_step_ms"] = timed(lambda: env.step(acts), a.reps)
    prims = load_control_set()
    fp = ship_footprint(LATTICE_SHIP_VERTICES, SCALE, 0.25)
    pose = (env.info[:, :3] * torch.tensor([SCALE, SCALE, 1.0], dtype=torch.float64, device=env.device)).contiguous()
    half = float(fp[:, 0].max() - fp[:, 0].min()) / 2
    mk = lambda: env.cost_maps(SCALE, 76, 12, horizon=HORIZON_M, ship_pos_y=pose[:, 1] - half, vs=0.3 * SCALE + 1e-8)   # noqa: E731
    maps = mk()
    res["cost_maps_ms"] = timed(mk, a.reps)
    res["masks_ms"] = timed(lambda: lattice_swath_masks(env, prims, fp, pose[:, 2]), max(2, a.reps // 3))
    masks = lattice_swath_masks(env, prims, fp, pose[:, 2])
    goal_y = (pose[:, 1] + HORIZON_M * SCALE).contiguous()      # the goal line a full horizon ahead of every ship (the map has 380 rows)
    kw = {} if a.max_expansions is None else {"max_expansions": a.max_expansions}
    out = env.lattice_search(maps, pose, goal_y, prims, masks, **kw)
    res["search_ms"] = timed(lambda: env.lattice_search(maps, pose, goal_y, prims, masks, out=out, **kw), a.reps)
    torch.cuda.synchronize()
    st = out.status.cpu().numpy()
    res["status_counts"] = {k: int((st == v).sum()) for k, v in (("found", 0), ("no_path", 1), ("cap", 2))}
    res["expanded"] = stats(out.expanded.cpu().numpy())
    res["path_nodes"] = stats(out.n_nodes.cpu().numpy())
    res["workspace_bytes"] = int(env._lattice_ws.numel())
    res["workspace_bytes_per_env"] = res["workspace_bytes"] // E
    T = LR.tables_from_prims(prims, lattice_max_val(prims, fp))
    n = min(a.cpu_envs, E)
    mp, ps, gy, mm = maps[:n].cpu().numpy(), pose[:n].cpu().numpy(), goal_y[:n].cpu().numpy(), masks[:n].cpu().numpy()
    walls, tables, queues = [], [], []
    for e in range(n):
        t0 = time.perf_counter()
        r = LR.lattice_search(mp[e], ps[e], gy[e], T, mm[e], margin=25)
        walls.append(time.perf_counter() - t0)
        tables.append(r.n_table)
        queues.append(r.max_queue)
        assert r.status == st[e] and (r.status != 0 or (r.g == float(out.g[e]) and r.expanded == int(out.expanded[e])))
    res["restatement_cpu_s_per_env"] = dict(mean=round(float(np.mean(walls)), 3), max=round(float(np.max(walls)), 3), envs=n)
    res["restatement_nodes_seen"], res["restatement_max_queue"] = stats(tables), stats(queues)
    env.check_errors()
    env.close()
    print(json.dumps(res))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_lattice.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
