"""Asynchronous step against the lock-step step() of the same build, alternating in one process (profiles/async/README.md).

    python tools/bench_async.py --env box  [--envs 4096] [--seconds 4] [--repeats 3] [--budgets 500,1000,2000,3000]
    python tools/bench_async.py --env area

The workloads are those of ``bench.py --env box`` (box-delivery-v0, small_empty, 12 boxes, heading actions ~ U(-1, 1), auto-reset) and ``--env area``.
Every window runs a fixed number of calls (sized in the warm-up to last about --seconds), ends in a device synchronise and reports emitted transitions per
second; an asynchronous window ends with drain(), whose transitions and time count.  Per window: minimum / median / maximum transitions per env -- the
asynchronous step samples short env steps more often than long ones, so envs advance at different rates.  One JSON line per window, then a Markdown table.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="box", choices=["box", "area"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budgets", default="500,1000,2000,3000")
    ap.add_argument("--warmup", type=int, default=3, help="lock-step env steps before anything is timed")
    args = ap.parse_args()
    E = args.envs
    dev = "cuda:0"
    if args.env == "box":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        env = BatchedBoxDeliveryEnv(E, cfg={"boxes": {"num_boxes_small": 12}}, num_trials=64, device=dev)
    else:
        from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
        env = BatchedAreaClearingEnv(E, num_trials=64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    table = (torch.rand((512, E), generator=g, device=dev, dtype=torch.float64) * 2 - 1).float().double()
    count = torch.zeros(E, dtype=torch.int64, device=dev)
    tick = [0]

    def done_mask(term, trunc):
        return (term | trunc) if args.env == "area" else term

    def lock_call():
        obs, rew, term, trunc, info = env.step(table[tick[0] % 512])
        tick[0] += 1
        count.add_(1)
        env.reset(done_mask(term, trunc))

    def async_call(budget):
        obs, rew, term, trunc, info, ready = env.step_async(table[tick[0] % 512], budget)
        tick[0] += 1
        count.add_(ready)
        env.reset(ready & done_mask(term, trunc))

    def window(calls, budget):
        """`calls` calls of one mode, from and to a closed handle; returns (seconds, per-env transition counts)."""
        count.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            if budget is None:
                lock_call()
            else:
                async_call(budget)
        if budget is not None:
            obs, rew, term, trunc, info, ready = env.drain()
            count.add_(ready)
            env.reset(ready & done_mask(term, trunc))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, count.cpu()

    env.reset()
    for _ in range(args.warmup):
        lock_call()
    budgets = [int(b) for b in args.budgets.split(",") if b]
    modes = [None] + budgets
    calls = {}
    for m in modes:   # warm-up of each mode, and the size of its windows
        n0 = 4 if m is None else 16
        dt, _ = window(n0, m)
        calls[m] = max(n0, int(round(n0 * args.seconds / dt)))
    rows = {m: [] for m in modes}
    for rep in range(args.repeats):
        for m in modes:   # alternating: lock-step, then every budget, then lock-step again ...
            dt, c = window(calls[m], m)
            r = dict(env=args.env, envs=E, mode="step" if m is None else "step_async", budget=m, repeat=rep, calls=calls[m], seconds=round(dt, 4),
                     transitions=int(c.sum()), transitions_per_s=round(float(c.sum()) / dt, 1), per_env_min=int(c.min()), per_env_median=float(c.double().median()),
                     per_env_max=int(c.max()))
            rows[m].append(r)
            print(json.dumps(r), flush=True)
    env.check_errors()
    env.close()
    print("\n| mode | budget | transitions/s per window | min | median | max | transitions per env (min / median / max) |\n|---|---|---|---|---|---|---|")
    for m in modes:
        v = sorted(r["transitions_per_s"] for r in rows[m])
        last = rows[m][-1]
        print("| %s | %s | %s | %.0f | %.0f | %.0f | %d / %.0f / %d |" % (
            "step()" if m is None else "step_async", "-" if m is None else m, ", ".join("%.0f" % r["transitions_per_s"] for r in rows[m]), v[0], v[len(v) // 2], v[-1],
            last["per_env_min"], last["per_env_median"], last["per_env_max"]))


if __name__ == "__main__":
    main()
