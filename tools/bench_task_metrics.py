"""What the on-device episode metrics of box-delivery / area-clearing cost a step: the step() time of a batch of envs, for one library build or for two
builds side by side (same box, same session, fresh processes, alternating -- the method of tools/ab_libs.sh).

  one measurement   python tools/bench_task_metrics.py --task box_delivery --envs 4096 --steps 30 --warmup 5 [--lib PATH.so]
  comparison        python tools/bench_task_metrics.py --ab NEW.so OLD.so --reps 3 --out profiles/task_metrics/ab.json

A measurement prints one JSON line: per-step wall times (host clock around step() between two device synchronisations; the resets of finished envs happen
outside the timed windows), their median, mean and extremes.  The comparison runs every (task, library) pair `reps` times in turn, each in a child process of
its own, and writes all lines plus, per task, the medians of each library and the spread of the repeats of one library -- the yardstick for the difference.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(task, envs, steps, warmup, seed):
    sys.path.insert(0, ROOT)
    import torch
    if task == "box_delivery":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        env = BatchedBoxDeliveryEnv(envs, num_trials=32)
    else:
        from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
        env = BatchedAreaClearingEnv(envs, num_trials=32)
    env.reset()
    gen = torch.Generator().manual_seed(seed)
    times = []
    for t in range(warmup + steps):
        a = (torch.rand(envs * env.action_dim, generator=gen, dtype=torch.float64) * 2 - 1).to(env.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, term, trunc, _ = env.step(a)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if t >= warmup:
            times.append(dt * 1e3)
        done = (term != 0) | (trunc != 0)
        if bool(done.any()):
            env.reset(done)
    env.check_errors()
    has_metrics = hasattr(env.L, "bp_task_metric_row")
    finished = int(env.episode_metrics()[1].sum().item()) if has_metrics else None
    env.close()
    return {"task": task, "envs": envs, "steps": steps, "warmup": warmup, "lib": os.path.basename(os.environ.get("BP_PROF_LIB", "default")), "episode_metrics": has_metrics,
            "episodes_finished": finished, "ms_per_step_median": statistics.median(times), "ms_per_step_mean": statistics.fmean(times),
            "ms_per_step_min": min(times), "ms_per_step_max": max(times), "ms": [round(v, 3) for v in times]}


def compare(libs, args):
    runs = []
    for task in ("box_delivery", "area_clearing"):
        for rep in range(args.reps):
            for lib in libs:
                env = dict(os.environ, BP_PROF="1", BP_PROF_LIB=os.path.abspath(lib))
                cmd = [sys.executable, os.path.abspath(__file__), "--task", task, "--envs", str(args.envs), "--steps", str(args.steps), "--warmup",
                       str(args.warmup), "--seed", str(args.seed)]
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:          # a child that failed ends the comparison: nothing more is started on the device
                    sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                    raise SystemExit("child failed (%d): %s %s" % (out.returncode, task, lib))
                r = json.loads(out.stdout.strip().splitlines()[-1])
                r["rep"] = rep
                runs.append(r)
                print(task, os.path.basename(lib), "rep", rep, "median %.3f ms/step" % r["ms_per_step_median"], flush=True)
                if args.out:
                    with open(args.out, "w") as f:
                        json.dump({"runs": runs}, f, indent=1)
    summary = {}
    for task in ("box_delivery", "area_clearing"):
        per = {os.path.basename(lib): [r["ms_per_step_median"] for r in runs if r["task"] == task and r["lib"] == os.path.basename(lib)] for lib in libs}
        summary[task] = {k: {"medians_ms": v, "median_of_medians_ms": statistics.median(v), "spread_ms": max(v) - min(v)} for k, v in per.items()}
    res = {"summary": summary, "runs": runs}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(summary))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=["box_delivery", "area_clearing"], default="box_delivery")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lib", default=None, help="library build to load instead of the package's own")
    ap.add_argument("--ab", nargs="+", default=None, help="library builds to compare")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.ab:
        return compare(args.ab, args)
    if args.lib:
        os.environ["BP_PROF"], os.environ["BP_PROF_LIB"] = "1", os.path.abspath(args.lib)
    print(json.dumps(measure(args.task, args.envs, args.steps, args.warmup, args.seed)))


if __name__ == "__main__":
    main()
