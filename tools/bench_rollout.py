"""Times the device rollout buffer (benchpush_amd/rollout.py) against the same work in torch ops, in one process, and the collection loop with and
without the buffer attached.  Needs a GPU; prints one JSON line per measurement (profiles/rollout/README.md holds a run).

    python tools/bench_rollout.py --envs 256 --steps 8 --batch 128 --reps 20 --loop-steps 48

Part 1 uses synthetic data at the ship-ice row size (4 x 150 x 150 bytes): each of begin / truncated_rows / end / finish / one epoch of minibatches, and
what a torch learner would run for the same result (a ``nonzero`` host read for the truncated rows, a [T] loop of tensor ops for GAE, ``randperm`` +
index + divide for the minibatches).  The two versions alternate inside the timed loop's repetitions; times are device events around `reps` calls after
a warm-up of every shape.  Part 2 steps a real ship-ice BatchedVecEnv(to_numpy=False) with random actions and zero values -- no network, so the difference
between the two loops is the buffer's calls and nothing else -- and reports env steps per second of each, alternating twice.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


def timed(fn, reps, warmup=3):
    """Milliseconds per call: device events around `reps` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def both(name, lib_fn, torch_fn, reps, note=""):
    """Alternates the two versions twice and reports the smaller time of each."""
    lib, ref = [], []
    for _ in range(2):
        lib.append(timed(lib_fn, reps))
        ref.append(timed(torch_fn, reps))
    out = {"call": name, "library_ms": round(min(lib), 4), "torch_ms": round(min(ref), 4), "library_runs_ms": [round(v, 4) for v in lib],
           "torch_runs_ms": [round(v, 4) for v in ref], "torch_over_library": round(min(ref) / min(lib), 2), "note": note}
    print(json.dumps(out), flush=True)
    return out


def part1(E, T, B, reps, shape):
    import types

    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    from benchpush_amd.rollout import DeviceRolloutBuffer
    stub = types.SimpleNamespace(cfg=DotDict(low_dim_state=False), action_dim=1, L=_lib.load(), device=torch.device(DEV), num_envs=E, obs_shape=shape,
                                 obs=torch.zeros(1, dtype=torch.uint8))
    gamma, lam = 0.97, 0.95
    buf = DeviceRolloutBuffer(stub, T, gamma, lam, seed=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.randint(0, 256, (E,) + shape, dtype=torch.uint8, device=DEV, generator=g)
    term_obs = torch.randint(0, 256, (E,) + shape, dtype=torch.uint8, device=DEV, generator=g)
    action, value, logp = (torch.randn(s, device=DEV, generator=g) for s in ((E, 1), (E,), (E,)))
    reward = torch.randn(E, dtype=torch.float64, device=DEV, generator=g)
    done = torch.rand(E, device=DEV, generator=g) < 0.05
    trunc = done & (torch.rand(E, device=DEV, generator=g) < 0.5)
    boot = torch.randn(E, device=DEV, generator=g)
    div = torch.full((), 255.0, device=DEV)
    # the torch learner's storage
    t_obs = torch.zeros((T, E) + shape, dtype=torch.uint8, device=DEV)
    t_action = torch.zeros((T, E, 1), device=DEV)
    t_reward, t_value, t_logp, t_adv, t_ret, t_start = (torch.zeros((T, E), device=DEV) for _ in range(6))
    t_last = torch.zeros(E, device=DEV)
    state = {"t": 0, "rows": None, "idx": None}

    def lib_begin():
        buf.t, buf._open = state["t"] % T, False
        buf.begin(obs, action, value, logp)
        state["t"] += 1

    def torch_begin():
        t = state["t"] % T
        t_obs[t].copy_(obs), t_action[t].copy_(action), t_value[t].copy_(value), t_logp[t].copy_(logp), t_start[t].copy_(t_last)
        state["t"] += 1

    def lib_pick():
        buf.truncated_rows(trunc, term_obs)

    def torch_pick():
        idx = torch.nonzero(trunc).squeeze(1)                    # the host read: the number of rows is data
        state["idx"], state["rows"] = idx, term_obs[idx].float() / div

    def lib_end():
        buf.t, buf._open = state["t"] % T, True
        buf.end(reward, done, buf._boot_ids, boot)
        state["t"] += 1

    def torch_end():
        t = state["t"] % T
        t_reward[t].copy_(reward)
        t_reward[t].index_add_(0, state["idx"], gamma * boot[:state["idx"].numel()])
        t_last.copy_(done)
        state["t"] += 1

    def lib_finish():
        buf.t, buf._open = T, False
        buf.finish(value)

    def torch_finish():
        adv = torch.zeros(E, device=DEV)
        for t in reversed(range(T)):
            nn_, nv = (1.0 - t_last, value) if t == T - 1 else (1.0 - t_start[t + 1], t_value[t + 1])
            delta = t_reward[t] + gamma * nv * nn_ - t_value[t]
            adv = delta + gamma * lam * nn_ * adv
            t_adv[t] = adv
        torch.add(t_adv, t_value, out=t_ret)

    def lib_epoch():
        for _ in buf.minibatches(B, state["t"]):
            pass
        state["t"] += 1

    def torch_epoch():
        N = T * E
        perm = torch.randperm(N, device=DEV)
        flat = t_obs.view((N,) + shape)
        for j in range((N + B - 1) // B):
            idx = perm[j * B:(j + 1) * B]
            _ = (flat[idx].float() / div, t_action.view(N, 1)[idx], t_value.view(N)[idx], t_logp.view(N)[idx], t_adv.view(N)[idx], t_ret.view(N)[idx])

    row = int(torch.tensor(shape).prod())
    res = [both("begin", lib_begin, torch_begin, reps, "%d envs x %d bytes stored per call" % (E, row)),
           both("truncated_rows", lib_pick, torch_pick, reps, "K = %d rows written as floats; torch gathers only the %d truncated rows after a host read"
                % (E, int(trunc.sum()))),
           both("end", lib_end, torch_end, reps),
           both("finish", lib_finish, torch_finish, reps, "GAE over [%d, %d]" % (T, E)),
           both("minibatches", lib_epoch, torch_epoch, max(2, reps // 4), "one epoch: %d minibatches of %d" % ((T * E + B - 1) // B, B))]
    return res


def part2(E, steps):
    from benchpush_amd.envs.vec_env import make_ship_ice_vec_env
    from benchpush_amd.rollout import DeviceRolloutBuffer
    venv = make_ship_ice_vec_env(E, cfg={"concentration": 0.3}, to_numpy=False, device=DEV)
    T = 8
    buf = DeviceRolloutBuffer(venv, T, 0.97, 0.95)
    g = torch.Generator(device=DEV).manual_seed(0)
    zeros = torch.zeros(E, device=DEV)
    obs = venv.reset()

    def loop(attached, n):
        nonlocal obs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            actions = torch.rand((E, 1), device=DEV, generator=g) * 2 - 1
            if attached:
                if buf.t == T:
                    buf.finish(zeros)
                    buf.clear()
                buf.begin(obs, actions, zeros, zeros)
            obs, reward, done, infos = venv.step(actions)
            if attached:
                ids, rows = buf.truncated_rows(infos.truncated_mask, infos.terminal_rows)
                buf.end(reward, done, ids, zeros)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    try:
        loop(True, T + 2), loop(False, 4)                          # warm-up of both
        runs = {"attached": [], "bare": []}
        for _ in range(2):
            runs["bare"].append(loop(False, steps))
            runs["attached"].append(loop(True, steps))
        out = {"loop": "ship-ice collection, random actions", "envs": E, "steps": steps,
               "bare_steps_per_s": [round(v, 2) for v in runs["bare"]], "attached_steps_per_s": [round(v, 2) for v in runs["attached"]],
               "bare_env_steps_per_s": round(max(runs["bare"]) * E, 1), "attached_env_steps_per_s": round(max(runs["attached"]) * E, 1),
               "unbootstrapped": buf.stats()["unbootstrapped"]}
        print(json.dumps(out), flush=True)
    finally:
        venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8, help="rollout length T of part 1")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-steps", type=int, default=48, help="env steps per timed loop of part 2 (0: skip)")
    ap.add_argument("--out", default=None, help="also write all results as one JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout needs a GPU: a timing on the host says nothing about the device")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "envs": a.envs, "steps": a.steps, "batch": a.batch, "reps": a.reps}), flush=True)
    res = {"calls": part1(a.envs, a.steps, a.batch, a.reps, (4, 150, 150))}
    if a.loop_steps > 0:
        res["loop"] = part2(a.envs, a.loop_steps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
