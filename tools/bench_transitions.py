"""Times the device transition buffer (benchpush_amd/transitions.py) against the same work in torch ops, in one process.  Needs a GPU; prints one JSON
line per measurement (profiles/transitions/README.md holds a run).

    python tools/bench_transitions.py --envs 4096 --steps 3 --batch 128 --reps 50

Synthetic data at the ship-ice row size (R = 4 x 150 x 150 bytes).  ``add``: one call against a ``torch.where`` over the [E, 4, 150, 150] batch plus the
two row copies and the scalar columns.  ``sample``: one call against ``randint`` + two fancy-index gathers + ``float() / 255`` each, plus the scalar
gathers.  The two versions alternate; times are device events around `reps` calls after a warm-up of every shape.  The bandwidth figures use the
algorithmic byte counts -- add reads and writes 2 E R bytes, sample reads 2 B R and writes 8 B R bytes -- over the call time (the call's launches
together, bookkeeping kernels included), against the 8.0 TB/s HBM3E specification and the 6.3 TB/s a float4 copy reaches.
"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


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


def both(name, lib_fn, torch_fn, reps, nbytes, note=""):
    """Alternates the two versions three times and reports the smallest time of each."""
    lib, ref = [], []
    for _ in range(3):
        lib.append(timed(lib_fn, reps))
        ref.append(timed(torch_fn, reps))
    rate = nbytes / (min(lib) * 1e-3)
    out = {"call": name, "library_ms": round(min(lib), 4), "torch_ms": round(min(ref), 4), "library_runs_ms": [round(v, 4) for v in lib],
           "torch_runs_ms": [round(v, 4) for v in ref], "torch_over_library": round(min(ref) / min(lib), 2), "algorithmic_bytes": nbytes,
           "library_TB_per_s": round(rate / 1e12, 3), "share_of_8.0_TBps_spec": round(rate / HBM_SPEC, 3),
           "share_of_6.3_TBps_copy": round(rate / HBM_COPY, 3), "note": note}
    print(json.dumps(out), flush=True)
    return out


def run(E, T, B, reps, shape):
    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    from benchpush_amd.transitions import DeviceTransitionBuffer
    stub = types.SimpleNamespace(cfg=DotDict(low_dim_state=False), action_dim=1, L=_lib.load(), device=torch.device(DEV), num_envs=E, obs_shape=shape,
                                 obs=torch.zeros(1, dtype=torch.uint8))
    buf = DeviceTransitionBuffer(stub, T * E, seed=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    obs, nxt, term = (torch.randint(0, 256, (E,) + shape, dtype=torch.uint8, device=DEV, generator=g) for _ in range(3))
    action = torch.randn((E, 1), device=DEV, generator=g)
    reward = torch.randn(E, dtype=torch.float64, device=DEV, generator=g)
    done = torch.rand(E, device=DEV, generator=g) < 0.05
    trunc = done & (torch.rand(E, device=DEV, generator=g) < 0.5)
    # the torch learner's storage
    t_obs, t_next = (torch.zeros((T, E) + shape, dtype=torch.uint8, device=DEV) for _ in range(2))
    t_action, t_reward = torch.zeros((T, E, 1), device=DEV), torch.zeros((T, E), device=DEV)
    t_done, t_timeout = (torch.zeros((T, E), dtype=torch.bool, device=DEV) for _ in range(2))
    state = {"t": 0}
    N = T * E
    where_mask = lambda: done.view((E,) + (1,) * len(shape))   # noqa: E731

    def lib_add():
        buf.add(obs, nxt, term, action, reward, done, trunc)

    def torch_add():
        t = state["t"] % T
        t_obs[t].copy_(obs)
        t_next[t].copy_(torch.where(where_mask(), term, nxt))
        t_action[t].copy_(action), t_reward[t].copy_(reward), t_done[t].copy_(done), t_timeout[t].copy_(done & trunc)
        state["t"] += 1

    def lib_sample():
        buf.sample(B)

    def torch_sample():
        idx = torch.randint(0, N, (B,), device=DEV)
        fo, fn_ = t_obs.view((N,) + shape), t_next.view((N,) + shape)
        d = t_done.view(N)[idx].float() * (1.0 - t_timeout.view(N)[idx].float())
        _ = (fo[idx].float() / 255, fn_[idx].float() / 255, t_action.view(N, 1)[idx], t_reward.view(N)[idx], d)

    for _ in range(T):                                             # a full ring for both, so that the samples read all of it
        lib_add(), torch_add()
    row = 1
    for s in shape:
        row *= s
    res = [both("add", lib_add, torch_add, reps, 4 * E * row, "%d envs x %d bytes: 2 E R read, 2 E R written" % (E, row)),
           both("sample", lib_sample, torch_sample, reps, 10 * B * row, "%d rows of %d bytes from %d stored: 2 B R read, 8 B R written" % (B, row, N))]
    torch.cuda.synchronize()
    assert buf.stats()["size"] == N
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3, help="step rows T of the ring")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write all results as one JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transitions needs a GPU: a timing on the host says nothing about the device")
    print(json.dumps({"device": torch.cuda.get_device_name(0), "envs": a.envs, "steps": a.steps, "batch": a.batch, "reps": a.reps}), flush=True)
    res = {"calls": run(a.envs, a.steps, a.batch, a.reps, (4, 150, 150))}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
