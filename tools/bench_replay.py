"""The device replay buffer against a torch-op restatement, and the queue loop with and without it (profiles/replay/README.md).

    python tools/bench_replay.py [--envs 4096] [--rows 1024] [--capacity 10000] [--rounds 50] [--loop-envs 4096] [--loop-batch 1024] [--seconds 3]

Part 1, no env: synthetic recv batches (P = 96) drive ``observe`` + ``record`` and ``sample`` (B = 32 and 256) of a DeviceReplayBuffer, and the same
rules written with torch ops (cumsum for the ranks, index_copy_ into buffers of the same sizes with one spare row for the rows that store nothing,
scatter_reduce for the winner, gather + permute + divide for the sample; no host read either), alternating in one process, timed with events.  For each
kernel path the bytes it must move (every byte once) and that as a fraction of --hbm-gbs.
Part 2: the queue loop of a box-delivery env at the SAM width with uniform position actions, recv / send with reset = done, alternating windows with
and without the buffer attached (tools/bench_async_queue.py's method: fixed calls per window sized in the warm-up, closed handle to closed handle, a
device synchronise at the end); transitions per second.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"


class TorchReplay:
    """The buffer's three rules in torch ops, on tensors of its own (one spare row C / E takes what stores nothing)."""

    def __init__(self, E, P, C, mcol):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)   # noqa: E731
        self.E, self.P, self.C, self.mcol = E, P, C, mcol
        self.state, self.next_state = z((C + 1, P, P, 4), torch.uint8), z((C + 1, P, P, 4), torch.uint8)
        self.action, self.reward, self.ministeps = z(C + 1, torch.int32), z(C + 1, torch.float32), z(C + 1, torch.float32)
        self.nonfinal, self.env = z(C + 1, torch.uint8), z(C + 1, torch.int32)
        self.pend_obs, self.pend_action, self.pend_flags = z((E + 1, P, P, 4), torch.uint8), z(E + 1, torch.int32), z(E + 1, torch.uint8)
        self.hdr = z(4, torch.int64)
        self.g = torch.Generator(device=DEV).manual_seed(0)
        self.d255 = torch.full((), 255.0, device=DEV)

    def observe(self, ids, obs, reward, terminated, truncated, info, slices):
        C, E = self.C, self.E
        valid = ids >= 0
        e = torch.where(valid, ids, torch.full_like(ids, E)).long()
        fl = self.pend_flags[e]
        tr = valid & (slices > 0)
        has = tr & ((fl & 3) == 3)
        rank = torch.cumsum(has.long(), 0) - 1
        total = has.sum()
        keep = has & (total - rank <= C)
        dest = torch.where(keep, (self.hdr[0] + rank) % C, torch.full_like(rank, C))
        self.state.index_copy_(0, dest, self.pend_obs[e])
        self.next_state.index_copy_(0, dest, obs)
        self.action.index_copy_(0, dest, self.pend_action[e])
        self.reward.index_copy_(0, dest, reward.float())
        self.ministeps.index_copy_(0, dest, info[:, self.mcol].float())
        self.nonfinal.index_copy_(0, dest, (terminated == 0).to(torch.uint8))
        self.env.index_copy_(0, dest, ids)
        self.pend_obs.index_copy_(0, e, obs)
        self.pend_flags.index_copy_(0, e, torch.full_like(fl, 5))
        self.hdr[0] += total
        self.hdr[2] += (tr & ~has).sum()

    def record(self, actions, ids, reset):
        E = self.E
        M = ids.shape[0]
        valid = ids >= 0
        e = torch.where(valid, ids, torch.full_like(ids, E)).long()
        j = torch.arange(M, device=DEV)
        win = torch.full((E + 1,), M, dtype=torch.int64, device=DEV).scatter_reduce_(0, e, j, "amin")
        fl = self.pend_flags[e]
        ok = valid & (win[e] == j) & ((fl & 4) != 0)
        dest = torch.where(ok, e, torch.full_like(e, E))
        rs = reset != 0
        self.pend_action.index_copy_(0, torch.where(ok & ~rs, e, torch.full_like(e, E)), actions.to(torch.int32))
        self.pend_flags.index_copy_(0, dest, torch.where(rs, torch.zeros_like(fl), (fl | 2) & 3))
        self.hdr[3] += (valid & ~ok).sum()

    def sample(self, B):
        n = torch.clamp(self.hdr[0], max=self.C)
        idx = (torch.rand(B, device=DEV, generator=self.g) * n).long().clamp_(max=self.C - 1)
        self.hdr[1] += 1
        img = lambda t: (t[idx].permute(0, 3, 1, 2).float() / self.d255).contiguous()   # noqa: E731
        v = (n > 0).to(torch.uint8).expand(B)
        return img(self.state), img(self.next_state), self.action[idx].long(), self.reward[idx], self.ministeps[idx], self.nonfinal[idx], idx.int(), v


def timed(fn, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for n in (3, rounds):       # the first pass warms up
        e0.record()
        for k in range(n):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / rounds     # us per call


def part1(args):
    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    from benchpush_amd.replay import DeviceReplayBuffer
    E, M, C, P = args.envs, args.rows, args.capacity, 96
    R = P * P * 4
    stub = types.SimpleNamespace(cfg=DotDict(agent=DotDict(action_type="position")), action_dim=1, L=_lib.load(), device=torch.device(DEV), num_envs=E,
                                 obs_shape=(P, P, 4))
    buf = DeviceReplayBuffer(stub, C)
    twin = TorchReplay(E, P, C, buf.ministeps_col)
    g = torch.Generator(device=DEV).manual_seed(1)
    feeds = []
    for k in range(4):          # four recv batches of distinct envs, all rows valid, three quarters transitions
        ids = torch.randperm(E, device=DEV, generator=g)[:M].int()
        feeds.append((ids, torch.randint(0, 256, (M, P, P, 4), device=DEV, dtype=torch.uint8, generator=g), torch.randn(M, device=DEV, dtype=torch.float64),
                      (torch.rand(M, device=DEV, generator=g) < 0.1).to(torch.uint8), torch.zeros(M, device=DEV, dtype=torch.uint8),
                      torch.rand((M, 16), device=DEV, dtype=torch.float64, generator=g), torch.randint(0, 4, (M,), device=DEV, generator=g).int()))
    acts = torch.randint(0, P * P, (M,), device=DEV, generator=g).double()
    rst = (torch.rand(M, device=DEV, generator=g) < 0.05).to(torch.uint8)

    def hip_feed(k):
        f = feeds[k % 4]
        buf.observe_rows(*f)
        buf.record(acts, f[0], rst)

    def torch_feed(k):
        f = feeds[k % 4]
        twin.observe(*f)
        twin.record(acts, f[0], rst)

    out = []
    for rep in range(args.repeats):
        for name, fn in (("hip", hip_feed), ("torch", torch_feed)):
            out.append(dict(part="observe+record", impl=name, rows=M, envs=E, repeat=rep, us_per_call=round(timed(fn, args.rounds), 1)))
            print(json.dumps(out[-1]), flush=True)
    st = buf.stats()
    frac = min(1.0, 0.75)       # about three quarters of the rows are transition rows once every env is armed
    feed_bytes = M * R * (2 + 3 * frac)      # per row: obs read + pend_obs write, and for a transition row pend_obs read + state write + next_state write
    for B in (32, 256):
        batch = [None]

        def hip_sample(k, B=B):
            batch[0] = buf.sample(B, out=batch[0])

        def torch_sample(k, B=B):
            twin.sample(B)

        for rep in range(args.repeats):
            for name, fn in (("hip", hip_sample), ("torch", torch_sample)):
                us = timed(fn, args.rounds)
                r = dict(part="sample", impl=name, B=B, repeat=rep, us_per_call=round(us, 1))
                if name == "hip":
                    r["bytes"] = B * R * 2 * 5       # two images: 1 byte read, 4 written per value
                    r["hbm_fraction"] = round(r["bytes"] / (us * 1e-6) / (args.hbm_gbs * 1e9), 4)
                print(json.dumps(r), flush=True)
    hip_us = min(o["us_per_call"] for o in out if o["impl"] == "hip")
    print(json.dumps(dict(part="observe+record", impl="hip", bytes_estimate=int(feed_bytes), hbm_fraction=round(feed_bytes / (hip_us * 1e-6) / (args.hbm_gbs * 1e9), 4),
                          stats=st)), flush=True)


def part2(args):
    from benchpush_amd.baselines.box_delivery.SAM import BoxDeliverySAM
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    from benchpush_amd.replay import DeviceReplayBuffer
    E, M = args.loop_envs, args.loop_batch
    env = BatchedBoxDeliveryEnv(E, cfg=BoxDeliverySAM().sam_cfg(), num_trials=64, device=DEV)
    P = env.obs_shape[0]
    buf = DeviceReplayBuffer(env, args.capacity)
    g = torch.Generator(device=DEV).manual_seed(0)
    count = torch.zeros(E, dtype=torch.int64, device=DEV)

    def window(attached, calls):
        count.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = env.async_queue(M)
        for _ in range(calls):
            ids, obs, rew, term, trunc, info = buf.recv(q) if attached else q.recv()
            count.index_add_(0, ids.clamp(min=0).long(), (q.slices > 0).long())
            a = torch.randint(0, P * P, (M,), device=DEV, generator=g).double()
            (buf.send(q, a, ids, term | trunc) if attached else q.send(a, ids, term | trunc))
        ready = q.close()[5]
        count.add_(ready)
        env.reset()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, int(count.sum().item())

    env.reset()
    calls = {}
    for attached in (False, True):
        window(attached, 16)
        dt, _ = window(attached, 16)
        calls[attached] = max(16, int(round(16 * args.seconds / dt)))
    for rep in range(args.repeats):
        for attached in (False, True):
            dt, n = window(attached, calls[attached])
            print(json.dumps(dict(part="queue loop", buffer=attached, envs=E, batch=M, repeat=rep, calls=calls[attached], seconds=round(dt, 3), transitions=n,
                                  transitions_per_s=round(n / dt, 1))), flush=True)
    env.check_errors()
    print(json.dumps(dict(part="queue loop", buffer_stats=buf.stats())), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--capacity", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth in GB/s the fractions refer to (MI355X: 8 TB/s)")
    ap.add_argument("--loop-envs", type=int, default=4096)
    ap.add_argument("--loop-batch", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    if "1" in args.parts.split(","):
        part1(args)
    if "2" in args.parts.split(","):
        part2(args)


if __name__ == "__main__":
    main()
