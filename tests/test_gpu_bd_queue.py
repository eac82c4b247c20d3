"""Ready queue of the asynchronous step (env.async_queue: recv / send batches of fixed size, the queue on the device): the transitions are step()'s, the order
is the model's (tests/async_queue_ref.py), bit for bit and id for id."""
import math

import numpy as np
import pytest
import torch

from async_queue_ref import BUSY, QueueModel
from test_gpu_bd_async import SharedOracle, _setup

pytestmark = pytest.mark.gpu

BOXES = 4   # info column "cumulative_boxes" (box-delivery)


class Streams:
    """Per-env action streams keyed by (env, k-th accepted action): the seeds and the forced first actions of the existing asynchronous tests."""

    def __init__(self, E, seed, first=None):
        self.rng = [np.random.RandomState(seed + e) for e in range(E)]
        self.first = {e: list(a) for e, a in (first or {}).items()}
        self.seq = [[] for _ in range(E)]

    def get(self, e, k):
        while len(self.seq[e]) <= k:
            self.seq[e].append(np.float64(self.first[e].pop(0)) if self.first.get(e) else self.rng[e].uniform(-1, 1, ()))
        return self.seq[e][k]


def _rows(env):
    return [t.clone() for t in (env.obs, env.reward, env.terminated, env.truncated, env.info)]


def run_twin(env, streams, N):
    """Lock-step reference: step() with the k-th action of every env, reset(mask) of the done envs (not after the last step).  log[e] is the env's sequence
    of ("fresh", obs, info) and ("trans", obs, reward, terminated, truncated, info) entries."""
    E = env.num_envs
    obs, info = env.reset()
    torch.cuda.synchronize()
    o, i = obs.cpu().numpy(), info.cpu().numpy()
    log = [[("fresh", o[e].copy(), i[e].copy())] for e in range(E)]
    for k in range(N):
        a = np.array([streams.get(e, k) for e in range(E)])
        env.step(torch.from_numpy(a))
        torch.cuda.synchronize()
        o, r, t, tr, i = [x.cpu().numpy() for x in _rows(env)]
        for e in range(E):
            log[e].append(("trans", o[e].copy(), r[e], t[e], tr[e], i[e].copy()))
        done = (t | tr).astype(bool)
        if done.any() and k < N - 1:
            env.reset(torch.from_numpy(done.astype(np.uint8)))
            torch.cuda.synchronize()
            o, i = env.obs.cpu().numpy(), env.info.cpu().numpy()
            for e in np.nonzero(done)[0]:
                log[e].append(("fresh", o[e].copy(), i[e].copy()))
    return log


def run_queue(env, streams, M, budget, N, cap):
    """The same streams through the queue: reset = terminated | truncated in every send, an env that has delivered N transitions is not sent any more (it stays
    taken).  Every recv is compared with the model (ids, count, counts); returns (log, seen, model, queue)."""
    E = env.num_envs
    env.reset()
    q = env.async_queue(M, budget)
    model = QueueModel(E, M)
    log = [[] for _ in range(E)]
    ntrans, nacc = [0] * E, [0] * E
    seen = dict(partial=0, delivered=0, resets=0, max_slices=0, recvs=0, rows=0)
    while min(ntrans) < N:
        assert seen["recvs"] < cap, ("an env never delivered its transitions", ntrans)
        ids, obs, rew, term, trunc, info = q.recv()
        torch.cuda.synchronize()
        seen["recvs"] += 1
        emitted = np.nonzero(q.emitted.cpu().numpy())[0].tolist()
        mids, n, mcounts = model.recv(emitted)
        model.check()
        assert ids.cpu().tolist() == mids, ("ids", seen["recvs"], ids.cpu().tolist(), mids)
        assert q.counts.cpu().tolist() == mcounts, ("counts", seen["recvs"], q.counts.cpu().tolist(), mcounts)
        assert mcounts[1] + mcounts[2] + mcounts[3] == E
        seen["partial"] += int(0 < n < M)
        seen["rows"] += n
        o, r, t, tr, i, sl = [x.cpu().numpy() for x in (obs, rew, term, trunc, info, q.slices)]
        assert not o[n:].any() and not r[n:].any() and not t[n:].any() and not tr[n:].any() and not i[n:].any() and not sl[n:].any()
        act = np.full(M, np.nan)          # rows without an action hold NaN: reset rows, unused rows and the rows of envs that have finished
        sid, rst = [-1] * M, [0] * M
        for j in range(n):
            e = mids[j]
            if sl[j] == 0:
                assert r[j] == 0 and t[j] == 0 and tr[j] == 0, "a fresh row carries no transition"
                log[e].append(("fresh", o[j].copy(), i[j].copy()))
            else:
                log[e].append(("trans", o[j].copy(), r[j], t[j], tr[j], i[j].copy()))
                ntrans[e] += 1
                seen["max_slices"] = max(seen["max_slices"], int(sl[j]))
                seen["delivered"] = max(seen["delivered"], int(i[j][BOXES]))
            if ntrans[e] >= N:
                continue
            sid[j] = e
            if t[j] or tr[j]:
                rst[j] = 1
                seen["resets"] += 1
            else:
                act[j] = streams.get(e, nacc[e])
                nacc[e] += 1
        dv = env.device
        q.send(torch.from_numpy(act).to(dv), torch.tensor(sid, dtype=torch.int32, device=dv), torch.tensor(rst, dtype=torch.uint8, device=dv))
        model.send(sid, rst)
        model.check()
    torch.cuda.synchronize()
    return log, seen, model, q


def same_logs(a, b, what):
    for e, (la, lb) in enumerate(zip(a, b)):
        assert [x[0] for x in la] == [x[0] for x in lb], (what, "env", e, [x[0] for x in la], [x[0] for x in lb])
        for k, (x, y) in enumerate(zip(la, lb)):
            for u, v in zip(x[1:], y[1:]):
                assert np.array_equal(u, v), (what, "env", e, "entry", k, x[0])


_RUN1 = {}


def _run1():
    """The run of tests 1 and 2, made once: E = 5, M = 2, budget 120, 12 transitions per env, and its lock-step twin."""
    if not _RUN1:
        N, E, M, budget = 12, 5, 2, 120
        first = {0: [1.0, 1.0, 1.0, 1.0]}
        env, cfg, trials = _setup(E=E)
        cap = N * (math.ceil(2 * 901 / budget) + math.ceil(E / M)) + 5
        assert cap == 233
        log, seen, model, q = run_queue(env, Streams(E, 1000, first), M, budget, N, cap)
        q.close()
        env.check_errors()
        env.close()
        twin, _, _ = _setup(E=E)
        tlog = run_twin(twin, Streams(E, 1000, first), N)
        twin.check_errors()
        twin.close()
        _RUN1.update(log=log, seen=seen, model=model, tlog=tlog, cfg=cfg, trials=trials, N=N, E=E)
    return _RUN1


def test_queue_transitions_are_step_transitions():
    """E = 5, M = 2, budget 120 on the scene of the asynchronous tests until every env has delivered 12 transitions (at most 12 * (16 + 3) + 5 = 233 recvs): the
    per-env sequences of transitions and fresh rows equal those of a lock-step twin driven with step() / reset(mask); the first 6 transitions of every env
    also equal the oracle's.  The run holds a partly filled batch, a ring wrap, a delivery, a reset row and a transition of three calls or more."""
    from oracle.oracle_bd import BD_INFO_KEYS
    from test_gpu_bd import _oracle
    R = _run1()
    same_logs(R["log"], R["tlog"], "queue vs lock-step twin")
    s = R["seen"]
    assert s["partial"] >= 1 and R["model"].wraps >= 1 and s["delivered"] >= 1 and s["resets"] >= 1 and s["max_slices"] >= 3, (s, R["model"].wraps)
    streams = Streams(R["E"], 1000, {0: [1.0, 1.0, 1.0, 1.0]})
    cfg, trials = R["cfg"], R["trials"]
    for e in range(R["E"]):
        o = SharedOracle(("bd", e), lambda: _oracle(cfg, trials[e % len(trials)], step_limit=900))
        entries = iter(R["log"][e])
        kind, obs, _ = next(entries)
        assert kind == "fresh" and np.array_equal(obs, o.observe())
        k = episode = 0
        while k < 6:
            ent = next(entries)
            if ent[0] == "fresh":
                episode += 1
                assert np.array_equal(ent[1], o.reset(trials[(e + episode) % len(trials)])), ("reset obs", e, k)
                continue
            oo, orr, ot, otr, oi = o.step(streams.get(e, k))
            assert np.array_equal(ent[1], oo) and ent[2] == orr and bool(ent[3]) == ot and bool(ent[4]) == otr, ("oracle", e, k)
            assert np.array_equal(ent[5], np.array([oi[n] for n in BD_INFO_KEYS])), ("oracle info", e, k)
            k += 1


def test_queue_order_is_the_models():
    """Every recv of that run returned the model's ids, count and counts (asserted recv by recv inside the run); here: the run fed the model every emitted mask
    and every send, no send row was rejected, and the rows delivered add up."""
    R = _run1()
    s, m = R["seen"], R["model"]
    assert m.rejected == 0 and s["recvs"] >= 12
    assert s["rows"] == sum(len(l) for l in R["log"]) and all(sum(x[0] == "trans" for x in l) == R["N"] for l in R["log"])


def test_queue_gather_and_scan_across_wave_and_workgroup_boundaries():
    """E = 1030 (past one 1024-thread pass of the scan, not a multiple of 64), M = 130, budget 200, random actions: after each recv the dense rows equal the envs'
    own rows at the returned ids (a fresh row: reward 0, flags 0), rows beyond the count are zero with id -1, ids and counts equal the model's and the counts
    add up to E.  Six rounds deliver fresh rows only (the ring holds 1030 of them first); four more rounds reach the transitions behind them."""
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    E, M = 1030, 130
    env = BatchedBoxDeliveryEnv(E, num_trials=2)
    env.reset()
    q = env.async_queue(M, 200)
    model = QueueModel(E, M)
    rng = np.random.RandomState(5)
    trans_rows = 0
    for rnd in range(10):
        ids, obs, rew, term, trunc, info = q.recv()
        torch.cuda.synchronize()
        mids, n, mcounts = model.recv(np.nonzero(q.emitted.cpu().numpy())[0].tolist())
        assert ids.cpu().tolist() == mids, rnd
        assert q.counts.cpu().tolist() == mcounts and mcounts[1] + mcounts[2] + mcounts[3] == E, (rnd, q.counts.cpu().tolist(), mcounts)
        idx = ids[:n].long()
        fresh = q.slices[:n] == 0
        assert torch.equal(obs[:n], env.obs[idx]) and torch.equal(info[:n], env.info[idx]), rnd
        for dense, rows in ((rew, env.reward), (term, env.terminated), (trunc, env.truncated), (q.slices, env.slices)):
            assert torch.equal(dense[:n][~fresh], rows[idx][~fresh]) and not dense[:n][fresh].any(), rnd
        assert (ids[n:] == -1).all() and not obs[n:].any() and not rew[n:].any() and not term[n:].any() and not trunc[n:].any() and not info[n:].any()
        assert not q.slices[n:].any()
        trans_rows += int((~fresh).sum())
        reset = term | trunc
        q.send(torch.from_numpy(rng.uniform(-1, 1, M)).to(env.device), ids, reset)
        model.send(mids, reset.cpu().tolist())
        model.check()
        if rnd == 5:
            assert trans_rows == 0   # (the six rounds of fresh rows)
    assert trans_rows >= 1 and model.rejected == 0
    torch.cuda.synchronize()
    q.close()
    env.check_errors()
    env.close()


def _open4(M=4):
    env, cfg, trials = _setup()
    env.reset()
    q = env.async_queue(M, 40)
    model = QueueModel(4, M)
    return env, q, model


def _recv(q, model):
    ids = q.recv()[0]
    torch.cuda.synchronize()
    mids, n, mcounts = model.recv(np.nonzero(q.emitted.cpu().numpy())[0].tolist())
    assert ids.cpu().tolist() == mids and q.counts.cpu().tolist() == mcounts, (ids.cpu().tolist(), mids, q.counts.cpu().tolist(), mcounts)
    return mids


def _send(env, q, model, ids, actions, reset=None):
    dv = env.device
    q.send(torch.tensor(actions, dtype=torch.float64, device=dv), torch.tensor(ids, dtype=torch.int32, device=dv),
           None if reset is None else torch.tensor(reset, dtype=torch.uint8, device=dv))
    return model.send(ids, reset)


def test_queue_send_guards():
    """E = 4, M = 4.  Rejected rows: a duplicate id, the id of a busy env, an id that was queued again and not taken since, id 7 (out of range); a row with id -1
    and a NaN action is ignored.  Four rows cannot hold an accepted row and all of these (the duplicate alone needs two), so they come in two consecutive
    sends with nothing in between.  `rejected` rises by exactly the model's number, the accepted row starts its env, the envs' rows and bodies stay bit-equal,
    check_errors() stays clean."""
    env, q, model = _open4()
    nan = float("nan")
    assert _recv(q, model) == [0, 1, 2, 3]
    _send(env, q, model, [0, 1, -1, -1], [0.3, -0.4, nan, nan])             # envs 0 and 1 get actions
    assert _recv(q, model) == [-1, -1, -1, -1]                              # 40 sim steps: both are busy, nothing emitted, nothing queued
    assert [model.state[e] == BUSY for e in range(4)] == [True, True, False, False]
    _send(env, q, model, [3, -1, -1, -1], [nan] * 4, [1, 0, 0, 0])          # env 3 is reset and queued again: in the ring, not taken
    torch.cuda.synchronize()
    before = _rows(env) + [env.body_state().clone()]
    r0 = model.rejected
    acts, _ = _send(env, q, model, [2, 2, 0, -1], [0.5, 0.9, 0.1, nan])     # accepted / duplicate / busy / ignored
    assert acts == [(0, 2)] and model.rejected == r0 + 2
    acts, _ = _send(env, q, model, [3, 7, 1, -1], [0.2, 0.2, 0.2, nan], [0, 1, 1, 0])   # queued and not taken / out of range / busy (reset rows too) / ignored
    assert not acts and model.rejected == r0 + 5
    torch.cuda.synchronize()
    for b, a in zip(before, _rows(env) + [env.body_state().clone()]):
        assert torch.equal(b, a)
    # the next recv starts env 2 and delivers env 3's fresh row first; busy count and rejected count are the model's (checked in _recv), and in the model
    # env 2 has started: had the device not started it, its busy count would be one short
    assert _recv(q, model)[0] == 3 and model.state[2] != "idle"
    c = q.counts.cpu().tolist()
    assert c[2] == sum(s == BUSY for s in model.state) and c[4] == r0 + 5
    assert q.stats()["rejected"] == r0 + 5
    q.close()
    env.check_errors()
    env.close()


def test_queue_refusals_and_close():
    """With a queue open step, step_async, drain, reset(mask), save_state, restore_state and clone_envs raise BpError and change nothing; close() finishes exactly
    the busy envs; afterwards step() continues the twin's sequence; a reset() of all envs closes the queue too; batch sizes 0 and E + 1, a damping config and a
    ship-ice handle are refused."""
    from benchpush_amd import _lib
    from benchpush_amd._lib import BpError
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    a0, a1 = np.array([0.3, -0.6, 0.8, 0.1]), np.array([-0.2, 0.5, 0.4, 0.1])
    twin, _, _ = _setup()
    twin.reset()
    twin.step(torch.from_numpy(a0))
    t1 = _rows(twin)
    twin.step(torch.from_numpy(a1))
    t2 = _rows(twin)
    torch.cuda.synchronize()
    twin.close()

    env, _, _ = _setup()
    env.reset()
    saved = env.save_state()
    for bad in (0, 5):
        with pytest.raises(BpError):
            env.async_queue(bad)
        assert not env.async_open
    q = env.async_queue(4, 40)
    model = QueueModel(4, 4)
    assert env.async_open and q.is_open
    with pytest.raises(BpError):
        env.async_queue(2)          # one queue at a time
    assert _recv(q, model) == [0, 1, 2, 3]
    _send(env, q, model, [0, 1, 2, -1], [a0[0], a0[1], a0[2], float("nan")])   # env 3 stays taken
    assert _recv(q, model) == [-1] * 4
    before = _rows(env) + [env.slices.clone(), env.body_state().clone()]
    z = torch.zeros(4, dtype=torch.float64)
    for call in (lambda: env.step(z), lambda: env.step_async(z, 100), lambda: env.drain(), lambda: env.reset(torch.tensor([0, 1, 0, 0], dtype=torch.uint8)),
                 lambda: env.save_state(), lambda: env.restore_state(saved), lambda: env.clone_envs([0], [1])):
        with pytest.raises(BpError):
            call()
    torch.cuda.synchronize()
    for b, a in zip(before, _rows(env) + [env.slices.clone(), env.body_state().clone()]):
        assert torch.equal(b, a)
    assert q.is_open
    ready = q.close()[5]
    torch.cuda.synchronize()
    busy = model.close()
    assert busy == [0, 1, 2] and np.nonzero(ready.cpu().numpy())[0].tolist() == busy
    assert not env.async_open and not q.is_open
    for x, y in zip(_rows(env), t1):
        assert torch.equal(x[:3], y[:3])
    with pytest.raises(BpError):
        q.recv()
    env.step(torch.from_numpy(np.array([a1[0], a1[1], a1[2], a0[3]])))   # envs 0-2 take their second action, env 3 its first
    torch.cuda.synchronize()
    for x, y1, y2 in zip(_rows(env), t1, t2):
        assert torch.equal(x[:3], y2[:3]) and torch.equal(x[3], y1[3])
    env.save_state()
    # a reset of all envs closes the queue without a drain
    q = env.async_queue(2)
    q.recv()
    assert env.async_open and q.is_open
    env.reset()
    assert not env.async_open and not q.is_open
    env.step(z)
    env.check_errors()
    env.close()
    damp = BatchedBoxDeliveryEnv(2, cfg={"sim": {"damping": 0.8}}, num_trials=2)
    damp.reset()
    with pytest.raises(BpError):
        damp.async_queue(2)
    assert not damp.async_open
    damp.close()
    ship = BatchedShipIceEnv(2, cfg={"concentration": 0.3}, trials=default_trials(0.3, 2, base_seed=7))
    ship.reset()
    assert ship.L.bp_bd_queue_open(ship.h, 1, ship._stream()) == -1 and ship.L.bp_bd_queue_batch(ship.h) == 0
    assert _lib.ERRORS[-1] == "BP_EINVAL"
    ship.step(torch.zeros(2, dtype=torch.float64))
    ship.close()


def test_queue_python_layer_does_not_synchronise():
    """recv(block=False) and send run under torch's sync debug mode "error" without raising (the torch side; the library enqueues kernels only).  Wrong shapes,
    dtypes and devices raise ValueError."""
    env, q, model = _open4(M=3)
    dv = env.device
    acts = torch.zeros(3, dtype=torch.float64, device=dv)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            ids, obs, rew, term, trunc, info = q.recv(block=False)
            q.send(acts, ids, term | trunc)
            q.send(acts, ids)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    ids = q.ids
    for bad in (lambda: q.send(acts[:2], ids), lambda: q.send(acts.long(), ids), lambda: q.send(acts.cpu(), ids), lambda: q.send(acts, ids.long()),
                lambda: q.send(acts, ids[:2]), lambda: q.send(acts, ids, torch.zeros(3, dtype=torch.float32, device=dv)),
                lambda: q.send(acts, ids, torch.zeros(2, dtype=torch.uint8, device=dv)), lambda: q.send([0.0] * 3, ids)):
        with pytest.raises(ValueError):
            bad()
    # block=True: a full batch, or nothing is busy any more
    ids = q.recv(block=True)[0]
    c = q.counts.cpu().tolist()
    assert c[0] == 3 or c[2] == 0
    st = q.stats()
    assert st["calls"] >= 4 and st["rejected"] == c[4] and 0.0 <= st["mean_fill"] <= 1.0
    q.close()
    env.check_errors()
    env.close()


def test_queue_area_clearing():
    """area-clearing-v0, E = 4, M = 3, budget 700, 8 transitions per env: the per-env sequences equal those of the lock-step twin, and so do the rows of
    episode_metrics() (the episodes closed by the reset rows of the sends / by reset(mask))."""
    from benchpush_amd import area_clearing_scenario as A
    from benchpush_amd.config import default_cfg
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    N, E, M, budget, step_limit = 8, 4, 3, 700, 600
    cfg = default_cfg("area_clearing")
    cfg.env = "clear_env"
    cfg.agent.action_type = "heading"
    cfg.sim.t_max = 7
    trials = A.generate_trials(cfg, 4)
    mk = lambda: BatchedAreaClearingEnv(E, cfg={"env": "clear_env", "agent": {"action_type": "heading"}, "sim": {"t_max": 7}}, trials=trials,   # noqa: E731
                                        bd_overrides={"step_limit": step_limit})
    env = mk()
    cap = N * (math.ceil(2 * (step_limit + 1) / budget) + math.ceil(E / M)) + 5
    log, seen, model, q = run_queue(env, Streams(E, 2000), M, budget, N, cap)
    q.close()
    rows, cnt = env.episode_metrics()
    env.check_errors()
    twin = mk()
    tlog = run_twin(twin, Streams(E, 2000), N)
    trows, tcnt = twin.episode_metrics()
    torch.cuda.synchronize()
    same_logs(log, tlog, "area-clearing queue vs twin")
    assert seen["resets"] >= 1 and int(cnt.sum()) >= 1
    assert torch.equal(cnt, tcnt) and torch.equal(rows.view(torch.int64), trows.view(torch.int64))
    env.close()
    twin.close()
