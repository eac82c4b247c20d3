"""Device replay buffer on the ready queue (benchpush_amd/replay.py, csrc/bp_replay.hpp): every tensor of the buffer equals the numpy model's
(tests/replay_ref.py) with == after every call, on synthetic feeds that cross the scan's wave and workgroup boundaries and wrap the ring, and on the
real queue of both tasks."""
import types

import numpy as np
import pytest
import torch

from replay_ref import AWAITS, ReplayModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stub_env(E, P, action_type="position"):
    """What DeviceReplayBuffer reads of an env, without one."""
    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    return types.SimpleNamespace(cfg=DotDict(agent=DotDict(action_type=action_type)), action_dim=2 if action_type == "velocity" else 1, L=_lib.load(),
                                 device=torch.device(DEV), num_envs=E, obs_shape=(P, P, 4))


def _pair(E, P, C, seed=0):
    from benchpush_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(_stub_env(E, P), C, seed=seed)
    return buf, ReplayModel(C, E, (P, P, 4), buf.ministeps_col, seed=seed)


def _same(buf, model, what):
    torch.cuda.synchronize()
    for n in ReplayModel.TENSORS:
        got, want = getattr(buf, n).cpu().numpy(), getattr(model, n)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, n)
        assert np.array_equal(got, want), (what, n, np.argwhere(got != want)[:4].tolist())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _observe_rows(rng, model, M, k):
    """One recv's worth of rows: k distinct envs at random rows (the others -1 and zero), about a quarter fresh, flags in all four combinations."""
    E, shape = model.E, model.obs_shape
    ids = np.full(M, -1, np.int32)
    rows = np.sort(rng.permutation(M)[:k])
    ids[rows] = rng.permutation(E)[:k]
    live = ids >= 0
    slices = np.where(live, rng.randint(0, 4, M), 0).astype(np.int32)
    obs = rng.randint(0, 256, (M,) + shape, dtype=np.uint8) * live.reshape(-1, 1, 1, 1).astype(np.uint8)
    reward = rng.randn(M) * live
    term = ((rng.rand(M) < 0.35) & live).astype(np.uint8)
    trunc = (np.where(rng.rand(M) < 0.5, term, rng.rand(M) < 0.2) & live).astype(np.uint8)      # both flags, either, none
    info = rng.rand(M, 16) * 20 * live.reshape(-1, 1)
    return ids, obs, reward, term, trunc, info, slices


def _record_rows(rng, model, ids, P):
    """The send that answers it: some rows not sent, a duplicate id, a row for an env that awaits nothing, reset rows."""
    M = len(ids)
    ids = ids.copy()
    ids[rng.rand(M) < 0.1] = -1
    live = np.nonzero(ids >= 0)[0]
    if len(live) >= 2 and rng.rand() < 0.8:
        ids[live[-1]] = ids[live[0]]                                   # the smaller row wins
    idle = np.nonzero((model.pend_flags & AWAITS) == 0)[0]
    if M >= 2 and len(idle) and rng.rand() < 0.8:
        ids[rng.randint(M)] = idle[rng.randint(len(idle))]             # awaits nothing (may also hit the duplicate's row: fine)
    if M >= 3 and rng.rand() < 0.3:
        ids[rng.randint(M)] = model.E + 5                              # no such env
    reset = (rng.rand(M) < 0.25).astype(np.uint8)
    actions = rng.randint(0, P * P, M).astype(np.float64)
    return actions, ids, reset


def _feed(buf, model, rng, M, rounds, P, what, full_first=True):
    for r in range(rounds):
        k = min(M, model.E) if (r % 2 == 0 and full_first) else rng.randint(0, min(M, model.E) + 1)
        rows = _observe_rows(rng, model, M, k)
        buf.observe_rows(*[_t(a) for a in rows])
        model.observe(*rows)
        _same(buf, model, (what, "observe", r))
        actions, ids, reset = _record_rows(rng, model, rows[0], P)
        use_reset = r % 4 != 3
        buf.record(_t(actions), _t(ids), _t(reset) if use_reset else None)
        model.record(actions, ids, reset if use_reset else None)
        _same(buf, model, (what, "record", r))


@pytest.mark.parametrize("C", [3, 7])
@pytest.mark.parametrize("M", [1, 5, 65, 1025])
@pytest.mark.parametrize("P", [2, 6, 96])
def test_synthetic_feed_equals_the_model_after_every_call(P, M, C):
    """P = 2 is one 16-byte piece per row, P = 6 nine (less than a wavefront), P = 96 the SAM width; M crosses the wave (64) and workgroup (1024) chunks of
    the scan; C = 3 and 7 wrap several times and M > C stores more rows than the ring holds in one call."""
    E = M + 3
    buf, model = _pair(E, P, C, seed=5)
    rng = np.random.RandomState(1000 * P + 10 * M + C)
    _feed(buf, model, rng, M, 6 if P == 96 and M > 100 else 14, P, (P, M, C))
    st = buf.stats()
    assert st == {"stored": int(model.hdr[0]), "size": min(int(model.hdr[0]), C), "draws": 0, "dropped": int(model.hdr[2]), "rejected": int(model.hdr[3])}
    assert buf.size() == st["size"]
    if M >= 5:
        assert st["stored"] > C and st["dropped"] > 0 and st["rejected"] > 0, st


def _check_sample(buf, model, B, out=None):
    got = buf.sample(B, out=out)
    want = model.sample(B)
    torch.cuda.synchronize()
    for n, w in want.items():
        g = getattr(got, n).cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, n
        assert np.array_equal(g, w), (n, B)
    if want["valid"].all():
        # the images once more, from the device buffer with torch's own conversion -- ToTensor()'s, which runs on the host: there div(255) is the IEEE
        # division; on the device torch multiplies by the reciprocal of a scalar divisor, which is another float for 126 of the 256 byte values
        s = torch.from_numpy(want["slot"].astype(np.int64))
        assert torch.equal(got.state.cpu(), buf.state.cpu()[s].permute(0, 3, 1, 2).float().div(255))
        assert torch.equal(got.next_state.cpu(), buf.next_state.cpu()[s].permute(0, 3, 1, 2).float().div(255))
    return got


def test_policy_planes_equal_the_sampled_planes_for_every_byte():
    """What the policy feeds the network when it acts (to_float_planes, on the device) is what the buffer hands the learner: u8 / 255 by IEEE division."""
    from benchpush_amd.baselines.box_delivery.SAM.policy import to_float_planes
    u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 8, 8, 4)
    want = u8.permute(0, 3, 1, 2).float().div(255)
    assert torch.equal(to_float_planes(u8), want)
    assert torch.equal(to_float_planes(u8.to(DEV)).cpu(), want)


@pytest.mark.parametrize("P,B", [(2, 1), (2, 65), (6, 3), (96, 3), (96, 65)])
def test_sample_equals_the_model(P, B):
    C, E, M = 7, 9, 4
    buf, model = _pair(E, P, C, seed=77)
    twin, _ = _pair(E, P, C, seed=77)
    other, _ = _pair(E, P, C, seed=78)
    rng = np.random.RandomState(B)
    out = _check_sample(buf, model, B)                                   # n == 0: zeros, valid 0
    assert not out.valid.any() and not out.state.any() and not out.next_state.any() and not out.slot.any() and not out.action.any()
    twin.sample(B), other.sample(B)
    # two stored transitions whose images count through the byte values (from P = 6 on, all 256 of them pass through the table)
    ids = np.array([0, 1, -1, -1], np.int32)
    img = (np.arange(2 * P * P * 4) % 256).astype(np.uint8).reshape(2, P, P, 4)
    obs = np.zeros((M, P, P, 4), np.uint8)
    obs[:2] = img
    z, info = np.zeros(M), np.zeros((M, 16))
    for k, slices in enumerate(([0, 0, 0, 0], [2, 1, 0, 0])):
        rows = (ids, (obs + 37 * k).astype(np.uint8), z + k, z.astype(np.uint8), z.astype(np.uint8), info + k, np.array(slices, np.int32))
        for b in (buf, twin, other):
            b.observe_rows(*[_t(a) for a in rows])
            b.record(_t(np.array([3., 2., 0., 0.])), _t(ids))
        model.observe(*rows)
        model.record(np.array([3., 2., 0., 0.]), ids)
    assert model.hdr[0] == 2
    _check_sample(buf, model, B, out=out)                                # n = 2, below B for B = 3 and 65
    twin.sample(B), other.sample(B)
    for _ in range(6):
        rows = _observe_rows(rng, model, M, M)
        model.observe(*rows)
        a, i, _ = _record_rows(rng, model, rows[0], P)
        model.record(a, i)
        for b in (buf, twin, other):
            b.observe_rows(*[_t(x) for x in rows]), b.record(_t(a), _t(i))
    assert model.hdr[0] > C
    _same(buf, model, "before the last draw")
    got = _check_sample(buf, model, B, out=out)
    t, o = twin.sample(B), other.sample(B)
    assert torch.equal(t.slot, got.slot) and torch.equal(t.state, got.state), "same seed, same history: same draw"
    if B > 1:
        assert not torch.equal(o.slot, got.slot), "another seed draws other slots"
        assert len(set(got.slot.tolist())) > 1
    assert buf.stats()["draws"] == 3


def test_state_dict_round_trip_and_rearming():
    P, C, E, M = 6, 7, 12, 8
    buf, model = _pair(E, P, C, seed=3)
    rng = np.random.RandomState(4)
    _feed(buf, model, rng, M, 6, P, "before the save")
    sd = buf.state_dict()
    _feed(buf, model, rng, M, 1, P, "the saved buffer goes on")         # the clones do not follow
    fresh, model2 = _pair(E, P, C, seed=0)
    fresh.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()})
    for n in ReplayModel.TENSORS:                                        # the model of the loaded buffer: the saved tensors, bits 1 and 2 cleared
        setattr(model2, n, sd[n].cpu().numpy().copy())
    model2.seed = 3
    armed = int(((model2.pend_flags & 3) == 3).sum())
    model2.clear_actions()
    assert armed > 0 and fresh.seed == 3
    _same(fresh, model2, "after the load")
    dropped = int(model2.hdr[2])
    rows = _observe_rows(rng, model2, M, M)
    rows = rows[:6] + (np.maximum(rows[6], (rows[0] >= 0).astype(np.int32)),)     # every row a transition row
    fresh.observe_rows(*[_t(a) for a in rows])
    model2.observe(*rows)
    _same(fresh, model2, "first rows after the load")
    assert int(model2.hdr[2]) == dropped + M, "nothing is paired with a stale action"
    _feed(fresh, model2, rng, M, 4, P, "after the load")
    _check_sample(fresh, model2, 5)
    with pytest.raises(ValueError):
        _pair(E, P, C + 1)[0].load_state_dict(sd)


def test_errors_are_raised_before_any_launch():
    from benchpush_amd.replay import DeviceReplayBuffer
    for at in ("heading", "velocity"):
        with pytest.raises(ValueError):
            DeviceReplayBuffer(_stub_env(4, 6, at), 5)
    with pytest.raises(ValueError):
        DeviceReplayBuffer(_stub_env(4, 6), 0)
    with pytest.raises(ValueError):
        DeviceReplayBuffer(_stub_env(4, 3), 5)                           # 3 * 3 * 4 bytes is no multiple of 16
    buf, model = _pair(4, 6, 5)
    rng = np.random.RandomState(0)
    rows = list(_observe_rows(rng, model, 3, 3))
    good = [_t(a) for a in rows]
    for k, bad in ((0, good[0].long()), (1, good[1][:, :5]), (2, good[2].float()), (5, good[5][:, :15]), (6, good[6].cpu()), (3, good[3][:2])):
        args = list(good)
        args[k] = bad
        with pytest.raises(ValueError):
            buf.observe_rows(*args)
    ids = good[0]
    for a, i, r in ((torch.zeros(4, device=DEV), ids, None), (torch.zeros(3, device=DEV), ids.long(), None), (torch.zeros(3), ids, None),
                    (torch.zeros(3, device=DEV), ids, torch.zeros(3, device=DEV))):
        with pytest.raises(ValueError):
            buf.record(a, i, r)
    with pytest.raises(ValueError):
        buf.sample(0)
    with pytest.raises(ValueError):
        buf.sample(4, out=buf.sample(3))
    torch.cuda.synchronize()
    assert buf.stats() == {"stored": 0, "size": 0, "draws": 1, "dropped": 0, "rejected": 0}


# -- the real queue ---------------------------------------------------------------------------------------------------
def _run_real(env, M, C, rounds, budget, seed, block=False):
    """recv / send rounds through DeviceReplayBuffer.recv / send with seeded random actions, resets of the finished envs and a few more; every call is
    mirrored through the model on host copies.  Returns (buffer, the transitions the loop itself saw, in order)."""
    from benchpush_amd.replay import DeviceReplayBuffer
    P = env.obs_shape[0]
    env.reset()
    buf = DeviceReplayBuffer(env, C, seed=seed)
    model = ReplayModel(C, env.num_envs, env.obs_shape, buf.ministeps_col, seed=seed)
    q = env.async_queue(M, budget)
    rng = np.random.RandomState(seed)
    last_obs, last_act, seen = {}, {}, []
    for r in range(rounds):
        ids, obs, rew, term, trunc, info = buf.recv(q, block=block)
        torch.cuda.synchronize()
        h = [t.cpu().numpy().copy() for t in (ids, obs, rew, term, trunc, info, q.slices)]
        model.observe(*h)
        _same(buf, model, ("recv", r))
        for j, e in enumerate(h[0].tolist()):
            if e < 0:
                continue
            if h[6][j] > 0 and e in last_obs and e in last_act:
                seen.append(dict(state=last_obs[e], action=last_act[e], reward=np.float32(h[2][j]), ministeps=np.float32(h[5][j, buf.ministeps_col]),
                                 next_state=h[1][j], nonfinal=0 if h[3][j] else 1, env=e))
            last_obs[e] = h[1][j]
            last_act.pop(e, None)
        actions = rng.randint(0, P * P, M)
        reset = ((h[3] | h[4]).astype(bool) | (rng.rand(M) < 0.1)).astype(np.uint8)
        buf.send(q, _t(actions.astype(np.float64)), ids, _t(reset))
        model.record(actions.astype(np.float64), h[0], reset)
        for j, e in enumerate(h[0].tolist()):
            if e >= 0 and reset[j]:
                last_obs.pop(e, None), last_act.pop(e, None)
            elif e >= 0:
                last_act[e] = int(actions[j])
        _same(buf, model, ("send", r))
    assert q.stats()["rejected"] == 0 and int(model.hdr[3]) == 0, "the buffer accepts exactly the rows the queue accepts"
    q.close()
    env.check_errors()
    return buf, seen


def _check_stored(buf, seen, C):
    """Every stored transition: state is the observation its env received before the stored action, next_state the one after, reward / ministeps the
    queue row's."""
    n = len(seen)
    assert int(buf.hdr[0].item()) == n
    for i in range(max(0, n - C), n):
        s, w = i % C, seen[i]
        for k, v in w.items():
            got = getattr(buf, k)[s].cpu().numpy()
            assert np.array_equal(got, v), (i, s, k)


def _sam_cfg(cls, extra=None):
    return cls(cfg=extra).sam_cfg()


def test_real_queue_box_delivery_sam_width():
    from benchpush_amd.baselines.box_delivery.SAM import BoxDeliverySAM
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    env = BatchedBoxDeliveryEnv(6, cfg=_sam_cfg(BoxDeliverySAM), num_trials=4, bd_overrides={"step_limit": 600})
    assert env.obs_shape == (96, 96, 4)
    buf, seen = _run_real(env, 4, 5, 30, 300, seed=21)
    env.close()
    assert len(seen) > 5, "the ring wrapped"
    _check_stored(buf, seen, 5)


def test_real_queue_box_delivery_default_width_round_trip():
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    env = BatchedBoxDeliveryEnv(2, cfg={"agent": {"action_type": "position"}}, num_trials=2, bd_overrides={"step_limit": 600})
    assert env.obs_shape == (224, 224, 4)
    buf, seen = _run_real(env, 2, 3, 3, 600, seed=22, block=True)
    env.close()
    assert len(seen) >= 1
    _check_stored(buf, seen, 3)


def test_real_queue_area_clearing_sam_width():
    from benchpush_amd.baselines.area_clearing.sam import AreaClearingSAM
    from benchpush_amd.envs.area_clearing import AC_INFO_KEYS, BatchedAreaClearingEnv
    env = BatchedAreaClearingEnv(6, cfg=_sam_cfg(AreaClearingSAM), num_trials=4, bd_overrides={"step_limit": 600})
    assert env.obs_shape == (96, 96, 4)
    buf, seen = _run_real(env, 4, 5, 30, 300, seed=23)
    env.close()
    assert buf.ministeps_col == AC_INFO_KEYS.index("ministeps") == 8
    assert len(seen) > 5, "the ring wrapped"
    _check_stored(buf, seen, 5)
