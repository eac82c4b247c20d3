"""Device transition buffer (benchpush_amd/transitions.py, csrc/bp_transitions.hpp): every tensor of the buffer and every sample output equals the numpy
model's (tests/transitions_ref.py) with == after every call, on synthetic feeds whose sizes cross a wave, the 1024-thread pass of the bookkeeping kernels
and the 256-lane strip of the copy, and on the real ship-ice and maze envs under a short TimeLimit.  The float images are compared with a reference
divided on the host (see the note in tests/test_gpu_rollout.py)."""
import types

import numpy as np
import pytest
import torch

from transitions_ref import TransitionModel, image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stub_env(E, obs_shape, action_dim=1, dtype=torch.uint8, low_dim_state=False):
    """What DeviceTransitionBuffer reads of an env, without one."""
    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    return types.SimpleNamespace(cfg=DotDict(low_dim_state=low_dim_state), action_dim=action_dim, L=_lib.load(), device=torch.device(DEV), num_envs=E,
                                 obs_shape=tuple(obs_shape), obs=torch.zeros(1, dtype=dtype))


def _pair(E, T, obs_shape, A=1, seed=0):
    from benchpush_amd.transitions import DeviceTransitionBuffer
    buf = DeviceTransitionBuffer(_stub_env(E, obs_shape, A), T * E + E // 2, seed=seed)      # T = buffer_size // E
    model = TransitionModel(E, T * E + E // 2, obs_shape, A, seed=seed)
    assert buf.steps == model.T == T
    return buf, model


def _same(buf, model, what):
    torch.cuda.synchronize()
    for n in TransitionModel.TENSORS:
        got, want = getattr(buf, n).cpu().numpy(), getattr(model, n)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, n)
        assert np.array_equal(got, want), (what, n, np.argwhere(got != want)[:4].tolist())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(rng, E, shape, A, pattern):
    obs, nxt, term = (rng.randint(0, 256, (E,) + tuple(shape), dtype=np.uint8) for _ in range(3))
    done = {"none": np.zeros(E, bool), "all": np.ones(E, bool), "mixed": rng.rand(E) < 0.4}[pattern]
    trunc = rng.rand(E) < 0.5                               # set on envs that are not done as well: their timeout stays 0
    return obs, nxt, term, rng.randn(E, A).astype(np.float32), rng.randn(E), done, trunc     # the rewards are float64, not float32-representable


def _add(buf, model, inp, what):
    buf.add(*[_t(a) for a in inp])
    model.add(*inp)
    _same(buf, model, (what, "add"))


def _sample(buf, model, B, what):
    batch = buf.sample(B)
    want = model.sample(B)
    torch.cuda.synchronize()
    for n in batch._fields:
        got, w = getattr(batch, n).cpu().numpy(), want[n].reshape(getattr(batch, n).shape)
        assert got.dtype == w.dtype, (what, n)
        assert np.array_equal(got, w), (what, "sample", B, n, np.argwhere(got != w)[:4].tolist())
    _same(buf, model, (what, "sample", B))
    return want


@pytest.mark.parametrize("E,shape,A", [(70, (3, 4, 4), 1), (1030, (16,), 3), (5, (16 * 257,), 3)])
def test_synthetic_feed_equals_the_model_after_every_call(E, shape, A):
    """E = 70 crosses a wave, E = 1030 the 1024-thread pass; rows of 48 bytes are three pieces, fewer than a wave; rows of 16 * 257 bytes leave one piece
    to the second 256-lane strip.  T = 3 with 5 adds: the ring wraps and the two oldest rows are overwritten.  Samples of 1, 64 and 130 rows before any
    add, with one and two rows filled, and with the full ring."""
    T = 3
    buf, model = _pair(E, T, shape, A, seed=9)
    rng = np.random.RandomState(E)
    for B in (1, 64, 130):
        want = _sample(buf, model, B, "empty")
        assert not want["valid"].any() and (want["slot"] == -1).all() and not want["obs"].any()
    saw_timeout = saw_plain_done = False
    for s, pattern in enumerate(("mixed", "none", "all", "mixed", "mixed")):
        inp = _inputs(rng, E, shape, A, pattern)
        _add(buf, model, inp, (E, s, pattern))
        row = s % T
        assert np.array_equal(model.timeout[row], (inp[5] & inp[6]).astype(np.uint8)) and not model.timeout[row][~inp[5]].any()
        for B in (1, 64, 130):
            want = _sample(buf, model, B, (E, s))
            assert want["valid"].all() and want["slot"].max() < min(s + 1, T) * E
            t, e = np.divmod(want["slot"], E)
            saw_timeout |= bool((model.timeout[t, e] != 0).any())
            saw_plain_done |= bool(((model.done[t, e] != 0) & (model.timeout[t, e] == 0)).any())
    assert saw_timeout and saw_plain_done, "the samples met both kinds of done"
    assert buf.stats() == {"adds": 5, "draws": 18, "size": T * E} and buf.size() == T * E
    assert int(model.hdr[1]) == 18, "one draw per call"


def test_vector_actions_and_every_byte_value():
    """Actions as [E] with A = 1; a row of all 256 byte values divides as on the host, where the reciprocal would not."""
    E, shape = 2, (256,)
    buf, model = _pair(E, 1, shape)
    obs = np.stack([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1).astype(np.uint8)])
    inp = (obs, obs[::-1].copy(), obs.copy(), np.array([0.25, -0.5], np.float32), np.array([1.0, 2.0]), np.array([True, False]), np.array([False, False]))
    buf.add(*[_t(a) for a in inp])
    model.add(*inp)
    _same(buf, model, "vector actions")
    want = _sample(buf, model, 64, "bytes")
    assert set(want["slot"].tolist()) == {0, 1}
    recip = (obs.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    assert (recip != image(obs)).any(), "the reciprocal would differ: the comparison above tells the two apart"


def test_same_seed_same_batches_other_seed_other_slots():
    E, T, shape = 70, 3, (48,)
    bufs = [_pair(E, T, shape, 1, seed=s)[0] for s in (4, 4, 5)]
    rng = np.random.RandomState(1)
    for s in range(2):
        inp = [_t(a) for a in _inputs(rng, E, shape, 1, "mixed")]
        for b in bufs:
            b.add(*inp)
    for call in range(3):
        batches = [b.sample(64) for b in bufs]
        torch.cuda.synchronize()
        for n in batches[0]._fields:
            assert torch.equal(getattr(batches[0], n), getattr(batches[1], n)), (call, n)
        assert not torch.equal(batches[0].slot, batches[2].slot), "another seed draws other slots"
        assert [int(b.hdr[1]) for b in bufs] == [call + 1] * 3, "the draw counter advances by one per call"
    first = bufs[0].sample(64).slot.clone()
    assert not torch.equal(first, bufs[0].sample(64).slot), "successive draws differ"
    assert bufs[0].sample(64) is bufs[0].sample(64), "the same tensors every call"


def test_checkpoint_round_trip():
    E, T, shape = 6, 3, (32,)
    buf, model = _pair(E, T, shape, 2, seed=4)
    rng = np.random.RandomState(11)
    for s in range(4):
        _add(buf, model, _inputs(rng, E, shape, 2, "mixed"), "before the checkpoint")
    _sample(buf, model, 8, "before the checkpoint")
    sd = buf.state_dict()
    buf2, _ = _pair(E, T, shape, 2, seed=0)
    buf2.load_state_dict(sd)
    assert buf2.seed == 4
    _same(buf2, model, "reloaded")
    a, b = buf.sample(64), buf2.sample(64)
    torch.cuda.synchronize()
    for n in a._fields:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    model.sample(64)
    _add(buf2, model, _inputs(rng, E, shape, 2, "mixed"), "after the checkpoint")
    _sample(buf2, model, 8, "after the checkpoint")
    assert int(buf.hdr[0]) == 4, "the state dict holds clones"
    other, _ = _pair(E, T + 1, shape, 2)
    with pytest.raises(ValueError):
        other.load_state_dict(sd)
    bad = dict(sd, reward=sd["reward"].double())
    with pytest.raises(ValueError):
        buf2.load_state_dict(bad)


def test_refusals_come_before_any_launch():
    from benchpush_amd.transitions import DeviceTransitionBuffer
    E, shape = 4, (16,)
    for bad in (dict(obs_shape=(15,)), dict(dtype=torch.float32), dict(low_dim_state=True)):
        kw = dict(obs_shape=shape)
        kw.update(bad)
        with pytest.raises(ValueError):
            DeviceTransitionBuffer(_stub_env(E, **kw), 8)
    with pytest.raises(ValueError):
        DeviceTransitionBuffer(_stub_env(2 ** 16, shape), 2 ** 31)          # T * E = 2^31 > 2^31 - 1, refused before anything is allocated
    with pytest.raises(ValueError):
        DeviceTransitionBuffer(_stub_env(E, shape), 0)
    buf, model = _pair(E, 2, shape, 2)
    rng = np.random.RandomState(0)
    good = [_t(a) for a in _inputs(rng, E, shape, 2, "mixed")]
    buf.add(*good)
    buf.sample(3)
    obs, nxt, term, action, reward, done, trunc = good
    bads = [(0, obs.cpu()), (0, obs.float()), (0, obs[:3]), (0, obs.repeat(1, 2)[:, ::2]), (1, nxt.int()), (1, nxt[:, :8]), (2, term.cpu()), (2, term[:2]),
            (3, action.double()), (3, action[:, :1]), (3, action.t().contiguous().t()), (3, action.reshape(-1)), (4, reward.float()), (4, reward[:3]),
            (5, done.int()), (5, done[:3]), (6, trunc.float()), (6, trunc.cpu()), (6, None), (0, obs.cpu().numpy())]
    for i, t in bads:
        args = list(good)
        args[i] = t
        with pytest.raises(ValueError):
            buf.add(*args)
    for B in (0, -1):
        with pytest.raises(ValueError):
            buf.sample(B)
    torch.cuda.synchronize()
    assert torch.equal(buf.hdr.cpu(), torch.tensor([1, 1])), "the refused calls stored and drew nothing"
    assert DeviceTransitionBuffer.storage_bytes(E, 2 * E + 2, shape, 2) == sum(getattr(buf, n).numel() * getattr(buf, n).element_size()
                                                                             for n in TransitionModel.TENSORS)


def _real_env_feed(venv, steps, B):
    """`steps` steps of a BatchedVecEnv(to_numpy=False) with random actions under a TimeLimit of 3; the model is fed the same device tensors, copied to
    the host before the next step."""
    from benchpush_amd.transitions import DeviceTransitionBuffer
    venv.max_episode_steps = 3
    E, shape = venv.num_envs, tuple(venv.env.obs_shape)
    buf = DeviceTransitionBuffer(venv, 5 * E, seed=21)
    model = TransitionModel(E, 5 * E, shape, 1, seed=21)
    rng = np.random.RandomState(E)
    obs = venv.reset()
    dones = timeouts = 0
    for s in range(steps):
        action = _t(rng.uniform(-1, 1, (E, 1)).astype(np.float32))
        held = obs.clone()                                  # the env rewrites its batch in place
        obs, reward, done, infos = venv.step(action)
        buf.add(held, obs, infos.terminal_rows, action, reward, done, infos.truncated_mask)
        host = [t.cpu().numpy() for t in (held, obs, infos.terminal_rows, action, reward, done, infos.truncated_mask)]
        model.add(*host)
        _same(buf, model, ("real", "add", s))
        _sample(buf, model, B, ("real", s))
        dones, timeouts = dones + int(host[5].sum()), timeouts + int((host[5] & host[6]).sum())
        for e in np.nonzero(host[5])[0]:
            assert np.array_equal(model.next_obs[s % model.T, e], host[2][e]), "a finished env's next observation is its terminal observation"
    assert dones > 0 and timeouts > 0 and int(model.timeout.sum()) > 0, "the TimeLimit of 3 steps ended episodes within the feed"
    assert buf.stats() == {"adds": steps, "draws": steps, "size": 5 * E}


def test_real_ship_ice_feed_equals_the_model():
    from benchpush_amd.envs.vec_env import make_ship_ice_vec_env
    venv = make_ship_ice_vec_env(6, to_numpy=False)
    try:
        _real_env_feed(venv, 8, 16)
    finally:
        venv.close()


def test_real_maze_feed_equals_the_model():
    from benchpush_amd.envs.vec_env import make_maze_vec_env
    venv = make_maze_vec_env(6, to_numpy=False)
    try:
        _real_env_feed(venv, 8, 16)
    finally:
        venv.close()
