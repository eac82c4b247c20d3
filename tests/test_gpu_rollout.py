"""Device rollout buffer (benchpush_amd/rollout.py, csrc/bp_rollout.hpp): every tensor of the buffer and every output equals the numpy model's
(tests/rollout_ref.py) with == after every call, on synthetic feeds that cross a wave and the scan's 1024-thread pass, and on the real ship-ice and maze
envs under a short TimeLimit.  The float images are compared with a reference divided on the host: torch's device kernel divides by a scalar through the
reciprocal, which rounds some byte values differently (see the note in tests/test_gpu_replay.py)."""
import types

import numpy as np
import pytest
import torch

from rollout_ref import RolloutModel, image

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAMMA, LAM = 0.97, 0.95


def _stub_env(E, obs_shape, action_dim=1, dtype=torch.uint8, low_dim_state=False):
    """What DeviceRolloutBuffer reads of an env, without one."""
    from benchpush_amd import _lib
    from benchpush_amd.config import DotDict
    return types.SimpleNamespace(cfg=DotDict(low_dim_state=low_dim_state), action_dim=action_dim, L=_lib.load(), device=torch.device(DEV), num_envs=E,
                                 obs_shape=tuple(obs_shape), obs=torch.zeros(1, dtype=dtype))


def _pair(E, T, obs_shape, A=1, seed=0, K=None):
    from benchpush_amd.rollout import DeviceRolloutBuffer
    buf = DeviceRolloutBuffer(_stub_env(E, obs_shape, A), T, GAMMA, LAM, seed=seed, bootstrap_rows=K)
    return buf, RolloutModel(T, E, obs_shape, A, GAMMA, LAM, seed=seed)


def _same(buf, model, what):
    torch.cuda.synchronize()
    for n in RolloutModel.TENSORS:
        got, want = getattr(buf, n).cpu().numpy(), getattr(model, n)
        assert got.dtype == want.dtype and got.shape == want.shape, (what, n)
        assert np.array_equal(got, want), (what, n, np.argwhere(got != want)[:4].tolist())


def _same_arrays(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _step(buf, model, t, obs, action, value, logp, reward, done, trunc, term_obs, boot_values, what):
    """One begin / truncated_rows / end on numpy inputs, the model alongside, compared after every call.  boot_values: [K] for the K bootstrap rows."""
    buf.begin(_t(obs), _t(action), _t(value), _t(logp))
    model.begin(t, obs, action, value, logp)
    _same(buf, model, (what, "begin", t))
    ids, rows = buf.truncated_rows(_t(trunc), _t(term_obs))
    want_ids, want_rows = model.pick_rows(trunc, term_obs, buf.bootstrap_rows)
    _same_arrays(ids, want_ids, (what, "ids", t))
    _same_arrays(rows, want_rows, (what, "rows", t))
    _same(buf, model, (what, "truncated_rows", t))
    buf.end(_t(reward), _t(done), ids, _t(boot_values))
    model.end(t, reward, done, want_ids, boot_values)
    _same(buf, model, (what, "end", t))


def _check_epoch(buf, model, B, epoch, what):
    N = model.T * model.E
    seen, count = [], 0
    for j, batch in enumerate(buf.minibatches(B, epoch)):
        want = model.minibatch(epoch, j, B)
        for n in batch._fields:
            _same_arrays(getattr(batch, n), want[n].reshape(getattr(batch, n).shape), (what, "minibatch", epoch, j, n))
        idx, valid = batch.index.cpu().numpy(), batch.valid.cpu().numpy()
        seen += idx[valid != 0].tolist()
        count += 1
        last_valid = int(valid.sum())
    assert count == (N + B - 1) // B
    assert sorted(seen) == list(range(N)), "an epoch visits every stored transition exactly once"
    return last_valid


def _synthetic_inputs(rng, E, shape, A, K):
    obs = rng.randint(0, 256, (E,) + shape, dtype=np.uint8)
    term_obs = rng.randint(0, 256, (E,) + shape, dtype=np.uint8)
    action = rng.randn(E, A).astype(np.float32)
    value, logp = rng.randn(E).astype(np.float32), -rng.rand(E).astype(np.float32)
    reward = rng.randn(E)                                   # float64, not float32-representable
    done = (rng.rand(E) < 0.3).astype(np.uint8)
    trunc = (done != 0) & (rng.rand(E) < 0.5)
    return obs, action, value, logp, reward, done, trunc, term_obs, rng.randn(K).astype(np.float32)


def test_synthetic_feed_equals_the_model_after_every_call():
    """E = 70 crosses a wave, R = 48 is three 16-byte pieces, B = 64 leaves 210 - 3 * 64 = 18 valid rows in the last minibatch; episode boundaries in every
    row, env 5 done at the last step, bootstrap rows at every step; two rollouts, so that last_done carries over ``clear``."""
    E, T, shape, B = 70, 3, (3, 4, 4), 64
    buf, model = _pair(E, T, shape, seed=9)
    rng = np.random.RandomState(7)
    for rollout in range(2):
        for t in range(T):
            inp = list(_synthetic_inputs(rng, E, shape, 1, E))
            if t == T - 1:
                inp[5][5], inp[5][6] = 1, 0                 # env 5 done, env 6 running after the last step
            _step(buf, model, t, *inp, what=("synthetic", rollout))
        assert model.episode_start.any() and (rollout == 0 or model.episode_start[0].any())
        last = rng.randn(E).astype(np.float32)
        buf.finish(_t(last))
        model.finish(last)
        _same(buf, model, ("synthetic", rollout, "finish"))
        for epoch in (0, 1):
            assert _check_epoch(buf, model, B, 2 * rollout + epoch, ("synthetic", rollout)) == 18
        _same(buf, model, ("synthetic", rollout, "minibatches leave the buffer alone"))
        buf.clear()
    assert buf.stats() == {"unbootstrapped": 0, "stored": 2 * T * E, "steps": 0}


def test_two_action_columns_and_the_vector_form_of_one():
    E, T, shape = 5, 2, (16,)
    buf, model = _pair(E, T, shape, A=2, seed=1)
    rng = np.random.RandomState(3)
    for t in range(T):
        _step(buf, model, t, *_synthetic_inputs(rng, E, shape, 2, E), what="A=2")
    last = rng.randn(E).astype(np.float32)
    buf.finish(_t(last))
    model.finish(last)
    _check_epoch(buf, model, 4, 0, "A=2")
    buf1, model1 = _pair(E, 1, shape, A=1)
    inp = list(_synthetic_inputs(rng, E, shape, 1, E))
    inp[1] = inp[1].reshape(E)                              # actions as [E]
    _step(buf1, model1, 0, *inp, what="A=1 vector")


@pytest.mark.parametrize("K", [1, 7, 1100])
def test_compaction_and_end_across_the_scan_pass(K):
    """E = 1100 crosses the 1024-thread pass of the scan; more masked envs than K leave hdr[0] at the model's count and the unpicked rows' rewards
    without a bootstrap."""
    E, shape = 1100, (16,)
    buf, model = _pair(E, 2, shape, seed=2, K=K)
    rng = np.random.RandomState(K)
    for t in range(2):
        inp = list(_synthetic_inputs(rng, E, shape, 1, K))
        trunc = rng.rand(E) < (0.02 if t == 0 else 0.5)
        trunc[[0, 63, 64, 1023, 1024, 1099]] = True          # the edges of the waves and of the pass
        inp[6] = trunc
        before = int(model.hdr[0])
        _step(buf, model, t, *inp, what=("compaction", K))
        n = int(trunc.sum())
        assert int(model.hdr[0]) - before == max(0, n - K)
        picked = np.nonzero(trunc)[0][:K]
        untouched = np.setdiff1d(np.arange(E), picked)
        assert np.array_equal(model.reward[t][untouched], inp[4][untouched].astype(np.float32)), "no bootstrap outside the picked rows"
        assert K > n or not np.array_equal(model.reward[t][picked], inp[4][picked].astype(np.float32))
    assert buf.stats()["unbootstrapped"] == int(model.hdr[0]) and (K == 1100) == (int(model.hdr[0]) == 0)
    # end without bootstrap rows, and a mask with nothing set
    buf.clear()
    inp = list(_synthetic_inputs(rng, E, shape, 1, K))
    inp[6] = np.zeros(E, bool)
    buf.begin(*[_t(a) for a in inp[:4]])
    model.begin(0, *inp[:4])
    ids, rows = buf.truncated_rows(_t(inp[6]), _t(inp[7]))
    assert bool((ids == -1).all()) and not bool(rows.any())
    buf.end(_t(inp[4]), _t(inp[5]))
    model.end(0, inp[4], inp[5])
    _same(buf, model, ("compaction", K, "end without bootstrap"))


def test_every_byte_value_divides_as_on_the_host():
    E, shape = 2, (256,)
    buf, model = _pair(E, 1, shape)
    obs = np.stack([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1).astype(np.uint8)])
    ids, rows = buf.truncated_rows(_t(np.array([1, 1], np.uint8)), _t(obs))
    _same_arrays(rows, image(obs), "all 256 byte values")
    assert ids.tolist() == [0, 1]
    recip = (obs.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
    assert (recip != image(obs)).any(), "the reciprocal would differ: the comparison above tells the two apart"


def test_refusals_come_before_any_launch():
    from benchpush_amd.rollout import DeviceRolloutBuffer
    E, shape = 4, (16,)
    for bad in (dict(obs_shape=(15,)), dict(dtype=torch.float32), dict(low_dim_state=True)):
        kw = dict(obs_shape=shape)
        kw.update(bad)
        with pytest.raises(ValueError):
            DeviceRolloutBuffer(_stub_env(E, **kw), 2, GAMMA, LAM)
    for bad in (dict(n_steps=0), dict(bootstrap_rows=0), dict(bootstrap_rows=5)):
        kw = dict(n_steps=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            DeviceRolloutBuffer(_stub_env(E, shape), gamma=GAMMA, gae_lambda=LAM, **kw)
    buf, model = _pair(E, 1, shape)
    rng = np.random.RandomState(0)
    obs, action, value, logp, reward, done, trunc, term_obs, boot = [_t(a) for a in _synthetic_inputs(rng, E, shape, 1, E)]
    with pytest.raises(ValueError):
        buf.end(reward, done)                               # no begin
    for bad in ((obs.cpu(), action, value, logp), (obs.float(), action, value, logp), (obs[:3], action, value, logp), (obs, action.double(), value, logp),
                (obs, action, value[:3], logp), (obs, action, value, logp.reshape(E, 1)), (obs.repeat(1, 2)[:, ::2], action, value, logp)):
        with pytest.raises(ValueError):
            buf.begin(*bad)
    with pytest.raises(ValueError):
        buf.finish(value)                                   # not full
    with pytest.raises(ValueError):
        next(buf.minibatches(2, 0))
    buf.begin(obs, action, value, logp)
    with pytest.raises(ValueError):
        buf.begin(obs, action, value, logp)                 # the begin before has no end
    for bad in ((reward.float(), done), (reward, done.int()), (reward, done, boot[:2].int(), None), (reward, done, torch.zeros(2, dtype=torch.int64, device=DEV), boot[:2])):
        with pytest.raises(ValueError):
            buf.end(*bad)
    with pytest.raises(ValueError):
        buf.truncated_rows(trunc.float(), term_obs)
    buf.end(reward, done)
    with pytest.raises(ValueError):
        buf.begin(obs, action, value, logp)                 # full
    with pytest.raises(ValueError):
        next(buf.minibatches(2, 0))                         # full but not finished
    buf.finish(value)
    with pytest.raises(ValueError):
        buf.minibatches(0, 0)
    assert len(list(buf.minibatches(3, 0))) == 2
    torch.cuda.synchronize()
    assert torch.equal(buf.hdr.cpu(), torch.tensor([0, E])), "the refused calls stored nothing"
    assert DeviceRolloutBuffer.storage_bytes(E, 1, shape, 1) == sum(getattr(buf, n).numel() * getattr(buf, n).element_size() for n in RolloutModel.TENSORS)


def test_checkpoint_round_trip():
    E, T, shape = 6, 3, (32,)
    buf, model = _pair(E, T, shape, seed=4)
    rng = np.random.RandomState(11)
    for t in range(2):
        _step(buf, model, t, *_synthetic_inputs(rng, E, shape, 1, E), what="before the checkpoint")
    sd = buf.state_dict()
    buf2, _ = _pair(E, T, shape, seed=0)
    buf2.load_state_dict(sd)
    assert buf2.t == 2 and buf2.seed == 4
    _same(buf2, model, "reloaded")
    inp = _synthetic_inputs(rng, E, shape, 1, E)
    _step(buf2, model, 2, *inp, what="after the checkpoint")
    last = rng.randn(E).astype(np.float32)
    buf2.finish(_t(last))
    model.finish(last)
    _check_epoch(buf2, model, 4, 0, "after the checkpoint")
    torch.cuda.synchronize()
    assert torch.equal(buf.obs[2], torch.zeros_like(buf.obs[2])), "the state dict holds clones"
    other, _ = _pair(E, T + 1, shape)
    with pytest.raises(ValueError):
        other.load_state_dict(sd)


def _real_env_rollout(venv, T, B):
    """T steps of a BatchedVecEnv(to_numpy=False) with random actions, values and bootstrap values; the model is fed the same outputs read back."""
    from benchpush_amd.rollout import DeviceRolloutBuffer
    E, shape = venv.num_envs, tuple(venv.env.obs_shape)
    buf = DeviceRolloutBuffer(venv, T, GAMMA, LAM, seed=21)
    model = RolloutModel(T, E, shape, 1, GAMMA, LAM, seed=21)
    rng = np.random.RandomState(E)
    obs = venv.reset()
    truncations = 0
    for t in range(T):
        action = rng.uniform(-1, 1, (E, 1)).astype(np.float32)
        value, logp, boot = rng.randn(E).astype(np.float32), -rng.rand(E).astype(np.float32), rng.randn(E).astype(np.float32)
        obs_h = obs.cpu().numpy()
        buf.begin(obs, _t(action), _t(value), _t(logp))
        model.begin(t, obs_h, action, value, logp)
        _same(buf, model, ("real", "begin", t))
        obs, reward, done, infos = venv.step(_t(action))
        trunc_h, term_h = infos.truncated_mask.cpu().numpy(), infos.terminal_rows.cpu().numpy()
        ids, rows = buf.truncated_rows(infos.truncated_mask, infos.terminal_rows)
        want_ids, want_rows = model.pick_rows(trunc_h, term_h, E)
        _same_arrays(ids, want_ids, ("real", "ids", t))
        _same_arrays(rows, want_rows, ("real", "rows", t))
        buf.end(reward, done, ids, _t(boot))
        model.end(t, reward.cpu().numpy(), done.cpu().numpy(), want_ids, boot)
        _same(buf, model, ("real", "end", t))
        truncations += int(trunc_h.sum())
    last = rng.randn(E).astype(np.float32)
    buf.finish(_t(last))
    model.finish(last)
    _same(buf, model, ("real", "finish"))
    _check_epoch(buf, model, B, 0, "real")
    assert truncations > 0 and model.episode_start[1:].any(), "the TimeLimit of 3 steps truncated episodes within the rollout"
    assert buf.stats()["unbootstrapped"] == 0


def test_real_ship_ice_rollout_equals_the_model():
    from benchpush_amd import _lib
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    from benchpush_amd.envs.vec_env import BatchedVecEnv
    venv = BatchedVecEnv(BatchedShipIceEnv(8, cfg={"concentration": 0.1}, num_trials=4, device=DEV), _lib.INFO_KEYS, max_episode_steps=3, to_numpy=False)
    try:
        _real_env_rollout(venv, 6, 16)
    finally:
        venv.close()


def test_real_maze_rollout_equals_the_model():
    """The maze's observation row is larger than ship-ice's: more than one 256-lane piece block per row either way, a different count."""
    from benchpush_amd.envs.maze_namo import MAZE_INFO_KEYS, BatchedMazeEnv
    from benchpush_amd.envs.vec_env import BatchedVecEnv
    venv = BatchedVecEnv(BatchedMazeEnv(4, num_layouts=4, device=DEV), MAZE_INFO_KEYS, max_episode_steps=3, to_numpy=False)
    try:
        _real_env_rollout(venv, 6, 16)
    finally:
        venv.close()
