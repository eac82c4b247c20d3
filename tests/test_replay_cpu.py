"""Replay buffer on the ready queue, the parts that need no GPU: the index rule (bp_replay_index against the model), the C surface, and the model's own
rules (tests/replay_ref.py) on hand-made feeds."""
import ctypes as C
import os

import numpy as np
import pytest

from replay_ref import ACTED, AWAITS, HELD, ReplayModel, replay_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bp_sizeof_replay_desc", "bp_sizeof_replay_batch", "bp_replay_index", "bp_replay_observe", "bp_replay_record", "bp_replay_sample")


@pytest.mark.parametrize("n", [1, 2, 5, 2 ** 31 - 1])
def test_replay_index_equals_the_model_and_stays_below_n(n):
    from benchpush_amd import _lib
    L = _lib.load()
    rng = np.random.RandomState(n % 1000)
    seen = set()
    for seed in [0, 1, 2 ** 64 - 1] + [int(s) for s in rng.randint(0, 2 ** 62, 5)]:
        for draw in (0, 1, 7, 2 ** 40 + 3):
            for b in list(range(40)) + [1023, 65535]:
                got = L.bp_replay_index(seed, draw, b, n)
                assert got == replay_index(seed, draw, b, n), (seed, draw, b, n)
                assert 0 <= got < n
                seen.add(got)
    assert len(seen) == min(n, len(seen)) and (n < 5 or len(seen) > 1)
    if n <= 5:
        assert seen == set(range(n)), "every slot is drawn"
    for bad in (0, -1, 2 ** 31):
        assert L.bp_replay_index(0, 0, 0, bad) == -1


def test_replay_abi_declared_and_exported():
    from benchpush_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "benchpush_amd.h")).read()
    L = _lib.load()
    for n in NAMES:
        assert n in _lib.EXPORTS and (n + "(") in hdr and hasattr(L, n), n
    assert "#define BP_ABI_VERSION 11" in hdr and L.bp_abi_version() == 11
    assert L.bp_sizeof_replay_desc() == C.sizeof(_lib.BpReplayDesc) and L.bp_sizeof_replay_batch() == C.sizeof(_lib.BpReplayBatch)


def _desc(_lib, **over):
    d = _lib.BpReplayDesc()
    d.capacity, d.num_envs, d.device, d.action_dim, d.row_bytes, d.max_rows = 4, 3, 0, 1, 16, 8
    for i, (n, _) in enumerate(_lib.BpReplayDesc._fields_[7:]):
        setattr(d, n, 4096 * (i + 1))       # never dereferenced: every call below is refused before anything is launched
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_replay_calls_refuse_bad_sizes_before_launching():
    from benchpush_amd import _lib
    L = _lib.load()
    p = C.c_void_p(4096)
    obs = lambda d, M=2, col=7: L.bp_replay_observe(C.byref(d), p, p, p, p, p, p, p, M, col, None)   # noqa: E731
    for over in (dict(row_bytes=24), dict(row_bytes=0), dict(capacity=0), dict(num_envs=0), dict(action_dim=2), dict(state=None), dict(hdr=None)):
        d = _desc(_lib, **over)
        assert obs(d) == -1, over
        assert L.bp_replay_record(C.byref(d), p, p, None, 2, None) == -1, over
        assert L.bp_replay_sample(C.byref(d), 2, 0, C.byref(_lib.BpReplayBatch()), None) == -1, over
    d = _desc(_lib)
    assert obs(d, M=0) == -1 and obs(d, M=9) == -1 and obs(d, col=16) == -1 and obs(d, col=-1) == -1
    assert L.bp_replay_record(C.byref(d), p, p, None, 0, None) == -1
    assert L.bp_replay_sample(C.byref(d), 0, 0, C.byref(_lib.BpReplayBatch()), None) == -1
    assert L.bp_replay_sample(C.byref(d), 2, 0, C.byref(_lib.BpReplayBatch()), None) == -1, "NULL outputs"


# -- the model's own rules ------------------------------------------------------------------------------------------
def _feed(m, ids, slices, tag, term=None):
    M = len(ids)
    obs = np.zeros((M,) + m.obs_shape, np.uint8)
    for j in range(M):
        obs[j] = tag + j
    info = np.zeros((M, 16))
    info[:, m.mcol] = np.arange(M) + 0.5
    m.observe(np.array(ids), obs, np.arange(M) * 1.25, np.zeros(M, np.uint8) if term is None else np.array(term, np.uint8), np.zeros(M, np.uint8), info,
              np.array(slices))
    return obs


def test_model_pairs_rows_of_the_same_env_and_wraps():
    m = ReplayModel(3, 4, (2, 2, 4), 7)
    o0 = _feed(m, [0, 1, 2, -1], [0, 0, 0, 0], 10)                      # fresh rows: nothing stored, three envs await a record
    assert m.hdr.tolist() == [0, 0, 0, 0] and m.pend_flags.tolist() == [HELD | AWAITS] * 3 + [0]
    m.record(np.array([5., 6., 7., 9.]), np.array([0, 1, 2, -1]))
    assert m.pend_flags.tolist() == [HELD | ACTED] * 3 + [0] and m.hdr[3] == 0
    o1 = _feed(m, [2, 0, -1, 1], [3, 1, 0, 2], 20, term=[1, 0, 0, 0])   # three transitions, in row order
    assert m.hdr[0] == 3 and m.env.tolist() == [2, 0, 1] and m.action.tolist() == [7, 5, 6] and m.nonfinal.tolist() == [0, 1, 1]
    assert np.array_equal(m.state[0], o0[2]) and np.array_equal(m.next_state[0], o1[0]) and np.array_equal(m.state[2], o0[1])
    assert m.reward.tolist() == [0.0, 1.25, 3.75] and m.ministeps.tolist() == [0.5, 1.5, 3.5]
    m.record(np.array([1., 2.]), np.array([0, 1]))
    o2 = _feed(m, [1, 0], [1, 1], 30)                                    # wraps: slots 0 and 1 again
    assert m.hdr[0] == 5 and m.env.tolist() == [1, 0, 1] and np.array_equal(m.state[0], o1[3]) and np.array_equal(m.next_state[1], o2[1])


def test_model_more_rows_than_capacity_keeps_the_last_ones():
    m = ReplayModel(2, 5, (2, 2, 4), 7)
    _feed(m, [0, 1, 2, 3, 4], [0] * 5, 10)
    m.record(np.arange(5.) + 40, np.arange(5))
    _feed(m, [0, 1, 2, 3, 4], [1] * 5, 20)
    assert m.hdr[0] == 5 and m.env.tolist() == [4, 3] and m.action.tolist() == [44, 43], "slot (0 + rank) % 2, the later rows overwrite the earlier ones"


def test_model_counts_dropped_and_rejected_rows():
    m = ReplayModel(4, 3, (2, 2, 4), 8)
    _feed(m, [0, 1], [2, 0], 10)                 # env 0: a transition row without a pending observation
    assert m.hdr.tolist() == [0, 0, 1, 0]
    m.record(np.array([3.]), np.array([1]))      # env 0 gets no action
    _feed(m, [0, 1], [1, 1], 20)                 # env 0 lacks bit 1: dropped; env 1 stored
    assert m.hdr.tolist() == [1, 0, 2, 0] and m.env[0] == 1
    m.record(np.array([1., 2., 3., 4.]), np.array([0, 0, 2, 7]))   # duplicate: the smaller row wins; env 2 awaits nothing; env 7 does not exist
    assert m.hdr[3] == 3 and m.pend_action[0] == 1 and m.pend_flags[0] == HELD | ACTED and m.pend_flags[2] == 0


def test_model_reset_rows_forget_the_pending_observation():
    m = ReplayModel(4, 2, (2, 2, 4), 7)
    _feed(m, [0, 1], [0, 0], 10)
    m.record(np.array([1., 2.]), np.array([0, 1]), np.array([1, 0], np.uint8))
    assert m.pend_flags.tolist() == [0, HELD | ACTED]
    _feed(m, [0, 1], [0, 1], 20)                 # env 0 comes back as a fresh row and is armed again; env 1 stores
    assert m.hdr.tolist() == [1, 0, 0, 0] and m.pend_flags.tolist() == [HELD | AWAITS] * 2
    m.record(np.array([4.]), np.array([0]))
    _feed(m, [0], [1], 30)
    assert m.hdr[0] == 2 and m.env[:2].tolist() == [1, 0] and m.action[1] == 4 and int(m.state[1][0, 0, 0]) == 20


def test_model_sample_rule():
    m = ReplayModel(3, 2, (2, 2, 4), 7, seed=11)
    assert m.sample_slots(4) is None and m.hdr[1] == 1
    _feed(m, [0], [0], 1)
    m.record(np.array([2.]), np.array([0]))
    _feed(m, [0], [1], 200)
    s = m.sample(5)
    assert s["slot"].tolist() == [0] * 5 and s["valid"].tolist() == [1] * 5 and m.hdr[1] == 2
    assert s["state"].shape == (5, 4, 2, 2) and s["state"][0, 0, 0, 0] == np.float32(1) / np.float32(255) and s["next_state"][0, 0, 0, 0] == np.float32(200) / np.float32(255)
