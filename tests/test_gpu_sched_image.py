"""Park images of the preemptive step scheduler (-m gpu): an env that yields inside a step leaves and returns as a raw copy of its running state
(LDS block, arbiter registers, sub-step state; csrc/bp_kernels.hpp: image_store / image_load) instead of going through the persistent format.

Bar: bit-exact.  Every variant -- the default, BP_SCHED_IMAGE=1 (images), BP_SCHED_IMAGE=0 (the store_state / load_state park), BP_SCHED=0 (one wavefront
per env for the whole step, never parked) and chunks of 20 sub-steps with a yield at every boundary from the first, with and without images -- must produce
the same outputs of every step() and the same exported body state, compared with ==.  A fresh handle per environment setting, as in test_gpu_parity.py's
variant test.  (Images are off by default -- bit-identical, but no gain on the launch: tools/experiments/README.md -- so the image cases ask for them.)
"""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

E, STEPS = 4096, 8
SWITCHES = ("BP_SCHED", "BP_SCHED_IMAGE", "BP_SCHED_YMASK", "BP_SCHED_PERSIST", "BP_PAIR")
EVERY = {"BP_SCHED": "20", "BP_SCHED_YMASK": "0xFFFFFFFF"}      # envs park at every boundary from the first
VARIANTS = ({}, {"BP_SCHED_IMAGE": "1"}, {"BP_SCHED_IMAGE": "0"}, EVERY, dict(EVERY, BP_SCHED_IMAGE="1"),
            dict(EVERY, BP_SCHED_IMAGE="1", BP_SCHED_PERSIST="0"))   # the last: the dispatcher-driven kernel parks and resumes with images too


def _actions(seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return (torch.rand((STEPS, E), generator=g, device="cuda:0", dtype=torch.float64) * 2 - 1).float().double()


def _run(monkeypatch, mk, acts, env_vars, expect=None):
    """All outputs of reset() and of STEPS steps under `env_vars` (observation, reward, termination / truncation flags, info) and the body state after every
    step, plus the device memory the handle took."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    gc.collect()
    torch.cuda.empty_cache()                                       # what the handle and its buffers take comes fresh from the device every time
    free0 = torch.cuda.mem_get_info(0)[0]
    env = mk()
    used = free0 - torch.cuda.mem_get_info(0)[0]
    # the scheduler runs with the chunk the setting asks for (a chunk the library cannot serve would silently mean one wavefront per env)
    chunk = int(env.L.bp_sched_chunk(env.h))
    assert chunk == int(env_vars["BP_SCHED"]) if "BP_SCHED" in env_vars else chunk > 0
    if expect is not None:
        expect(env)
    obs, info = env.reset()
    out = {"reset_obs": obs.clone(), "reset_info": info.clone(), "obs": [], "rew": [], "term": [], "trunc": [], "info": [], "bodies": []}
    for t in range(STEPS):
        obs, rew, term, trunc, info = env.step(acts[t])
        out["obs"].append(obs.clone()); out["rew"].append(rew.clone()); out["term"].append(term.clone()); out["trunc"].append(trunc.clone()); out["info"].append(info.clone())
        out["bodies"].append(env.body_state().clone())
        env.reset(term)
    env.check_errors()
    out["final_bodies"] = env.body_state().clone()                 # after the last auto-reset
    env.close()
    return out, used


def _assert_equal(ref, got, what):
    assert ref.keys() == got.keys()
    for k in ref:
        a, b = ref[k], got[k]
        if isinstance(a, list):
            assert len(a) == len(b) == STEPS
            for t in range(STEPS):
                assert torch.equal(a[t], b[t]), (what, k, t)
        else:
            assert torch.equal(a, b), (what, k)


def _compare_variants(monkeypatch, mk, seed):
    acts = _actions(seed)
    ref, _ = _run(monkeypatch, mk, acts, {"BP_SCHED": "0"})       # never parked: the state every resumed wave must be in
    moved = sum(int((ref["bodies"][t] != ref["bodies"][t - 1]).any(dim=-1).sum().item()) for t in range(1, STEPS))
    assert moved > E                                               # bodies are pushed around in the window: the steps are not idle
    for variant in VARIANTS:
        got, _ = _run(monkeypatch, mk, acts, variant)
        _assert_equal(ref, got, variant)


def _ship(conc, ntrials, seed):
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    trials = default_trials(conc, ntrials, base_seed=seed)
    return lambda: BatchedShipIceEnv(E, cfg={"concentration": conc}, trials=trials, device="cuda:0")


def test_park_images_are_bit_identical_ship_ice_c2(monkeypatch):
    """4096 envs of the flagship configuration (30 % concentration), 8 steps from reset."""
    _compare_variants(monkeypatch, _ship(0.3, 24, 3), seed=5)


def test_park_images_are_bit_identical_ship_ice_50pct(monkeypatch):
    """The same at 50 % concentration: more arbiters, more velocity slots, longer moving lists in the image."""
    _compare_variants(monkeypatch, _ship(0.5, 12, 7), seed=6)


def test_park_images_are_bit_identical_maze(monkeypatch):
    """maze-NAMO-v0 (k_physics_step_schedl_maze / _sched_maze): five kinematic robot slots and the sticky wall flag travel in the image."""
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    _compare_variants(monkeypatch, lambda: BatchedMazeEnv(E, cfg={"num_obstacles": 20}, num_layouts=16, base_seed=2, device="cuda:0"), seed=9)


def test_pairing_launches_keep_the_persistent_park(monkeypatch):
    """BP_PAIR=2 (two envs per wavefront inside the scheduler): a parked env may be continued by a half-wave with another LDS layout, so such a handle takes
    the store_state / load_state park whatever BP_SCHED_IMAGE says.  Seen from outside: it is a pairing handle, it allocates no images (its device memory
    does not depend on the switch, while a solo handle's grows by at least E x 32 KB with images on), and its results equal the unparked kernel's."""
    mk = _ship(0.3, 24, 3)
    acts = _actions(5)
    ref, _ = _run(monkeypatch, mk, acts, {"BP_SCHED": "0"})

    def is_pairing(env):
        assert int(env.L.bp_pair_mode(env.h)) == 2

    got, used_pair = _run(monkeypatch, mk, acts, {"BP_PAIR": "2", "BP_SCHED_IMAGE": "1"}, expect=is_pairing)
    _assert_equal(ref, got, "BP_PAIR=2 BP_SCHED_IMAGE=1")
    got0, used_pair0 = _run(monkeypatch, mk, acts, {"BP_PAIR": "2", "BP_SCHED_IMAGE": "0"}, expect=is_pairing)
    _assert_equal(ref, got0, "BP_PAIR=2 BP_SCHED_IMAGE=0")
    del got, got0
    _, used_img = _run(monkeypatch, mk, acts, {"BP_SCHED_IMAGE": "1"})
    _, used_noimg = _run(monkeypatch, mk, acts, {"BP_SCHED_IMAGE": "0"})
    assert used_img - used_noimg >= E * 32 * 1024                  # solo handle: one image of 33 KB per env
    assert abs(used_pair - used_pair0) < E * 16 * 1024             # pairing handle: none with either setting (half an image per env would show)


def test_completion_launch_finishes_a_dropped_env_from_its_image(monkeypatch):
    """The scheduler fault path of test_gpu_parity.py (its hook, BP_SCHED_DEBUG_DROP=1 in the diagnostic twin: env 1 is parked after its first chunk and its
    queue item is lost) with images on: the completion launch that follows resumes the env from its image.  Results equal the unscheduled kernel's."""
    from benchpush_amd import _lib
    from benchpush_amd.build import DBG_LIB_PATH, build_debug_paths
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    build_debug_paths()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setenv("BP_PROF", "1")
    monkeypatch.setenv("BP_PROF_LIB", DBG_LIB_PATH)
    trials = default_trials(0.3, 3, base_seed=5)
    n, steps = 9, 12
    g = torch.Generator(device="cuda:0")
    g.manual_seed(11)
    acts = (torch.rand((steps, n), generator=g, device="cuda:0", dtype=torch.float64) * 2 - 1).float().double()

    def run(env_vars):
        for k in SWITCHES + ("BP_SCHED_DEBUG_DROP",):
            monkeypatch.delenv(k, raising=False)
        for k, v in env_vars.items():
            monkeypatch.setenv(k, v)
        env = BatchedShipIceEnv(n, cfg={"concentration": 0.3}, trials=trials, device="cuda:0")
        env.reset()
        rews, bodies = [], []
        for t in range(steps):
            obs, rew, term, _, info = env.step(acts[t])
            rews.append(rew.clone()); bodies.append(env.body_state().clone())
            env.reset(term)
        env.check_errors()
        out = (torch.stack(bodies), torch.stack(rews), env.obs.clone(), env.info.clone(), env.sched_warnings())
        env.close()
        return out

    try:
        ref = run({"BP_SCHED": "0"})
        got = run({"BP_SCHED_DEBUG_DROP": "1", "BP_SCHED_IMAGE": "1"})
        for a, b in zip(ref[:4], got[:4]):
            assert torch.equal(a, b)
        assert ref[4] == (0, 0)
        assert got[4][0] == steps and got[4][1] == steps          # one watchdog event and one env finished by the completion launch per step
    finally:
        monkeypatch.setattr(_lib, "_lib", None)                   # the next test loads the product library afresh
