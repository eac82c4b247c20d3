"""k_render on the GPU: frames byte-equal to the independent painter (tests/render_painter.py) for the four tasks, read-only rendering, batch
layout (two envs per wavefront, 64-bit offsets), the adapters' render(), the vector env's get_images() / render(), and argument checks."""
import os
import warnings

import numpy as np
import pytest
import torch

from render_painter import paint, paint_env

pytestmark = pytest.mark.gpu


def _ship(E, **kw):
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials
    return BatchedShipIceEnv(E, cfg={"concentration": 0.3}, trials=default_trials(0.3, 4, base_seed=3), **kw)


def _make(task, E):
    if task == "ship_ice":
        return _ship(E)
    if task == "maze":
        from benchpush_amd.envs.maze_namo import BatchedMazeEnv
        return BatchedMazeEnv(E, num_layouts=4)
    if task == "box_delivery":
        from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
        return BatchedBoxDeliveryEnv(E, num_trials=4)
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    return BatchedAreaClearingEnv(E, num_trials=4)


def _paths(env, ids, rng):
    """A random polyline per frame inside the map (world metres), one of them empty."""
    H, W = env.frame_size(1.0)
    out = []
    for i, _ in enumerate(ids):
        if i == 1:
            out.append(None)
            continue
        n = int(rng.integers(2, 7))
        out.append(np.stack([rng.uniform(-W / 2, W, n), rng.uniform(-H / 2, H, n)], 1))
    return out


@pytest.mark.parametrize("task,E", [("ship_ice", 8), ("maze", 4), ("box_delivery", 4), ("area_clearing", 4)])
def test_frames_equal_painter(task, E):
    env = _make(task, E)
    rng = np.random.default_rng(1)
    env.reset()
    ids = [0, 2, E - 1]
    for t in range(3):
        env.step(torch.from_numpy(rng.uniform(-1, 1, E)))
        if t == 1:
            m = torch.zeros(E, dtype=torch.uint8); m[2] = 1
            env.reset(m)
    s0 = float(env.cfg.render_scale)
    for s in (s0, s0 / 4):
        paths = _paths(env, ids, rng)
        fr = env.render_frames(ids, scale=s, paths=paths).cpu().numpy()
        H, W = env.frame_size(s)
        assert fr.shape == (3, H, W, 3)
        for i, e in enumerate(ids):
            want = paint_env(env, e, scale=s, path=paths[i])
            bad = np.argwhere(np.any(fr[i] != want, axis=2))
            assert len(bad) == 0, "%s env %d scale %g: %d pixels differ, first %s" % (task, e, s, len(bad), bad[:5].tolist())
        assert len(np.unique(fr[0].reshape(-1, 3), axis=0)) >= 3
    env.check_errors()
    env.close()


def test_ship_frame_equals_painter_over_oracle():
    from oracle.oracle import OracleShipIce
    from benchpush_amd import render as R
    env = _ship(2)
    trials = env.trials
    orcs = [OracleShipIce(env.params, env.cfg.ship.vertices, env.cfg.ship.head, env.cfg.ship.tail) for _ in range(2)]
    for e, o in enumerate(orcs):
        o.reset(trials[e % len(trials)])
    env.reset()
    rng = np.random.default_rng(5)
    for _ in range(3):
        a = rng.uniform(-1, 1, 2)
        env.step(torch.from_numpy(a))
        for e, o in enumerate(orcs):
            o.step(float(a[e]))
    fr = env.render_frames([0, 1]).cpu().numpy()
    t = env.render_table()
    for e, o in enumerate(orcs):
        ov, oc = o.world_polys()
        nbc = env.nb_cap
        verts = np.zeros((nbc, 20, 2)); counts = np.zeros(nbc, np.int32)
        assert oc.max() <= 20
        verts[: len(oc)], counts[: len(oc)] = ov[:, :20], oc
        want = paint("ship_ice", env.cfg, env.cfg.render_scale, verts, counts, len(oc), t["order"][0], t["rgb"][0], t["prims"])
        assert np.array_equal(fr[e], want)
    assert R.task_of(env) == "ship_ice"
    env.close()


def test_rendering_is_read_only():
    a, b = _ship(8), _ship(8)
    a.reset(); b.reset()
    rng = np.random.default_rng(2)
    for _ in range(10):
        act = torch.from_numpy(rng.uniform(-1, 1, 8))
        ra = [x.clone() for x in a.step(act)]
        a.render_frames([0, 3, 7], paths=[np.array([[1.0, 1.0], [5.0, 9.0]])] * 3)
        rb = [x.clone() for x in b.step(act)]
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
    assert torch.equal(a.body_state(), b.body_state())
    a.close(); b.close()


def test_two_envs_per_wavefront_last_env():
    env = _ship(5120)
    env.reset()
    env.step(torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, 5120)))
    fr = env.render_frames([5119]).cpu().numpy()
    assert np.array_equal(fr[0], paint_env(env, 5119))
    env.close()


def test_large_batch_64bit_offsets():
    env = _ship(2048)
    env.reset()
    env.step(torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, 2048)))
    ids = list(range(148, 2048))
    H, W = env.frame_size()
    assert len(ids) * H * W * 3 > 2 ** 32
    out = env.render_frames(ids)
    last = out[-1].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    assert np.array_equal(last, paint_env(env, 2047))
    env.close()


def test_adapters_render(tmp_path):
    from benchpush_amd.envs.ship_ice import ShipIceEnv, default_trials
    from benchpush_amd.envs.maze_namo import MazeNAMO
    from benchpush_amd.envs.box_delivery import BoxDeliveryEnv
    from benchpush_amd.envs.area_clearing import AreaClearingEnv
    from benchpush_amd.obs_log import read_png
    env = ShipIceEnv(cfg={"concentration": 0.2, "render_snapshot": True, "output_dir": str(tmp_path)}, trials=default_trials(0.2, 2))
    env.reset()
    env.step(0.3)
    env.update_path(np.array([[6.0, 1.0, 0.0], [6.5, 5.0, 0.0], [5.0, 12.0, 0.0]]))
    rgb = env.render(mode="rgb_array")
    assert np.array_equal(rgb, env._b.render_frames([0], paths=[env.path])[0].cpu().numpy())
    assert np.array_equal(rgb, paint_env(env._b, 0, path=env.path))
    assert env.render() is None
    assert np.array_equal(read_png(os.path.join(str(tmp_path), "t0", "1.png")), rgb)
    env.close()
    for cls, kw in [(MazeNAMO, dict(num_layouts=2)), (BoxDeliveryEnv, dict(num_trials=2)), (AreaClearingEnv, dict(num_trials=2))]:
        e = cls(**kw)
        e.reset()
        e.step(np.array([0.2]))
        fr = e.render(mode="rgb_array")
        assert fr.dtype == np.uint8 and fr.shape == e._b.frame_size() + (3,)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert e.render() is None and e.render() is None
        assert len([x for x in w if issubclass(x.category, RuntimeWarning)]) == 1
        e.close()
    ac = AreaClearingEnv(cfg={"render": {"show": True}, "anim": {"plot_steps": 1}, "output_dir": str(tmp_path / "ac")}, num_trials=2)
    ac.reset()
    ac.step(np.array([0.1]))
    assert ac.render() is None
    assert np.array_equal(read_png(os.path.join(str(tmp_path / "ac"), "t0", "1.png")), ac.render(mode="rgb_array"))
    ac.close()


def test_vec_env_images():
    from benchpush_amd.envs.vec_env import make_ship_ice_vec_env
    from benchpush_amd.render import tile_images
    v = make_ship_ice_vec_env(20, cfg={"concentration": 0.2})
    v.reset()
    imgs = v.get_images()
    H, W = v.env.frame_size()
    assert v.render_mode == "rgb_array" and len(imgs) == 16 and all(i.shape == (H, W, 3) for i in imgs)
    v.render_indices = [3, 19]
    imgs = v.get_images()
    assert np.array_equal(imgs[1], v.env.render_frames([19])[0].cpu().numpy())
    mosaic = v.render()
    assert np.array_equal(mosaic, tile_images(imgs)) and mosaic.shape == (H, 2 * W, 3)
    v.close()


def test_bad_arguments_raise_and_handle_survives():
    from benchpush_amd import _lib
    env = _ship(4)
    with pytest.raises(_lib.BpError):
        env.render_frames([0])           # before reset
    env.reset()
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(_lib.BpError):
            env.render_frames(bad)
    with pytest.raises(_lib.BpError):
        env.render_frames([])
    env.step(torch.zeros(4, dtype=torch.float64))
    assert np.array_equal(env.render_frames([1])[0].cpu().numpy(), paint_env(env, 1))
    env.close()
