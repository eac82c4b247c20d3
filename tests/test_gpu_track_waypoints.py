"""bp_track_waypoints on the device (-m gpu): the kernel against the restatement (tests/rrt_ref.py) on the poses recorded next to the reference's
``DP.ideal_control``, ``==`` on every output, plus the edge rules."""
import math

import numpy as np
import pytest
import torch

import rrt_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    G, A = R.load_golden(), np.load(R.GOLDEN + "/rrt_golden.npz")
    rows = [(A[t["path"] + "/pruned"], pose) for t in G["track"] for pose in t["poses"]]
    return G, rows


def _env(E):
    from benchpush_amd.envs.maze_namo import BatchedMazeEnv
    env = BatchedMazeEnv(E, num_layouts=1, device="cuda:0")
    env.reset()
    return env


def test_kernel_equals_restatement_on_the_recorded_poses(recorded):
    G, rows = recorded
    E, P = len(rows), max(len(p) for p, _ in rows)
    assert E == 160 and P > 128 and min(len(p) for p, _ in rows) < 64      # paths below one lane round and above two
    paths, lengths, poses = np.zeros((E, P, 2)), np.zeros(E, np.int32), np.zeros((E, 3))
    for e, (p, pose) in enumerate(rows):
        paths[e, :len(p)], lengths[e], poses[e] = p, len(p), pose
    env = _env(E)
    scale = G["action_scale"]
    assert scale == env.max_yaw_rate_step
    actions, diag = env.track_waypoints(torch.from_numpy(paths).cuda(), torch.from_numpy(lengths).cuda(), torch.from_numpy(poses).cuda())
    actions, diag = actions.cpu().numpy(), diag.cpu().numpy()
    want = [R.track_waypoints_ref(p, pose, scale) for p, pose in rows]
    assert np.array_equal(actions, np.array([w[0] for w in want])) and np.array_equal(diag, np.array([w[1] for w in want], np.int32))
    recorded_idx = np.array([i for t in G["track"] for i in t["indices"]], np.int32)
    assert np.array_equal(diag, recorded_idx)                                # the reference's own indices
    worst = np.abs(actions - np.array([a for t in G["track"] for a in t["actions"]])).max()
    print("device against the reference's recorded actions: largest difference %.3g, allowed %.3g" % (worst, R.THETA_TOL / (0.8 * scale)))
    assert worst <= R.THETA_TOL / (0.8 * scale)
    # other tunables, all P counted (lengths None)
    a2, d2 = env.track_waypoints(torch.from_numpy(paths[:, :9].copy()).cuda(), None, torch.from_numpy(poses).cuda(), Lfc=1.3, dt=0.25, action_scale=0.5)
    want2 = [R.track_waypoints_ref(paths[e, :9], poses[e], 0.5, cfg=dict(Lfc=1.3, dt=0.25)) for e in range(E)]
    assert np.array_equal(a2.cpu().numpy(), np.array([w[0] for w in want2])) and np.array_equal(d2.cpu().numpy(), np.array([w[1] for w in want2], np.int32))
    env.close()


def test_edge_rules():
    from benchpush_amd import _lib
    env = _env(6)
    line = np.stack([np.arange(70) * 0.1, np.zeros(70)], 1)
    paths = np.repeat(line[None], 6, 0)
    paths[4, 3, 1] = math.inf                       # a non-finite counted waypoint; env 5 has it past its length
    paths[5, 60, 0] = math.nan
    lengths = np.array([70, 70, 0, 70, 70, 50], np.int32)
    poses = np.array([[0.0, 0.2, 0.3], [100.0, 0.0, 0.0], [1.0, 0.0, 0.0], [math.nan, 0.0, 0.0], [1.0, 0.1, 0.0], [6.9, -0.1, 3.0]])
    active = np.array([1, 0, 1, 1, 1, 1], np.uint8)
    out = (torch.full((6,), 5.0, dtype=torch.float64, device="cuda:0"), torch.full((6, 2), 9, dtype=torch.int32, device="cuda:0"))
    a, d = env.track_waypoints(torch.from_numpy(paths).cuda(), torch.from_numpy(lengths).cuda(), torch.from_numpy(poses).cuda(),
                               torch.from_numpy(active).cuda(), out=out)
    a, d = a.cpu().numpy(), d.cpu().numpy()
    for e in (1, 2, 3, 4):                          # inactive, length 0, non-finite pose, non-finite waypoint: NaN and -1
        assert math.isnan(a[e]) and d[e].tolist() == [-1, -1]
    for e in (0, 5):
        w = R.track_waypoints_ref(paths[e], poses[e], env.max_yaw_rate_step, lengths[e])
        assert a[e] == w[0] and d[e].tolist() == list(w[1])
    assert d[0].tolist() == [0, 5] and d[5].tolist() == [49, 49]     # first waypoint not within Lfc = 0.5; past the end: the last one
    with pytest.raises(ValueError):
        env.track_waypoints(torch.from_numpy(paths).cuda().float())
    with pytest.raises(ValueError):
        env.track_waypoints(torch.from_numpy(paths[:5]).cuda())
    with pytest.raises(_lib.BpError):
        env.track_waypoints(torch.from_numpy(paths).cuda(), dt=0.0)
    env.close()
