"""The SAM baseline's network and learner arithmetic on the CPU: shapes, the reference's parameter names, the reference module's recorded float64 output
(tests/golden/sam_state_dict.json, written by tests/golden/make_golden_sam.py), predict, and the double-DQN target."""
import json
import os

import numpy as np
import torch

import sam_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, "golden", "sam_state_dict.json")) as f:
        return json.load(f)


def test_network_maps_observation_planes_to_one_q_map():
    from benchpush_amd.baselines.feature_extractors import DenseActionSpaceDQN
    torch.manual_seed(0)
    net = DenseActionSpaceDQN(num_input_channels=4)
    out = net(torch.rand(2, 4, 32, 32))
    assert tuple(out.shape) == (2, 1, 32, 32) and bool(torch.isfinite(out).all())
    assert not any(isinstance(m, (torch.nn.BatchNorm2d, torch.nn.GroupNorm, torch.nn.LayerNorm)) for m in net.modules())


def test_state_dict_has_the_reference_names_and_shapes():
    from benchpush_amd.baselines.box_delivery.SAM.policy import DenseActionSpacePolicy
    g = _golden()
    sd = DenseActionSpacePolicy(32 * 32, 4, 0.01, device="cpu").policy_net.state_dict()
    assert list(sd.keys()) == g["names"]
    assert [list(v.shape) for v in sd.values()] == g["shapes"]
    assert g["names"][0] == "module.resnet18.conv1.weight" and g["names"][-1] == "module.conv3.bias"


def test_float64_output_equals_the_reference_modules():
    """Relative 1e-9 per element: summation-order differences of these float64 sums are ~1e-13, any structural difference is O(1)."""
    from benchpush_amd.baselines.feature_extractors import DenseActionSpaceDQN
    g = _golden()
    net = DenseActionSpaceDQN(num_input_channels=4).double()
    sam_ref.deterministic_fill(net)
    with torch.no_grad():
        out = net(sam_ref.golden_input())
    assert list(out.shape) == g["output_shape"]
    got, want = out.reshape(-1).numpy(), np.array(g["output"], np.float64)
    assert want.std() > 1.0, "the fixture exercises the network (a constant map would not)"
    rel = np.abs(got - want) / np.abs(want)
    print("max relative difference", rel.max())
    assert rel.max() <= 1e-9


def test_predict_returns_an_action_index():
    from benchpush_amd.baselines.box_delivery.SAM.policy import DenseActionSpacePolicy
    P = 32
    pol = DenseActionSpacePolicy(P * P, 4, 0.01, device="cpu", random_seed=3)
    obs = np.random.RandomState(0).randint(0, 256, (P, P, 4)).astype(np.uint8)
    for eps in (0.0, 1.0, None):
        action, info = pol.predict(obs, exploration_eps=eps)
        assert type(action) is int and 0 <= action < P * P and info == {}
    a0, _ = pol.predict(obs, 0.0)
    _, dbg = pol.predict(obs, 0.0, debug=True)
    assert tuple(dbg["output"].shape) == (P, P) and int(dbg["output"].reshape(-1).argmax()) == a0
    batch = pol.predict_batch(torch.from_numpy(np.stack([obs, obs[::-1].copy()])), 0.0)
    assert batch.dtype == torch.int64 and tuple(batch.shape) == (2,) and int(batch[0]) == a0
    rnd = pol.predict_batch(torch.from_numpy(np.stack([obs] * 64)), 1.0)
    assert int(rnd.min()) >= 0 and int(rnd.max()) < P * P and len(set(rnd.tolist())) > 8


def test_double_dqn_target_equals_the_numpy_restatement():
    from benchpush_amd.baselines.box_delivery.SAM.policy import double_dqn_target
    reward = np.array([1.0, -0.25, 0.0, 2.5], np.float32)
    ministeps = np.array([1.0, 2.4, 0.0, 7.2], np.float32)
    nonfinal = np.array([1, 0, 1, 1], np.uint8)
    qp = np.array([[0.1, 0.9, 0.3], [0.5, 0.2, 0.1], [0.0, 0.0, 1.0], [0.7, 0.6, 0.8]], np.float32)
    qt = np.array([[10., 20., 30.], [1., 2., 3.], [-4., -5., -6.], [0.5, 0.25, 0.125]], np.float32)
    want = sam_ref.double_dqn_target_np(reward, ministeps, nonfinal, qp, qt, 0.99)
    by_hand = np.array([1.0 + 0.99 ** 1.0 * 20.0, -0.25, -6.0, 2.5 + 0.99 ** 7.2 * 0.125])
    np.testing.assert_allclose(want, by_hand, rtol=1e-6)
    got = double_dqn_target(*[torch.from_numpy(a) for a in (reward, ministeps, nonfinal, qp, qt)], 0.99).numpy()
    # float32, ulp 6e-8: the two pow implementations may each be 2 ulp off (4 between them), two products and a sum add half an ulp each; no cancellation here
    np.testing.assert_allclose(got, want, rtol=5e-7, atol=0)
