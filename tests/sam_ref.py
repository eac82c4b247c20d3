"""Shared by tests/golden/make_golden_sam.py and tests/test_sam_cpu.py: the deterministic weight fill and input under which the reference's
DenseActionSpaceDQN and this project's network are compared in float64, and the numpy restatement of the double-DQN target."""
import math

import numpy as np
import torch


def deterministic_fill(module):
    """Parameter k of state_dict() order with n elements and fan-in f (elements per output unit) becomes u * sqrt(12) * sqrt(2 / f), a bias u * 0.1, with
    u in [-0.5, 0.5) from a 32-bit integer hash of (element index, k) -- exact integer arithmetic, so the fill is the same on every machine; zero mean and
    variance 2 / f keep the activations of order one through all layers (a smooth fill such as a cosine cancels in the sums and leaves only the biases)."""
    M32 = 0xFFFFFFFF
    with torch.no_grad():
        for k, (name, p) in enumerate(module.state_dict().items()):
            n = p.numel()
            x = (torch.arange(n, dtype=torch.int64) * 2654435761 + (k + 1) * 0x9E3779B1) & M32
            for _ in range(2):
                x = ((x ^ (x >> 16)) * 0x45D9F3B) & M32
            x = x ^ (x >> 16)
            u = x.to(torch.float64) / 4294967296.0 - 0.5
            scale = 0.1 if p.dim() == 1 else math.sqrt(12.0) * math.sqrt(2.0 / (n // p.shape[0]))
            p.copy_((u * scale).reshape(p.shape).to(p.dtype))


def golden_input():
    """float64 [1, 4, 32, 32] in [0, 1): the fractional parts of 0.6180339887 * arange."""
    return torch.remainder(0.6180339887 * torch.arange(4 * 32 * 32, dtype=torch.float64), 1.0).reshape(1, 4, 32, 32)


def double_dqn_target_np(reward, ministeps, nonfinal, q_policy_next, q_target_next, gamma):
    """r + gamma ** ministeps * nonfinal * Q_target(s', argmax_a Q_policy(s', a)) on numpy arrays [B] / [B, A]."""
    best = q_policy_next.argmax(axis=1)
    nxt = q_target_next[np.arange(len(best)), best]
    return reward + np.power(np.float32(gamma), ministeps) * nonfinal.astype(np.float32) * nxt
