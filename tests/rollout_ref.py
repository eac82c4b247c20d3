"""numpy model of the device rollout buffer (benchpush_amd/rollout.py, csrc/bp_rollout.hpp): begin / pick_rows / end / finish / minibatch, every rule stated
once in plain loops.  The GPU tests compare every tensor of the device buffer with this model using ==."""
import numpy as np

from replay_ref import MASK, splitmix64

F = np.float32


def rollout_index(seed, epoch, i, n):
    """Position i of epoch `epoch`'s permutation of range(n): 4-round balanced Feistel network over 2h bits, 4^h >= n, walked until below n."""
    h = 0
    while (1 << (2 * h)) < n:
        h += 1
    mask = (1 << h) - 1
    key = splitmix64((seed & MASK) ^ splitmix64(epoch & MASK))
    x = i
    while True:
        left, right = x >> h, x & mask
        for r in range(4):
            f = (splitmix64(key ^ ((r << 32) | right)) >> 32) & mask
            left, right = right, left ^ f
        x = (left << h) | right
        if x < n:
            return x


def gae(reward, value, episode_start, last_values, last_done, gamma, gae_lambda):
    """(advantage, ret) float32 [T, E]: stable-baselines3's compute_returns_and_advantage as an explicit float32 loop, one operation at a time."""
    T, E = reward.shape
    g, gl = F(gamma), F(np.float64(gamma) * np.float64(gae_lambda))
    adv, ret = np.zeros((T, E), F), np.zeros((T, E), F)
    one = F(1)
    for e in range(E):
        a = F(0)
        for t in range(T - 1, -1, -1):
            if t == T - 1:
                nn, v_next = one - F(1 if last_done[e] else 0), F(last_values[e])
            else:
                nn, v_next = one - F(1 if episode_start[t + 1, e] else 0), value[t + 1, e]
            delta = F(F(reward[t, e] + F(F(g * v_next) * nn)) - value[t, e])
            a = F(delta + F(F(gl * nn) * a))
            adv[t, e] = a
            ret[t, e] = F(a + value[t, e])
    return adv, ret


def image(rows):
    """uint8 -> float32 by IEEE division on the host."""
    return (rows.astype(np.float32) / np.float32(255.0)).astype(np.float32)


class RolloutModel:
    TENSORS = ("obs", "action", "reward", "value", "logp", "advantage", "ret", "episode_start", "last_done", "hdr")

    def __init__(self, n_steps, num_envs, obs_shape, action_dim, gamma, gae_lambda, seed=0):
        T, E, A = n_steps, num_envs, action_dim
        self.T, self.E, self.A, self.obs_shape, self.gamma, self.gae_lambda, self.seed = T, E, A, tuple(obs_shape), gamma, gae_lambda, seed
        self.obs = np.zeros((T, E) + self.obs_shape, np.uint8)
        self.action = np.zeros((T, E, A), F)
        self.reward, self.value, self.logp, self.advantage, self.ret = (np.zeros((T, E), F) for _ in range(5))
        self.episode_start, self.last_done, self.hdr = np.zeros((T, E), np.uint8), np.zeros(E, np.uint8), np.zeros(2, np.int64)

    def begin(self, t, obs, action, value, logp):
        self.obs[t], self.action[t], self.value[t], self.logp[t] = obs, np.asarray(action, F).reshape(self.E, self.A), value, logp
        self.episode_start[t] = self.last_done != 0

    def pick_rows(self, mask, src, K):
        """(ids int32 [K], rows float32 [K, *obs_shape]): ascending compaction of the masked envs, the overflow counted in hdr[0]."""
        ids, rows = np.full(K, -1, np.int32), np.zeros((K,) + self.obs_shape, F)
        k = 0
        for e in range(self.E):
            if mask[e]:
                if k < K:
                    ids[k], rows[k] = e, image(src[e])
                else:
                    self.hdr[0] += 1
                k += 1
        return ids, rows

    def end(self, t, reward, done, boot_ids=None, boot_values=None):
        for e in range(self.E):
            self.reward[t, e] = F(reward[e])
            self.last_done[e] = 1 if done[e] else 0
        if boot_ids is not None:
            g = F(self.gamma)
            for k in range(len(boot_ids)):
                e = int(boot_ids[k])
                if 0 <= e < self.E:
                    self.reward[t, e] = F(self.reward[t, e] + F(g * F(boot_values[k])))
        self.hdr[1] += self.E

    def finish(self, last_values):
        self.advantage, self.ret = gae(self.reward, self.value, self.episode_start, last_values, self.last_done, self.gamma, self.gae_lambda)

    def minibatch(self, epoch, j, B):
        """dict of the outputs of bp_rollout_minibatch (numpy)."""
        N = self.T * self.E
        out = dict(obs=np.zeros((B,) + self.obs_shape, F), action=np.zeros((B, self.A), F), value=np.zeros(B, F), logp=np.zeros(B, F),
                   advantage=np.zeros(B, F), ret=np.zeros(B, F), index=np.zeros(B, np.int32), valid=np.zeros(B, np.uint8))
        for b in range(B):
            pos = j * B + b
            if pos >= N:
                continue
            i = rollout_index(self.seed, epoch, pos, N)
            t, e = divmod(i, self.E)
            out["index"][b], out["valid"][b] = i, 1
            out["obs"][b], out["action"][b] = image(self.obs[t, e]), self.action[t, e]
            for n in ("value", "logp", "advantage", "ret"):
                out[n][b] = getattr(self, n)[t, e]
        return out
