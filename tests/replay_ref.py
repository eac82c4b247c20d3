"""numpy model of the device replay buffer (benchpush_amd/replay.py, csrc/bp_replay.hpp): observe / record / sample, the three rules stated once,
row after row in plain loops.  The GPU tests compare every tensor of the device buffer with this model using ==."""
import numpy as np

MASK = (1 << 64) - 1
HELD, ACTED, AWAITS = 1, 2, 4


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def replay_index(seed, draw, b, n):
    """Slot of sample b of draw `draw` among n stored transitions."""
    key = splitmix64((seed & MASK) ^ splitmix64(draw & MASK))
    z = splitmix64(key ^ (b & 0xFFFFFFFF))
    return ((z >> 32) * n) >> 32


class ReplayModel:
    def __init__(self, capacity, num_envs, obs_shape, ministeps_col, seed=0):
        C, E = capacity, num_envs
        self.C, self.E, self.obs_shape, self.mcol, self.seed = C, E, tuple(obs_shape), ministeps_col, seed
        self.state = np.zeros((C,) + self.obs_shape, np.uint8)
        self.next_state = np.zeros((C,) + self.obs_shape, np.uint8)
        self.action = np.zeros(C, np.int32)
        self.reward = np.zeros(C, np.float32)
        self.ministeps = np.zeros(C, np.float32)
        self.nonfinal = np.zeros(C, np.uint8)
        self.env = np.zeros(C, np.int32)
        self.pend_obs = np.zeros((E,) + self.obs_shape, np.uint8)
        self.pend_action = np.zeros(E, np.int32)
        self.pend_flags = np.zeros(E, np.uint8)
        self.hdr = np.zeros(4, np.int64)

    TENSORS = ("state", "next_state", "action", "reward", "ministeps", "nonfinal", "env", "pend_obs", "pend_action", "pend_flags", "hdr")

    def observe(self, ids, obs, reward, terminated, truncated, info, slices):
        for j in range(len(ids)):
            e = int(ids[j])
            if e < 0 or e >= self.E:
                continue
            if slices[j] > 0:
                if self.pend_flags[e] & (HELD | ACTED) == (HELD | ACTED):
                    s = int(self.hdr[0] % self.C)
                    self.state[s] = self.pend_obs[e]
                    self.next_state[s] = obs[j]
                    self.action[s] = self.pend_action[e]
                    self.reward[s] = np.float32(reward[j])
                    self.ministeps[s] = np.float32(info[j, self.mcol])
                    self.nonfinal[s] = 0 if terminated[j] else 1
                    self.env[s] = e
                    self.hdr[0] += 1
                else:
                    self.hdr[2] += 1
            self.pend_obs[e] = obs[j]
            self.pend_flags[e] = HELD | AWAITS

    def record(self, actions, ids, reset=None):
        seen = set()
        for j in range(len(ids)):
            e = int(ids[j])
            if e < 0:
                continue
            ok = e < self.E and e not in seen and bool(self.pend_flags[e] & AWAITS)
            seen.add(e)                       # a smaller row named e: the later ones lose whether or not it was accepted
            if not ok:
                self.hdr[3] += 1
            elif reset is not None and reset[j]:
                self.pend_flags[e] = 0
            else:
                self.pend_action[e] = int(actions[j])
                self.pend_flags[e] = (int(self.pend_flags[e]) | ACTED) & (0xFF ^ AWAITS)

    def sample_slots(self, B):
        n = int(min(self.hdr[0], self.C))
        draw = int(self.hdr[1])
        self.hdr[1] += 1
        if n == 0:
            return None
        return np.array([replay_index(self.seed, draw, b, n) for b in range(B)], np.int64)

    def sample(self, B):
        """dict of the outputs of DeviceReplayBuffer.sample (numpy)."""
        P = self.obs_shape[0]
        s = self.sample_slots(B)
        if s is None:
            z = lambda dt, *sh: np.zeros((B,) + sh, dt)   # noqa: E731
            return dict(state=z(np.float32, 4, P, P), next_state=z(np.float32, 4, P, P), action=z(np.int64), reward=z(np.float32),
                        ministeps=z(np.float32), nonfinal=z(np.uint8), slot=z(np.int32), valid=z(np.uint8))
        img = lambda a: (a[s].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)).astype(np.float32)   # noqa: E731
        return dict(state=img(self.state), next_state=img(self.next_state), action=self.action[s].astype(np.int64), reward=self.reward[s],
                    ministeps=self.ministeps[s], nonfinal=self.nonfinal[s], slot=s.astype(np.int32), valid=np.ones(B, np.uint8))

    def clear_actions(self):
        """What load_state_dict does to the flags."""
        self.pend_flags &= 1
