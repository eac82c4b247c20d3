"""MazeNAMOPPO: the reference's PPO baseline of maze-NAMO-v0 (benchpush/baselines/maze_NAMO/ppo/policy.py) on the batched env and the device rollout
buffer.  Network, loss, loop and the deviations from the reference are DevicePPO's (benchpush_amd/baselines/ppo.py); the hyper-parameters are the
reference's ``train()`` defaults (n_steps 320, batch_size 160, n_epochs 10, learning_rate 5e-4, gamma 0.995)."""
from ...ppo import TRAIN_DEFAULTS, DevicePPO

__all__ = ["MazeNAMOPPO", "TRAIN_DEFAULTS"]


class MazeNAMOPPO(DevicePPO):
    task = "maze_namo"

    def _make_vec_env(self, num_envs):
        from ....envs.vec_env import make_maze_vec_env
        return make_maze_vec_env(num_envs, cfg=self._env_cfg(), to_numpy=False, **self.env_kwargs)

    def _max_episode_steps(self):
        return 400
