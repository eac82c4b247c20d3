"""ShipIcePPO: the reference's PPO baseline of ship-ice-v0 (benchpush/baselines/ship_ice_nav/ppo/policy.py) on the batched env and the device rollout
buffer.  Network, loss, loop and the deviations from the reference are DevicePPO's (benchpush_amd/baselines/ppo.py); the hyper-parameters are the
reference's ``train()`` defaults (n_steps 256, batch_size 128, n_epochs 10, learning_rate 5e-4, gamma 0.97)."""
from ...ppo import TRAIN_DEFAULTS, DevicePPO

__all__ = ["ShipIcePPO", "TRAIN_DEFAULTS"]


class ShipIcePPO(DevicePPO):
    task = "ship_ice"

    def _make_vec_env(self, num_envs):
        from ....envs.vec_env import make_ship_ice_vec_env
        return make_ship_ice_vec_env(num_envs, cfg=self._env_cfg(), to_numpy=False, **self.env_kwargs)

    def _max_episode_steps(self):
        return 300
