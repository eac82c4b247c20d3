"""ShipIceSAC: the reference's SAC baseline of ship-ice-v0 (benchpush/baselines/ship_ice_nav/sac/policy.py) on the batched env and the device transition
buffer.  Networks, losses, loop and the deviations from the reference are DeviceSAC's (benchpush_amd/baselines/sac.py); the hyper-parameters are the
reference's ``train()`` defaults (batch_size 128, buffer_size 15000, learning_starts 200, learning_rate 5e-4, gamma 0.97)."""
from ...sac import TRAIN_DEFAULTS, DeviceSAC

__all__ = ["ShipIceSAC", "TRAIN_DEFAULTS"]


class ShipIceSAC(DeviceSAC):
    task = "ship_ice"

    def _make_vec_env(self, num_envs):
        from ....envs.vec_env import make_ship_ice_vec_env
        return make_ship_ice_vec_env(num_envs, cfg=self._env_cfg(), to_numpy=False, **self.env_kwargs)

    def _max_episode_steps(self):
        return 300
