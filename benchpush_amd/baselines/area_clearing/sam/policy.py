"""AreaClearingSAM: the reference's spatial-action-map baseline of area-clearing-v0 (benchpush/baselines/area_clearing/sam/policy.py) on the batched env
and the ready queue.  Network, replay buffer, learner and schedule are BoxDeliverySAM's (benchpush_amd/baselines/box_delivery/SAM/policy.py, where the
deviations from the reference's loop are listed); the env is a BatchedAreaClearingEnv with position actions whose local map has the layout's
``sam_local_map_pixel_width`` -- what the reference's ``configure_env_for_SAM`` sets.  Whether the batched schedule learns as well as the reference's
one-env loop has not been measured."""
from ...box_delivery.SAM.policy import DenseActionSpacePolicy, SpatialActionMapBaseline

__all__ = ["AreaClearingSAM", "DenseActionSpacePolicy"]


class AreaClearingSAM(SpatialActionMapBaseline):
    task = "area_clearing"

    def _task_cfg(self, c):
        lay = c.envs[c.env]
        lay.local_map_pixel_width = lay.sam_local_map_pixel_width
        return c

    def _make_env(self, num_envs, cfg):
        from ....envs.area_clearing import BatchedAreaClearingEnv
        return BatchedAreaClearingEnv(num_envs, cfg=cfg, **self.env_kwargs)
