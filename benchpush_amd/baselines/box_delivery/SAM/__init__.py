"""The spatial-action-map baseline: a double DQN over a dense per-pixel action space (benchpush/baselines/box_delivery/SAM in the reference)."""
from .policy import BoxDeliverySAM, DenseActionSpacePolicy

__all__ = ["BoxDeliverySAM", "DenseActionSpacePolicy"]
