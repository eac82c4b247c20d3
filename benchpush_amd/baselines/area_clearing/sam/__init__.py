"""The spatial-action-map baseline of area-clearing-v0 (benchpush/baselines/area_clearing/sam in the reference)."""
from .policy import AreaClearingSAM

__all__ = ["AreaClearingSAM"]
