"""The SAC baseline of ship-ice-v0 (benchpush/baselines/ship_ice_nav/sac in the reference)."""
from .policy import ShipIceSAC

__all__ = ["ShipIceSAC"]
