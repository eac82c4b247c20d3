"""The PPO baseline of ship-ice-v0 (benchpush/baselines/ship_ice_nav/ppo in the reference)."""
from .policy import ShipIcePPO

__all__ = ["ShipIcePPO"]
