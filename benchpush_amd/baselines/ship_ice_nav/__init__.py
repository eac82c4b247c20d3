"""Baselines of ship-ice-v0 (benchpush/baselines/ship_ice_nav in the reference): planning_based, ppo and sac."""
