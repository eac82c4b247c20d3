"""The planning-based baseline: plan a path, then track it (benchpush/baselines/ship_ice_nav/planning_based in the reference)."""
from .policy import PlanningBasedPolicy

__all__ = ["PlanningBasedPolicy"]
