"""The planning-based baseline: a GTSP tour over push paths, then a waypoint controller (benchpush/baselines/area_clearing/planning_based in the reference)."""
from .policy import PlanningBasedPolicy

__all__ = ["PlanningBasedPolicy"]
