"""The planning-based baseline: an RRT path, then a look-ahead heading controller (benchpush/baselines/maze_NAMO/planning_based in the reference)."""
from .policy import PlanningBasedPolicy

__all__ = ["PlanningBasedPolicy"]
