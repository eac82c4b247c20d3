"""The SAC baseline of maze-NAMO-v0 (benchpush/baselines/maze_NAMO/sac in the reference)."""
from .policy import MazeNAMOSAC

__all__ = ["MazeNAMOSAC"]
