"""The PPO baseline of maze-NAMO-v0 (benchpush/baselines/maze_NAMO/ppo in the reference)."""
from .policy import MazeNAMOPPO

__all__ = ["MazeNAMOPPO"]
