"""Baselines of maze-NAMO-v0 (benchpush/baselines/maze_NAMO in the reference)."""
