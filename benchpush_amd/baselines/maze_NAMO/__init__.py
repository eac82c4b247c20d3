"""Baselines of maze-NAMO-v0 (benchpush/baselines/maze_NAMO in the reference): planning_based, ppo and sac."""
