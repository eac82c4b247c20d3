"""Baselines of area-clearing-v0 (benchpush/baselines/area_clearing in the reference)."""
