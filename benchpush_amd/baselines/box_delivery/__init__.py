"""Baselines of box-delivery-v0 (benchpush/baselines/box_delivery in the reference)."""
