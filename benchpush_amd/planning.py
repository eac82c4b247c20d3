"""Small helpers for planners that score candidate paths on the device with ``BatchedShipIceEnv.swath_costs``.

Plain torch / numpy, not a hot path: the footprint of the reference's ``Ship`` (common/ship.py:18-20), constant-curvature candidate paths in closed
form, and the replanning comparison of ``Path.update`` (common/utils/utils.py:58-89).  The lattice A* itself (Dubins primitives, pre-rotated swath
dictionaries) is not ported.
"""
import numpy as np
import torch

__all__ = ["ship_footprint", "arc_paths", "replan_mask", "LATTICE_SHIP_VERTICES"]

# ship.vertices of the reference's lattice planner configuration (17 vertices, some collinear); with padding 0.25 and scale 5 it is the planner's footprint
LATTICE_SHIP_VERTICES = [[1., -0.], [0.9, 0.10], [0.5, 0.25], [0.25, 0.25], [0, 0.25], [-0.25, 0.25], [-0.5, 0.25], [-0.75, 0.25], [-1., 0.25],
                         [-1., -0.25], [-0.75, -0.25], [-0.5, -0.25], [-0.25, -0.25], [0, -0.25], [0.25, -0.25], [0.5, -0.25], [0.9, -0.10]]


def ship_footprint(vertices, scale, padding=0.0):
    """``Ship(scale, vertices, padding).vertices``: every coordinate a becomes sign(a) * (|a| + padding) * scale, so a zero coordinate stays zero.
    Returns a float64 numpy array [nv, 2] in cost-map cells (ship facing +x)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 2)
    return np.sign(v) * (np.abs(v) + padding) * scale


def arc_paths(pose, curvature, length, step):
    """Constant-curvature candidate paths: pose [E, 3] = (x, y, theta) in cells / radians, curvature [K] or [E, K] in 1 / cell (positive turns left,
    towards growing theta), arc length `length` sampled every `step` cells from s = 0.  Returns [E, K, P, 3] float64 on pose's device with
    P = floor(length / step) + 1: theta = theta0 + k * s, x = x0 + (sin(theta) - sin(theta0)) / k, y = y0 - (cos(theta) - cos(theta0)) / k, and the
    straight line x0 + s * cos(theta0), y0 + s * sin(theta0) where |k| < 1e-9."""
    pose = torch.as_tensor(pose, dtype=torch.float64)
    if pose.dim() != 2 or pose.shape[1] != 3:
        raise ValueError("arc_paths: pose must be [E, 3]")
    E = pose.shape[0]
    k = torch.as_tensor(curvature, dtype=torch.float64).to(pose.device)
    if k.dim() == 1:
        k = k[None, :].expand(E, k.shape[0])
    if k.dim() != 2 or k.shape[0] != E:
        raise ValueError("arc_paths: curvature must be [K] or [E, K]")
    if not (step > 0 and length >= 0):
        raise ValueError("arc_paths: step must be positive and length non-negative")
    P = int(np.floor(length / step + 1e-9)) + 1
    s = (torch.arange(P, dtype=torch.float64, device=pose.device) * step)[None, None, :]
    x0, y0, th0 = (pose[:, i, None, None] for i in range(3))
    kk = k[:, :, None]
    straight = kk.abs() < 1e-9
    ks = torch.where(straight, torch.ones_like(kk), kk)
    th = th0 + kk * s
    x = torch.where(straight, x0 + s * torch.cos(th0), x0 + (torch.sin(th) - torch.sin(th0)) / ks)
    y = torch.where(straight, y0 + s * torch.sin(th0), y0 - (torch.cos(th) - torch.cos(th0)) / ks)
    return torch.stack([x, y, th.expand_as(x)], dim=-1).contiguous()


def replan_mask(new_cost, old_cost, threshold_cost=0.95):
    """The comparison of ``Path.update``: True where the new path's swath cost is below threshold_cost times the old path's (tensors or arrays of any
    equal shape; both costs taken over the same row window, ``swath_costs(rows=...)``)."""
    return new_cost < old_cost * threshold_cost
