"""Independent painter of the rgb_array frame (benchpush_amd/render.py states the rules): numpy + the oracle's skimage polygon fill.

The GPU tests compare k_render's frames with `paint` byte for byte; tests/test_render_cpu.py pins the primitives."""
import math

import numpy as np

from oracle.oracle import draw_polygon


def world_to_px(pts, s, tx, ty, cx, cy):
    """(cols, rows) of world points: col = (x + tx) * s + cx, row = cy - (y + ty) * s."""
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    return (p[:, 0] + tx) * s + cx, cy - (p[:, 1] + ty) * s


def polygon_mask(rows, cols, H, W):
    """Pixels of [H, W] covered by the polygon (skimage rule), filled within its bounding box only: the vertices are shifted by the box's
    whole-pixel origin, which is exact in binary64, so the result is the full-frame fill's."""
    r0, c0 = max(0, int(math.floor(rows.min()))), max(0, int(math.floor(cols.min())))
    r1, c1 = min(H - 1, int(math.ceil(rows.max()))), min(W - 1, int(math.ceil(cols.max())))
    mask = np.zeros((H, W), bool)
    if r1 < r0 or c1 < c0:
        return mask
    rr, cc = draw_polygon(rows - r0, cols - c0, (r1 - r0 + 1, c1 - c0 + 1))
    mask[rr + r0, cc + c0] = True
    return mask


def capsule_mask(a, b, h, H, W):
    """Pixels (r, c) with dist2 <= h*h from the point (c, r) to the segment a -> b (a, b = (col, row)), binary64 in the stated order."""
    ax, ay = float(a[0]), float(a[1])
    bx, by = float(b[0]), float(b[1])
    r0, r1 = max(0, int(math.floor(min(ay, by) - h)) - 1), min(H - 1, int(math.ceil(max(ay, by) + h)) + 1)
    c0, c1 = max(0, int(math.floor(min(ax, bx) - h)) - 1), min(W - 1, int(math.ceil(max(ax, bx) + h)) + 1)
    mask = np.zeros((H, W), bool)
    if r1 < r0 or c1 < c0:
        return mask
    py, px = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.float64), np.arange(c0, c1 + 1, dtype=np.float64), indexing="ij")
    dx, dy = bx - ax, by - ay
    dd = dx * dx + dy * dy
    if dd == 0.0:
        t = np.zeros_like(px)
    else:
        t = ((px - ax) * dx + (py - ay) * dy) / dd
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    qx, qy = ax + t * dx, ay + t * dy
    ex, ey = px - qx, py - qy
    mask[r0: r1 + 1, c0: c1 + 1] = ex * ex + ey * ey <= h * h
    return mask


def paint(task, cfg, scale, verts, counts, nb, order, rgb, prims, path=None, alive=None, first_box=6, nbox=0, wall_radius=0.0):
    """The frame of one env.  verts [nb_cap, 20, 2] / counts [nb_cap] = its world_polys() rows, nb its body count, order [nb_cap] / rgb
    [nb_cap, 3] the render table of its trial, prims = render.overlay_prims, path [n, 2] world points or None, alive [24] (box-delivery,
    area-clearing) or None, wall_radius the radius of 2-vertex slots (maze walls)."""
    from benchpush_amd import render as R
    s = float(scale)
    H, W = R.frame_size(task, cfg, s)
    tx, ty, cx, cy = R.transform(task, cfg, s)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = R.PALETTES[task]["background"]

    def fill(mask, colour):
        img[mask] = colour

    def prim(p):
        cols, rows = world_to_px(p["v"], s, tx, ty, cx, cy)
        if p["kind"] == "poly":
            fill(polygon_mask(rows, cols, H, W), p["rgb"])
        else:
            fill(capsule_mask((cols[0], rows[0]), (cols[1], rows[1]), p["half_px"] + p["half_world"] * s, H, W), p["rgb"])

    for p in prims:
        if p["layer"] == 0:
            prim(p)
    for slot in order:
        if slot < 0 or slot >= nb:
            continue
        if alive is not None and first_box <= slot < first_box + nbox and not alive[slot - first_box]:
            continue
        n = int(counts[slot])
        if n < 2:
            continue
        cols, rows = world_to_px(verts[slot, :n], s, tx, ty, cx, cy)
        if n == 2:
            fill(capsule_mask((cols[0], rows[0]), (cols[1], rows[1]), float(wall_radius) * s, H, W), rgb[slot])
        else:
            fill(polygon_mask(rows, cols, H, W), rgb[slot])
    if path is not None and len(path) >= 2:
        cols, rows = world_to_px(np.asarray(path, np.float64)[:, :2], s, tx, ty, cx, cy)
        for i in range(len(cols) - 1):
            fill(capsule_mask((cols[i], rows[i]), (cols[i + 1], rows[i + 1]), R.PATH_HALF_PX, H, W), R.PATH_RGB)
    for p in prims:
        if p["layer"] == 1:
            prim(p)
    return img


def paint_env(benv, e, scale=None, path=None, verts=None, counts=None, nb=None, alive=None):
    """`paint` for env e of a batched environment, from its world_polys(), render_table() and (box-delivery, area-clearing) box_state()."""
    from benchpush_amd import render as R
    task = R.task_of(benv)
    s = float(benv.cfg.render_scale if scale is None else scale)
    if verts is None:
        v, c = benv.world_polys()
        verts, counts = v[e].cpu().numpy(), c[e].cpu().numpy()
    if nb is None:
        nb = int(benv.num_bodies()[e])
    if alive is None and task in ("box_delivery", "area_clearing"):
        alive = benv.box_state()[0][e]
    t = benv.render_table()
    trial = 0   # the table is the same for every trial
    return paint(task, benv.cfg, s, verts, counts, nb, t["order"][trial], t["rgb"][trial], t["prims"], path=path, alive=alive,
                 nbox=int(getattr(benv, "nbox", 0) or 0), wall_radius=benv.params.get("wall_radius", 0.0) if hasattr(benv, "params") else 0.0)
