"""rgb_array frames of the four tasks: what the reference ``Renderer`` draws (benchpush/common/utils/renderer.py), restated as exact pixel rules.

A frame is uint8 [H, W, 3], row 0 at the top (pymunk's ``positive_y_is_up``, renderer.py:36).  ``s`` is ``cfg.render_scale`` unless a scale is
given.  World point (x, y) maps to the frame point

    col = (x + tx) * s + cx,    row = cy - (y + ty) * s          (binary64, in this order)

with (tx, ty, cx, cy) per task (``transform``): the debug-draw transform ``Transform.scaling(s)`` with the flip of ``positive_y_is_up``
(renderer.py:44) for ship-ice and maze-NAMO; the same plus the centring translation of ``centered=True`` (renderer.py:46) for area-clearing,
which shifts BOTH axes by env_width / 2 (the reference's quirk, kept); the centred ``to_pygame`` (renderer.py:56-65) of box-delivery's manual
draw (renderer.py:184-200).  Pixel (r, c) is sampled at the point (col c, row r).

* Polygon (3+ vertices): covered where skimage's point_in_polygon rule holds on the transformed vertex columns and rows (``pip_arrays`` of
  the observation kernels; ``oracle.oracle.draw_polygon``).  Vertices are not truncated to int as pygame does.  Polygons are filled without
  outlines; their shape radius is ignored.
* Capsule (segment a -> b, half-width h): covered where dist2 <= h * h, with d = b - a, t = 0 if d.d == 0 else clip(((p - a).d) / (d.d), 0, 1),
  q = a + t d, dist2 = (p - q).(p - q), in binary64 in this order.  Used for maze walls (h = shape radius * s), path segments (0.5), the
  clearance boundary (1.5), the goal line (3, over the full frame width) and the goal disc (a = b, h = goal_radius * s).
* Painter's order: background, layer-0 primitives (the box-delivery receptacle), the shapes -- static shapes, then the movable ones in slot
  order, then the agent's shapes (ship; robot outline, wheels, bumper) -- then the path, then the overlays in ``Renderer.render``'s order
  (goal line, goal region, clearance boundary; renderer.py:179-218).  pymunk draws in Chipmunk's spatial-index order, which nothing here can
  reproduce; this order never hides the agent.

Choices where the frame does not follow pymunk / pygame (neither is a dependency): no outlines, no fat polygon edges, no anti-aliasing;
shapes the reference leaves uncoloured (maze walls, area-clearing walls and obstacles) are drawn in ``UNCOLOURED_STATIC`` = (149, 165, 166).
"""
import ctypes as C

import numpy as np

__all__ = ["TASKS", "PALETTES", "frame_size", "transform", "slot_labels", "render_table", "overlay_prims", "tile_images", "RenderPrim", "RenderArgs",
           "pack_rgb", "PATH_RGB", "PATH_HALF_PX"]

TASKS = ("ship_ice", "maze", "box_delivery", "area_clearing")
UNCOLOURED_STATIC = (149, 165, 166)
PATH_RGB = (255, 0, 0)          # display_planned_path: red, 1 px (renderer.py:83-92)
PATH_HALF_PX = 0.5
WHITE, GREEN = (255, 255, 255), (144, 238, 144)

# colours per shape label and the background of each task
PALETTES = {
    "ship_ice": {"background": (28, 107, 160),      # ship_ice_env.py:487
                 "ice": (173, 216, 230),            # ship_ice_env.py:210
                 "ship": (64, 64, 64)},             # ship_ice_env.py:214
    "maze": {"background": (200, 200, 200),         # maze_NAMO_env.py:602
             "wall": UNCOLOURED_STATIC,             # Segment(radius 0.5) without a colour (sim_utils.py:177-180)
             "box": (204, 153, 102),                # maze_NAMO_env.py:256
             "robot": (100, 100, 100),              # maze_NAMO_env.py:260
             "wheel": (0, 0, 0)},                   # sim_utils.py:50
    "box_delivery": {"background": (234, 234, 234),   # box_delivery_env.py:235
                     "boundary": (140, 155, 155),      # BOUNDARY, sim_utils.py:14: walls, corners, dividers, columns
                     "receptacle": GREEN,              # GREEN, sim_utils.py:11 (box_delivery_env.py:341)
                     "box": (204, 153, 102),           # BOX, sim_utils.py:12
                     "robot": (100, 100, 100),         # AGENT, sim_utils.py:13
                     "wheel": (0, 0, 0),               # create_agent, sim_utils.py:50
                     "bumper": (76, 59, 77)},          # create_agent, sim_utils.py:59
    "area_clearing": {"background": (245, 245, 245),   # area_clearing.py:353-357
                      "obstacle": UNCOLOURED_STATIC,   # walls and static obstacles without a colour (area_clearing.py:445, 472, 505)
                      "box": (204, 153, 102),          # area_clearing.py:393
                      "robot": (100, 100, 100),        # area_clearing.py:376
                      "wheel": (0, 0, 0),              # create_agent, sim_utils.py:50
                      "bumper": (76, 59, 77)},         # create_agent, sim_utils.py:59
}
# draw layer of each label: 0 static, 1 movable, 2 agent
LAYERS = {"wall": 0, "boundary": 0, "obstacle": 0, "receptacle": 0, "ice": 1, "box": 1, "ship": 2, "robot": 2, "wheel": 2, "bumper": 2}


def task_of(env):
    """The task of a batched environment object (its class's ``render_task``)."""
    t = getattr(env, "render_task", None)
    if t not in TASKS:
        raise ValueError("no render task for %r" % type(env).__name__)
    return t


def _scale(cfg, scale):
    s = float(cfg.render_scale if scale is None else scale)
    if not s > 0:
        raise ValueError("render scale must be positive, got %r" % (scale,))
    return s


def _env_extent(task, cfg):
    """(env_width, env_height) in metres that the reference gives its Renderer."""
    if task == "ship_ice":
        return float(cfg.occ.map_width), float(cfg.occ.map_height)            # ship_ice_env.py:486
    if task == "maze":
        return float(cfg.env.width), float(cfg.env.length)                    # maze_NAMO_env.py:601
    if task == "box_delivery":
        from .box_delivery_scenario import room_dims
        L, Wd = room_dims(cfg)[:2]
        t = float(cfg.env.wall_thickness)
        return L + t / 2, Wd + t / 2                                          # box_delivery_env.py:233-235
    if task == "area_clearing":
        from .area_clearing_scenario import env_layout
        ob = env_layout(cfg).outer_boundary
        xs, ys = [p[0] for p in ob], [p[1] for p in ob]
        return float(max(xs) - min(xs)) + 2, float(max(ys) - min(ys)) + 2     # area_clearing.py:353: map_width + 2, map_height + 2
    raise ValueError(task)


def frame_size(task, cfg, scale=None):
    """(H, W) of a frame: int(env_height * s), int(env_width * s) (pygame's window size, renderer.py:31)."""
    s = _scale(cfg, scale)
    ew, eh = _env_extent(task, cfg)
    return int(eh * s), int(ew * s)


def transform(task, cfg, scale=None):
    """(tx, ty, cx, cy) of col = (x + tx) * s + cx, row = cy - (y + ty) * s."""
    s = _scale(cfg, scale)
    ew, eh = _env_extent(task, cfg)
    H, W = frame_size(task, cfg, scale)
    if task in ("ship_ice", "maze"):
        return 0.0, 0.0, 0.0, float(H)
    if task == "area_clearing":
        return ew / 2, ew / 2, 0.0, float(H)          # translated(env_width / 2, env_width / 2), both axes (renderer.py:46)
    return 0.0, 0.0, ew * s / 2, eh * s / 2           # to_pygame, centered (renderer.py:63)


def slot_labels(task, env):
    """Label of every shape slot of the handle (length nb_cap; None = no shape), from the slot layout of the scenario builders."""
    nbcap = int(env.nb_cap)
    lab = [None] * nbcap
    if task == "ship_ice":             # bp_load_scenarios: ship, then the floes (scenario.py)
        lab = ["ship"] + ["ice"] * (nbcap - 1)
    elif task == "maze":               # bp_load_maze: robot outline, wheels, boxes, walls (maze_scenario.py)
        nw = len(env.cfg.robot.wheel_vertices)
        nbox = len(env.layouts[0]["centres"])
        lab = ["robot"] + ["wheel"] * nw + ["box"] * nbox
        lab += ["wall"] * (nbcap - len(lab))
    else:                              # bp_bd_load: agent, 4 wheels, bumper, boxes, statics without the receptacle
        lab = ["robot"] + ["wheel"] * 4 + ["bumper"] + ["box"] * int(env.nbox)
        lab += ["boundary" if task == "box_delivery" else "obstacle"] * (nbcap - len(lab))
    return lab[:nbcap]


def pack_rgb(c):
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


def render_table(task, env):
    """The per-slot table of every trial: dict(labels [nb_cap], rgb uint8 [T, nb_cap, 3], rank int32 [T, nb_cap] (higher = drawn later),
    order int32 [T, nb_cap] (slots bottom first))."""
    pal = PALETTES[task]
    labels = slot_labels(task, env)
    nbcap, T = len(labels), len(env.trials)
    rgb = np.zeros((nbcap, 3), np.uint8)
    rank = np.zeros(nbcap, np.int32)
    for i, l in enumerate(labels):
        rgb[i] = pal[l]
        rank[i] = LAYERS[l] * nbcap + i
    order = np.argsort(rank, kind="stable").astype(np.int32)
    return dict(labels=labels, rgb=np.broadcast_to(rgb, (T, nbcap, 3)).copy(), rank=np.broadcast_to(rank, (T, nbcap)).copy(),
                order=np.broadcast_to(order, (T, nbcap)).copy())


def overlay_prims(task, env):
    """Primitives of the task as dicts: kind 'poly' (world vertices) or 'capsule' (world a, b; half-width half_px + half_world * s), layer 0
    (under the shapes) or 1 (over the shapes and the path), colour."""
    cfg = env.cfg
    out = []
    if task == "ship_ice":             # display_goal_line: white, 6 px, across the window (renderer.py:124-137)
        out.append(dict(kind="capsule", layer=1, rgb=WHITE, v=[(0.0, float(cfg.goal_y)), (float(cfg.occ.map_width), float(cfg.goal_y))],
                        half_px=3.0, half_world=0.0))
    elif task == "maze":               # display_goal_region: filled green disc (renderer.py:139-153)
        g = (float(cfg.env.goal_x), float(cfg.env.goal_y))
        out.append(dict(kind="capsule", layer=1, rgb=GREEN, v=[g, g], half_px=0.0, half_world=float(cfg.goal_radius)))
    elif task == "box_delivery":       # the receptacle: a static polygon labelled 'receptacle' (box_delivery_env.py:338-342), not a physics slot here
        from .box_delivery_scenario import RECEPTACLE
        rec = None
        for t in env.trials:
            verts, counts, poses, _, types = t["statics"]
            k = [i for i in range(len(types)) if types[i] == RECEPTACLE]
            if len(k) != 1 or np.any(poses[k[0]] != 0):
                raise ValueError("box-delivery trials hold one receptacle at the origin pose")
            r = np.asarray(verts[k[0]][: counts[k[0]]], np.float64)
            if rec is not None and not np.array_equal(rec, r):
                raise ValueError("the trials of a box-delivery handle must share one receptacle")
            rec = r
        out.append(dict(kind="poly", layer=0, rgb=PALETTES[task]["receptacle"], v=[tuple(p) for p in rec], half_px=0.0, half_world=0.0))
    else:                              # display_clearance_boundary: green outline, 3 px (renderer.py:167-177)
        from .area_clearing_scenario import env_layout
        b = [(float(p[0]), float(p[1])) for p in env_layout(cfg).boundary]
        for i in range(len(b)):
            out.append(dict(kind="capsule", layer=1, rgb=GREEN, v=[b[i], b[(i + 1) % len(b)]], half_px=1.5, half_world=0.0))
    return out


class RenderPrim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("layer", C.c_int32), ("rgb", C.c_uint32), ("nv", C.c_int32), ("half_px", C.c_double),
                ("half_world", C.c_double), ("v", (C.c_double * 2) * 8)]


class RenderArgs(C.Structure):
    _fields_ = [("scale", C.c_double), ("tx", C.c_double), ("ty", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("width", C.c_int32), ("height", C.c_int32), ("background", C.c_uint32), ("max_path", C.c_int32), ("path_half_px", C.c_double)]


def prim_array(prims):
    arr = (RenderPrim * max(1, len(prims)))()
    for i, p in enumerate(prims):
        arr[i].kind = 0 if p["kind"] == "poly" else 1
        arr[i].layer, arr[i].rgb, arr[i].nv = int(p["layer"]), pack_rgb(p["rgb"]), len(p["v"])
        arr[i].half_px, arr[i].half_world = float(p["half_px"]), float(p["half_world"])
        for q, (x, y) in enumerate(p["v"]):
            arr[i].v[q][0], arr[i].v[q][1] = float(x), float(y)
    return arr


def render_args(task, cfg, scale=None, max_path=0):
    s = _scale(cfg, scale)
    H, W = frame_size(task, cfg, s)
    tx, ty, cx, cy = transform(task, cfg, s)
    return RenderArgs(scale=s, tx=tx, ty=ty, cx=cx, cy=cy, width=W, height=H, background=pack_rgb(PALETTES[task]["background"]),
                      max_path=int(max_path), path_half_px=PATH_HALF_PX)


def tile_images(frames):
    """Mosaic of N frames [N, H, W, 3] (numpy or a list): ceil(sqrt(N)) columns, rows to fit, blank tiles black (SB3's tile_images)."""
    imgs = np.asarray(frames)
    n, h, w, c = imgs.shape
    cols = int(np.ceil(np.sqrt(n)))
    rows = int(np.ceil(float(n) / cols))
    imgs = np.concatenate([imgs, np.zeros((rows * cols - n, h, w, c), imgs.dtype)], axis=0)
    return imgs.reshape(rows, cols, h, w, c).transpose(0, 2, 1, 3, 4).reshape(rows * h, cols * w, c)


def adapter_render(adapter, mode, path, snapshot):
    """render() of the single-env adapters.  mode "rgb_array": numpy [H, W, 3] of env 0 with `path` drawn.  mode "human": there is no window
    backend; the frame is written as a PNG to `snapshot` (where and when the reference saves one) and None returned; without a snapshot a
    warning is issued once per adapter object and None returned."""
    if mode not in ("human", "rgb_array"):
        raise ValueError("render mode must be 'human' or 'rgb_array', got %r" % (mode,))
    if mode == "human" and snapshot is None:
        if not getattr(adapter, "_render_warned", False):
            import warnings
            warnings.warn("%s.render(mode='human'): no window backend exists; use mode='rgb_array' or the configured snapshots" % type(adapter).__name__,
                          RuntimeWarning, stacklevel=3)
            adapter._render_warned = True
        return None
    paths = None if path is None or len(path) == 0 else [np.asarray(path, np.float64)]
    frame = adapter._b.render_frames([0], paths=paths)[0].cpu().numpy()
    if mode == "rgb_array":
        return frame
    import os
    from .obs_log import write_rgb_png
    d = os.path.dirname(snapshot)
    if d:
        os.makedirs(d, exist_ok=True)
    write_rgb_png(snapshot, frame)
    return None


def snapshot_path(cfg, episode_idx, t):
    """<output_dir>/t<episode_idx>/<t>.png (ship_ice_env.py:489-491, maze_NAMO_env.py:604-606, area_clearing.py:1146)."""
    import os
    return os.path.join(str(cfg.output_dir), "t" + str(episode_idx), str(t) + ".png")
