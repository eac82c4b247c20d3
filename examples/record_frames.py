"""Record a short ship-ice rollout as images: 8 envs, 50 random steps, one mosaic PNG of the 8 frames per step.

    python examples/record_frames.py [--out frames/] [--scale 10]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv  # noqa: E402
from benchpush_amd.obs_log import write_rgb_png  # noqa: E402
from benchpush_amd.render import tile_images  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="frames")
    ap.add_argument("--scale", type=float, default=10.0, help="pixels per metre (cfg.render_scale is 40)")
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    env = BatchedShipIceEnv(8, cfg={"concentration": 0.3}, num_trials=8)
    env.reset()
    rng = np.random.default_rng(0)
    for t in range(a.steps):
        _, _, term, _, _ = env.step(torch.from_numpy(rng.uniform(-1, 1, 8)))
        frames = env.render_frames(scale=a.scale).cpu().numpy()
        write_rgb_png(os.path.join(a.out, "%03d.png" % t), tile_images(frames))
        if term.any():
            env.reset(term)
    env.close()
    print("wrote %d mosaics to %s" % (a.steps, a.out))


if __name__ == "__main__":
    main()
