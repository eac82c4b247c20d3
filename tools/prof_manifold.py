"""Trip counters and cycles of the narrow phase's manifold stage from a -DBP_PROF library, per sub-step, for the mean env and the heaviest 3 %:

    BP_PROF_LIB=<library> python tools/prof_manifold.py [E] [steps] [concentration]

(default 4096 envs, 30 steps of which the last 6 are read, 30 %; BP_PROF_LIB defaults to the -DBP_PROF twin of the tree.)  Slots 50..55 exist from the
side-lane mapping on (DESIGN.md 4g'); an older library leaves them zero.
"""
import os
import sys

os.environ["BP_PROF"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from benchpush_amd.envs.ship_ice import BatchedShipIceEnv, default_trials

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
CONC = float(sys.argv[3]) if len(sys.argv) > 3 else 0.3
LAST, SUB = 6, 400
env = BatchedShipIceEnv(E, cfg={"concentration": CONC}, trials=default_trials(CONC, 100, base_seed=0))
env.reset()
prof = torch.zeros((E, 64), dtype=torch.int64, device=env.device)
env.L.bp_debug_prof(env.h, prof.data_ptr())
g = torch.Generator(device=env.device)
g.manual_seed(1234)
acc = np.zeros((E, 64), np.float64)
for t in range(STEPS):
    a = (torch.rand(E, generator=g, device=env.device, dtype=torch.float64) * 2 - 1).float().double()
    prof.zero_()
    _, _, term, _, _ = env.step(a)
    torch.cuda.synchronize()
    if t >= STEPS - LAST:
        p = prof.cpu().numpy()
        for s in (51, 53, 54):                      # two counts in one slot: low word, high word -> slots s and s + 8 of the accumulator's spare columns
            acc[:, s] += p[:, s] & 0xFFFFFFFF
            acc[:, s + 8] += p[:, s] >> 32
        keep = [k for k in range(56) if k not in (51, 53, 54)]
        acc[:, keep] += p[:, keep]
    env.reset(term)
acc /= LAST * SUB
order = np.argsort(-acc[:, 23])
heavy = order[: max(1, E * 3 // 100)]
cols = (("rounds_with_survivors", 25), ("survivors", 18), ("manifold_trips", 50), ("normal_plane_A", 51), ("normal_plane_B", 59), ("normal_vertex_pair", 52),
        ("query_A", 53), ("query_B", 61), ("support_queries", 39), ("one_point_first", 54), ("one_point_second", 62), ("two_points", 55),
        ("cyc_normal", 31), ("cyc_support", 32), ("cyc_manifold", 10), ("cyc_deliver", 4), ("cyc_substep", 23))
print("%s per sub-step, last %d of %d steps, %d envs at %.0f %%" % (os.path.basename(os.environ.get("BP_PROF_LIB", "libbenchpush_hip_prof.so")), LAST, STEPS, E, 100 * CONC))
for who, rows in (("mean env   ", acc), ("heaviest 3%", acc[heavy])):
    print("  %s " % who + " ".join("%s=%.3f" % (n, rows[:, k].mean()) for n, k in cols))
