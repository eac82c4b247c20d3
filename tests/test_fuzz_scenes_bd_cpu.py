"""The scene generator of the box-delivery / area-clearing fuzz (tests/fuzz_scenes_bd.py) on its own, no GPU: 40 scenes per layout, two layouts per task.
Every family is there, the constructed contacts are what their records say (parallel to within the stated angle, vertex to vertex at the stated gap,
straddling the edge they name), every centre is inside the range the reference draws from, and the oracle alone plays every scene for three steps
with a finite state."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzz_scenes_bd as F  # noqa: E402
from fuzz_scenes_bd import ANGLES, BOX_R, EDGE_OFFS, GAPS, box_corners  # noqa: E402

N = 40
LAYOUTS = ["bd-small_columns-heading", "bd-large_divider-heading", "ac-clear_env_small-heading", "ac-walled_env-heading"]


@pytest.fixture(scope="module", params=LAYOUTS)
def batch(request):
    case = request.param
    cfg, over, scenes, actions, make_oracle = F.case_setup(case, nscenes=N)
    return case, cfg, scenes, actions, make_oracle


def _half(case, cfg):
    return float(cfg.boxes.box_size) / 2 if case.startswith("bd") else float(cfg.obstacle_size)


def _angle(e, f):
    return abs(math.atan2(e[0] * f[1] - e[1] * f[0], e @ f))


def test_every_family_is_present_and_every_centre_is_in_range(batch):
    case, cfg, scenes, _, _ = batch
    assert len(scenes) == N and [s["fuzz"]["family"] for s in scenes] == [i % 4 for i in range(N)]
    half = _half(case, cfg)
    if case.startswith("bd"):
        L, W = 10.0, 5.0 if "small" in case else 10.0
        lo, hi = np.array([-L / 2 + half, -W / 2 + half]), np.array([L / 2 - half, W / 2 - half])      # generate_boxes' own draw
        slo, shi = np.array([-L / 2 + 0.92, -W / 2 + 0.92]), np.array([L / 2 - 0.92, W / 2 - 0.92])    # get_random_robot_start's
        nbox = 10 if "small" in case else 20
    else:
        out, inn = (6.0, 4.0) if "small" in case else (8.0, 5.0)
        lo, hi = np.array([-out + half] * 2), np.array([out - half] * 2)
        slo, shi = np.array([-inn + 0.5] * 2), np.array([inn - 0.5] * 2)
        nbox = 10
    for s in scenes:
        assert s["boxes"].shape == (nbox, 3) and np.isfinite(s["boxes"]).all() and np.isfinite(s["start"]).all()
        assert (s["boxes"][:, :2] >= lo).all() and (s["boxes"][:, :2] <= hi).all()
        assert (s["start"][:2] >= slo).all() and (s["start"][:2] <= shi).all()
    for s in scenes[1::4]:      # family 1: the re-centred boxes are on the robot
        k = s["fuzz"]["constructs"][0]["boxes"]
        assert 1 <= len(k) <= 4
        assert (np.linalg.norm(s["boxes"][k, :2] - s["start"][:2], axis=1) <= (0.6 if case.startswith("bd") else 1.0) + 1e-12).all()
    heads = np.concatenate([s["boxes"][:, 2] for s in scenes[0::4]])
    assert heads.min() < 0.5 and heads.max() > 2 * math.pi - 0.5      # family 0: any heading (area-clearing's own generator only knows 0)


def test_constructed_contacts_are_what_they_claim(batch):
    case, cfg, scenes, _, _ = batch
    half = _half(case, cfg)
    angs, gaps, kinds = [], [], set()
    for s in scenes[2::4]:
        for c in s["fuzz"]["constructs"]:
            kinds.add(c["kind"])
            v = [box_corners(s["boxes"][k], half) for k in c["boxes"]]
            if c["kind"] == "pair":
                a = _angle(v[0][1] - v[0][0], v[1][1] - v[1][0])
                d = s["boxes"][c["boxes"][1], :2] - s["boxes"][c["boxes"][0], :2]
                phi = s["boxes"][c["boxes"][0], 2]
                assert abs(d @ np.array([math.cos(phi), math.sin(phi)]) - (2 * half + 2 * BOX_R + c["gap"])) < 1e-13     # face to face at the stated gap
                assert 0.2 * 2 * half - 1e-9 <= abs(d @ np.array([-math.sin(phi), math.cos(phi)])) <= 0.8 * 2 * half + 1e-9   # partial tangential overlap
            elif c["kind"] in ("wall", "face"):
                t = np.array([-math.sin(c["normal"]), math.cos(c["normal"])])
                a = _angle(v[0][0] - v[0][3], t)        # the box's +x face against the wall's tangent
            elif c["kind"] == "vertex":
                tip_a = v[0][0]                                                  # the (+half, +half) corner of the first box
                d = np.linalg.norm(v[1] - tip_a, axis=1).min()
                assert abs(d - math.hypot(2 * BOX_R + c["gap"], c["lateral"])) < 1e-9, (c, d)     # the second box may be turned by 1e-9: its corner moves by 3e-10
                continue
            else:
                continue
            assert c["angle"] in ANGLES and c["gap"] in GAPS
            assert abs(a - c["angle"]) < 2e-14 + 1e-9 * c["angle"], (c, a)       # parallel up to the rounding of the corner coordinates
            angs.append(a); gaps.append(c["gap"])
    want = {"wall", "face", "pair", "vertex", "corner"} | ({"wall_end"} if "walled" in case else set())
    assert kinds == want
    angs, gaps = np.array(angs), np.array(gaps)
    assert (angs < 1e-13).sum() >= 2 and ((angs > 1e-13) & (angs < 1e-8)).sum() >= 2 and (angs > 1e-5).sum() >= 2
    assert (np.abs(gaps) <= 1e-12).any() and (gaps < 0).any() and (gaps > 0).any()     # touching to within rounding, overlapping, apart
    for s in scenes[2::4]:
        c = [c for c in s["fuzz"]["constructs"] if c["kind"] == "corner"][0]
        v = box_corners(s["boxes"][c["boxes"][0]], half) - np.array(c["corner"])
        if case.startswith("bd"):   # the box's nearest corner is `gap` from the rounded surface of the middle corner triangle's inner edge (x - y = 1 + S - C)
            from benchpush_amd.box_delivery_scenario import _C, _S
            along = v @ (np.array(c["diagonal"]) / math.sqrt(2))
            assert abs(along.min() - ((1 + _S - _C) / math.sqrt(2) + 0.02 + BOX_R + c["gap"])) < 1e-12 and -0.03 <= c["gap"] <= 1e-4
        else:                       # the box touches both walls of the outer corner (radius 0.1) to within `gap`
            assert np.allclose(np.abs(s["boxes"][c["boxes"][0], :2] - np.array(c["corner"])), 0.1 + BOX_R + half + c["gap"], rtol=0, atol=1e-12)


def test_task_edges_are_what_they_claim(batch):
    case, cfg, scenes, _, _ = batch
    half = _half(case, cfg)
    offs = []
    for s in scenes[3::4]:
        cons = s["fuzz"]["constructs"]
        if case.startswith("bd"):
            L, W = 10.0, 5.0 if "small" in case else 10.0
            assert [c["kind"] for c in cons] == ["straddle", "straddle", "inside", "bumper"]
            for c in cons[:2]:
                v = box_corners(s["boxes"][c["boxes"][0]], half)
                assert c["edge"] == (L / 2 if c["axis"] == 0 else W / 2) - 1.5
                assert v[:, c["axis"]].min() < c["edge"] < v[:, c["axis"]].max()                 # corners on both sides of the receptacle's edge
                assert (v[:, 1 - c["axis"]] > (W / 2 if c["axis"] == 0 else L / 2) - 1.5).all()    # ... within the edge's own extent
                offs.append(c["off"])
            for k in cons[2]["boxes"]:
                v = box_corners(s["boxes"][k], half)
                assert (v[:, 0] > L / 2 - 1.5).all() and (v[:, 0] < L / 2).all() and (v[:, 1] > W / 2 - 1.5).all() and (v[:, 1] < W / 2).all()
            st, b = s["start"], s["boxes"][cons[3]["boxes"][0]]
            fwd = np.array([math.cos(st[2]), math.sin(st[2])])
            assert abs((b[:2] - st[:2]) @ fwd - (0.31 + 2 * BOX_R + half + cons[3]["gap"])) < 1e-12      # bumper front 0.31, both shapes rounded by 0.02
            to_recept = np.array([L / 2 - 0.75, W / 2 - 0.75]) - st[:2]
            assert _angle(fwd, to_recept) <= 0.05 + 1e-12
        else:
            inn = 4.0 if "small" in case else 5.0
            out = 6.0 if "small" in case else 8.0
            assert [c["kind"] for c in cons] == ["centre_on_edge"] * 4 + ["face_on_edge"] * 2 + ["outside", "outer_corner"]
            for c in cons[:6]:
                p0, nrm = np.array(c["p0"]), np.array(c["normal"])
                assert abs(abs(p0 @ nrm) - inn) < 1e-12 and c["off"] in EDGE_OFFS
                sd = (box_corners(s["boxes"][c["boxes"][0]], half) - p0) @ nrm      # signed distance of the corners from the edge's line, outward
                if c["kind"] == "centre_on_edge":
                    assert abs((s["boxes"][c["boxes"][0], :2] - p0) @ nrm - c["off"]) < 1e-13 and sd.min() < 0 < sd.max()
                else:
                    assert abs(sd.min() - c["off"]) < 1e-13 and (np.sort(sd)[2:] > 2 * half - 2e-3).all()   # the inner face on the line, the box outside
                offs.append(c["off"])
            v = box_corners(s["boxes"][cons[6]["boxes"][0]], half)
            assert (np.abs(v).max(axis=1) > inn).all() and ((v > inn).all(axis=0).any() or (v < -inn).all(axis=0).any())   # beyond one edge's line: outside
            b = s["boxes"][cons[7]["boxes"][0]]
            assert np.allclose(np.abs(b[:2]), out - 0.1 - BOX_R - half - cons[7]["gap"], rtol=0, atol=1e-12)
    offs = np.array(offs)
    assert (offs > 0).any() and (offs < 0).any() and (case.startswith("bd") or (offs == 0).any())


def test_oracle_alone_plays_every_scene(batch):
    case, cfg, scenes, actions, make_oracle = batch
    ref = F.oracle_case(make_oracle, scenes, actions, observe=False)
    nbox = len(scenes[0]["boxes"])
    for e, r in enumerate(ref):
        assert len(r["steps"]) == F.STEPS
        for info, rew, term, trunc, st, alive in r["steps"]:
            assert st.shape == (6 + nbox, 9) and np.isfinite(st).all() and np.isfinite(info).all() and math.isfinite(rew), (case, e)
    seen = F.teeth(F.CASES[case][0], ref)
    assert seen["work"] >= N // 2 and seen["limited"] >= N and seen["task"] >= 1, seen
