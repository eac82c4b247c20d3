"""State records without a GPU: the C ABI surface, the pure layout helper and EnvState's (de)serialisation."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bp_state_bytes", "bp_state_layout_id", "bp_save_state", "bp_load_state", "bp_clone_state")


@pytest.fixture(scope="module")
def lib():
    from benchpush_amd import _lib
    from benchpush_amd.build import build_hip
    build_hip()
    return _lib.load()


def test_header_declares_and_library_exports_the_state_entry_points(lib):
    from benchpush_amd import _lib
    header = open(os.path.join(ROOT, "include", "benchpush_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)           # declarations only, comments stripped
    for name in NEW + ("bp_state_layout_query",):
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared in the header"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.EXPORTS
    assert re.search(r"#define\s+BP_STATE_TRUSTED\s+1\b", code)
    assert lib.bp_abi_version() == 11                              # additive: the ABI version does not move


def test_null_handle_is_refused_without_a_crash(lib):
    assert lib.bp_state_bytes(None) < 0
    assert lib.bp_state_layout_id(None) == 0
    assert lib.bp_save_state(None, None, 1, None, None) < 0
    assert lib.bp_load_state(None, None, 1, None, 0, None) < 0
    assert lib.bp_clone_state(None, None, None, 1, 0, None) < 0
    assert lib.bp_load_state(None, None, 1, None, 1, None) < 0     # BP_STATE_TRUSTED skips the id checks, not the handle check


SHAPES = [(0, 0, 264, 0), (0, 0, 8, 0), (0, 0, 136, 0), (1, 0, 40, 0), (2, 0, 24, 96 * 96), (2, 1, 40, 97 * 101)]


@pytest.mark.parametrize("kind,task,nbcap,cells", SHAPES)
def test_segment_layout_is_aligned_disjoint_and_complete(lib, kind, task, nbcap, cells):
    from benchpush_amd import _lib
    lay = _lib.state_layout(kind, nbcap, task=task, map_cells=cells)
    off, nbytes, width = lay["offsets"], lay["bytes"], lay["widths"]
    assert len(off) >= 40 and off[0] == 0 and nbytes[0] == 32      # the header is segment 0
    assert np.all(off % 16 == 0)
    assert np.all(nbytes > 0)
    # in record order, back to back with less than 16 bytes of padding: no overlap, no hole
    assert np.array_equal(off[1:], off[:-1] + (nbytes[:-1] + 15) // 16 * 16)
    assert lay["total"] == off[-1] + (nbytes[-1] + 15) // 16 * 16 and lay["total"] % 16 == 0
    # the widest safe access divides the bytes of one env slot (every array starts on an allocation boundary, so env * bytes keeps that alignment)
    assert set(width.tolist()) <= {1, 2, 4, 8, 16}
    assert np.all(nbytes % width == 0)
    assert np.all((nbytes % (2 * width) != 0) | (width == 16))     # ... and it is the widest one
    # the arrays whose size the body capacity decides: 2 + 1 + 2 + 2 + 2 + 2 doubles, 3 x 20 vertices, 2 boxes, 24 neighbour slots (u16 + u64), 1 count byte
    per_body = 8 * 11 + 3 * 20 * 16 + 2 * 32 + 24 * (2 + 8) + 1
    rest = sum(int(n) for n in nbytes) - per_body * nbcap - 4 * cells
    assert 0 < rest < 16 * 1024                                    # header, arbiter slots, scalars, metrics, box bookkeeping: independent of the capacities
    if kind == 2:
        assert 4 * cells in nbytes.tolist()                        # the robot's distance map (observation channel 2)


def test_adjn_width_follows_the_body_capacity(lib):
    """adjn is one byte per body slot and the capacity only a multiple of 8: odd env slots are 8-byte aligned, so that segment must not be copied 16 bytes wide."""
    from benchpush_amd import _lib
    for nbcap, want in ((264, 8), (256, 16), (8, 8), (48, 16)):
        lay = _lib.state_layout(0, nbcap)
        idx = [i for i, n in enumerate(lay["bytes"]) if n == nbcap]
        assert idx, "no one-byte-per-body segment"
        assert all(lay["widths"][i] == want for i in idx), (nbcap, lay["widths"][idx])


def test_layout_id_depends_on_the_shapes(lib):
    from benchpush_amd import _lib
    a, b = _lib.state_layout(0, 264), _lib.state_layout(0, 272)
    assert a["structure_id"] != b["structure_id"] and a["total"] != b["total"]
    assert _lib.state_layout(0, 264)["structure_id"] == a["structure_id"]          # a pure function
    assert _lib.state_layout(1, 264)["structure_id"] != a["structure_id"]          # env kind
    c, d = _lib.state_layout(2, 24, task=0, map_cells=9216), _lib.state_layout(2, 24, task=1, map_cells=9216)
    assert c["structure_id"] != d["structure_id"] and c["total"] == d["total"]     # task
    assert _lib.state_layout(2, 24, task=0, map_cells=9217)["structure_id"] != c["structure_id"]


def test_layout_query_refuses_bad_shapes(lib):
    q = lambda *a: lib.bp_state_layout_query(*a, 0, None, None, None, None, None)   # noqa: E731
    assert q(0, 0, 264, 0) > 0
    assert q(0, 0, 263, 0) < 0      # capacities are multiples of 8
    assert q(0, 0, 0, 0) < 0
    assert q(3, 0, 264, 0) < 0      # no such env kind
    assert q(2, 0, 24, 0) < 0       # a box handle has a map
    assert q(0, 0, 264, 5) < 0      # the others have none


def _state(k=3, nbytes=64):
    from benchpush_amd.state import EnvState
    g = torch.Generator().manual_seed(3)
    return EnvState(records=torch.randint(0, 256, (k, nbytes), dtype=torch.uint8, generator=g),
                    obs=torch.randint(0, 256, (k, 4, 6, 5), dtype=torch.uint8, generator=g),
                    reward=torch.rand(k, dtype=torch.float64, generator=g),
                    terminated=torch.tensor([0, 1, 0], dtype=torch.uint8), truncated=torch.tensor([0, 0, 1], dtype=torch.uint8),
                    info=torch.rand((k, 16), dtype=torch.float64, generator=g), layout_id=0xFEDCBA9876543210,
                    env_ids=torch.tensor([5, 2, 7], dtype=torch.int32),
                    extra={"vec_steps": torch.tensor([4, 0, 9]), "adapter": {"t": 3, "total_work": [1.5, [0.5, 1.0]], "path": None,
                                                                             "obstacles": [np.arange(6.0).reshape(3, 2), np.ones((4, 2))]}})


def _same(a, b):
    for n in ("records", "obs", "reward", "terminated", "truncated", "info", "env_ids"):
        x, y = getattr(a, n), getattr(b, n)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), n
    assert a.layout_id == b.layout_id and len(a) == len(b)


def test_envstate_round_trips_through_a_file(tmp_path):
    from benchpush_amd.state import EnvState
    s = _state()
    p = str(tmp_path / "state.pt")
    s.save(p)
    r = EnvState.load(p)
    _same(s, r)
    assert r.layout_id == 0xFEDCBA9876543210                      # all 64 bits survive
    assert torch.equal(r.extra["vec_steps"], s.extra["vec_steps"])
    ad = r.extra["adapter"]
    assert ad["t"] == 3 and ad["total_work"] == [1.5, [0.5, 1.0]] and ad["path"] is None
    assert all(np.array_equal(np.asarray(x), y) for x, y in zip(ad["obstacles"], s.extra["adapter"]["obstacles"]))
    torch.save({"something": 1}, p)
    with pytest.raises(ValueError):
        EnvState.load(p)


def test_envstate_to_keeps_dtype_and_shape():
    s = _state()
    for r in (s.to("cpu"), s.cpu(), s.clone()):
        _same(s, r)
        assert r.device == torch.device("cpu")
        assert r.extra["vec_steps"].dtype == torch.int64
    c = s.clone()
    c.records.zero_()
    assert s.records.any()                                          # a clone owns its tensors
