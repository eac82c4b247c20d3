"""The public surface of the env classes as data: tests/golden/env_surface.json records, for each class, its package bases, and for every public
attribute [kind, text, sha256 of the docstring]: the signature of a callable, nothing for a property, the value of a plain class attribute.  A class
that derives from another recorded class lists only what it adds or overrides.  A change of the Python layer that is meant to keep behaviour must
leave this file's comparison green without the fixture being regenerated.

Regenerate (only when the surface is meant to change): ``python tests/test_env_surface_cpu.py``.
"""
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "env_surface.json")
CLASSES = [("ship_ice", "BatchedShipIceEnv"), ("ship_ice", "ShipIceEnv"), ("ship_ice", "LatticeResult"), ("maze_namo", "BatchedMazeEnv"),
           ("maze_namo", "MazeNAMO"), ("box_delivery", "BatchedBoxDeliveryEnv"), ("box_delivery", "BoxDeliveryEnv"), ("box_delivery", "AsyncQueue"),
           ("area_clearing", "BatchedAreaClearingEnv"), ("area_clearing", "AreaClearingEnv"), ("vec_env", "BatchedVecEnv")]   # (bases before subclasses)
# implementation bases that hold shared code and are no part of the class relations that callers test with isinstance
SHARED_BASES = {"_BatchedBase", "_AdapterBase"}


def _sha(doc):
    return None if doc is None else hashlib.sha256(doc.encode()).hexdigest()


def _surface():
    """{class: {"mro": names, "doc": sha, "attrs": {name: [kind, text, doc sha]}}} with every public attribute, inherited ones included."""
    import importlib
    out = {}
    for mod, name in CLASSES:
        cls = getattr(importlib.import_module("benchpush_amd.envs." + mod), name)
        # the classes of benchpush_amd.envs only: the Env base is gymnasium's where that is installed
        mro = [c.__name__ for c in cls.__mro__ if c.__module__.startswith("benchpush_amd.envs") and c.__name__ not in SHARED_BASES]
        attrs = {}
        for a in sorted(n for n in dir(cls) if not n.startswith("_")):
            static = inspect.getattr_static(cls, a)
            if isinstance(static, property):
                attrs[a] = ["property", None, _sha(static.__doc__)]
            elif callable(getattr(cls, a)):
                attrs[a] = ["callable", str(inspect.signature(getattr(cls, a))), _sha(getattr(cls, a).__doc__)]
            else:
                attrs[a] = ["value", repr(static), None]
        out[name] = {"mro": mro, "doc": _sha(cls.__doc__), "attrs": attrs}
    return out


def _expand(fixture):
    """The fixture with the attributes of each class's recorded base (mro[1]) filled in."""
    full = {}
    for _, name in CLASSES:
        rec = fixture[name]
        base = full[rec["mro"][1]]["attrs"] if len(rec["mro"]) > 1 else {}
        full[name] = dict(rec, attrs={**base, **rec["attrs"]})
    return full


def test_env_classes_keep_their_bases_signatures_and_docstrings():
    want = _expand(json.load(open(FIXTURE)))
    got = _surface()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["mro"] == want[name]["mro"], name
        assert got[name]["doc"] == want[name]["doc"], name
        assert sorted(got[name]["attrs"]) == sorted(want[name]["attrs"]), name
        for a, rec in want[name]["attrs"].items():
            assert got[name]["attrs"][a] == rec, (name, a)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    full, lines = _surface(), []
    for _, name in CLASSES:
        rec = full[name]
        base = full[rec["mro"][1]]["attrs"] if len(rec["mro"]) > 1 else {}
        assert set(base) <= set(rec["attrs"])
        attrs = ",\n".join("   %s: %s" % (json.dumps(a), json.dumps(r)) for a, r in rec["attrs"].items() if base.get(a) != r)
        lines.append(' %s: {"mro": %s, "doc": %s, "attrs": {\n%s}}' % (json.dumps(name), json.dumps(rec["mro"]), json.dumps(rec["doc"]), attrs))
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
