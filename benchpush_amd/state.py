"""Saved environment state: what ``save_state`` returns and ``restore_state`` takes (include/benchpush_amd.h: state records).

An ``EnvState`` holds k state records (one fixed-size byte image per env, written and read by the library's pack / unpack kernels) and the matching
rows of the env's output tensors, so that ``env.obs[dst]`` / ``env.info[dst]`` show the restored state without a step.  Wrappers add their own per-env
rows and fields under ``extra``.  Everything is plain tensors and python scalars: ``save`` / ``load`` go through ``torch.save``.
"""
import copy

import numpy as np
import torch

__all__ = ["EnvState", "adapter_save", "adapter_restore"]

_ROWS = ("records", "obs", "reward", "terminated", "truncated", "info", "env_ids")


def _map(x, fn):
    """fn over every tensor of a nest of dicts / lists / tuples; numpy arrays become tensors first, everything else passes through."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if torch.is_tensor(x):
        return fn(x)
    if isinstance(x, dict):
        return {k: _map(v, fn) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_map(v, fn) for v in x]
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


class EnvState:
    """k saved environments.

    records     uint8 [k, state_bytes]   the library's state records
    obs, reward, terminated, truncated, info   rows of the env's output tensors at the time of the save
    env_ids     int32 [k]                the envs the rows were taken from
    layout_id   int                      the saving handle's layout id (a handle with another configuration or other trials refuses the records)
    extra       dict                     per-wrapper additions (BatchedVecEnv: step counters and terminal observations; single-env adapters: their fields)
    """

    def __init__(self, records, obs, reward, terminated, truncated, info, layout_id, env_ids, extra=None):
        self.records, self.obs, self.reward, self.terminated, self.truncated, self.info = records, obs, reward, terminated, truncated, info
        self.layout_id = int(layout_id)
        self.env_ids = env_ids
        self.extra = {} if extra is None else extra

    def __len__(self):
        return int(self.records.shape[0])

    @property
    def device(self):
        return self.records.device

    def _apply(self, fn):
        return EnvState(*[fn(getattr(self, n)) for n in _ROWS[:6]], self.layout_id, fn(self.env_ids), _map(self.extra, fn))

    def to(self, device):
        """A copy on `device` (dtype and shape of every tensor are kept)."""
        return self._apply(lambda t: t.to(device))

    def cpu(self):
        return self.to("cpu")

    def clone(self):
        return self._apply(lambda t: t.clone())

    def save(self, path):
        d = {n: getattr(self, n).cpu() for n in _ROWS}
        # the id is a full 64-bit word: kept as two halves, int64 tensors and some serialisers do not hold values above 2^63
        d["layout_id"] = [self.layout_id & 0xFFFFFFFF, self.layout_id >> 32]
        d["extra"] = _map(self.extra, lambda t: t.cpu())
        d["format"] = "benchpush_amd.EnvState.1"
        torch.save(d, path)

    @classmethod
    def load(cls, path):
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != "benchpush_amd.EnvState.1":
            raise ValueError("%s does not hold an EnvState" % (path,))
        lo, hi = d["layout_id"]
        return cls(*[d[n] for n in _ROWS[:6]], (int(hi) << 32) | int(lo), d["env_ids"], d.get("extra", {}))


def adapter_save(adapter, fields):
    """save_state() of a single-env adapter: the state of its one batched env plus the adapter's own python-side `fields`."""
    s = adapter._b.save_state()
    s.extra["adapter"] = {f: copy.deepcopy(getattr(adapter, f)) for f in fields if hasattr(adapter, f)}
    return s


def adapter_restore(adapter, state, fields):
    """restore_state(s) of a single-env adapter (arrays that went through a file or another device come back as numpy)."""
    adapter._b.restore_state(state, [0])
    saved = state.extra.get("adapter", {})
    for f in fields:
        if f in saved:
            setattr(adapter, f, _map(copy.deepcopy(saved[f]), lambda t: t.cpu().numpy()))
