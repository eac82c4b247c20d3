"""Writes tests/golden/sam_state_dict.json: the parameter names and shapes of the reference's ``DenseActionSpaceDQN`` (benchpush/baselines/
feature_extractors.py) wrapped in ``DataParallel`` as its SAM policy builds it, and the module's float64 CPU output for one input.

Run once, from the repository root, with an interpreter that has torch:

    python tests/golden/make_golden_sam.py /path/to/reference/checkout

The reference module is imported as it is; ``torchvision.models``, ``gymnasium`` and ``stable_baselines3`` -- which the file imports for its other
extractor and which this job calls nothing of -- are stand-ins in ``sys.modules`` where absent.  Only data is recorded:

  names / shapes   ``DataParallel(DenseActionSpaceDQN(num_input_channels=4)).state_dict()``, in its order
  output           ``DenseActionSpaceDQN(num_input_channels=4).double()`` under ``sam_ref.deterministic_fill`` (parameter k of state_dict order becomes
                   u * sqrt(12) * sqrt(2 / fan-in), a bias 0.1 * u, u in [-0.5, 0.5) from an integer hash of (element, k)) applied to ``sam_ref.golden_input()`` (float64 [1, 4, 32, 32], the
                   fractional parts of 0.6180339887 * arange): the [1, 1, 32, 32] result as a flat list of float64 (repr round-trips exactly)."""
import importlib
import importlib.util
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests")]

import sam_ref   # noqa: E402


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sub = ".".join(parts[:i])
        if sub not in sys.modules:
            sys.modules[sub] = types.ModuleType(sub)
        if i > 1:
            setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], sys.modules[sub])
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference_module(ref_root):
    _stub("torchvision.models", resnet18=None)
    _stub("gymnasium", spaces=types.SimpleNamespace(Box=object))
    _stub("stable_baselines3.common.torch_layers", BaseFeaturesExtractor=torch.nn.Module)
    spec = importlib.util.spec_from_file_location("ref_feature_extractors", os.path.join(ref_root, "benchpush", "baselines", "feature_extractors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root):
    ref = load_reference_module(ref_root)
    torch.manual_seed(0)
    wrapped = torch.nn.DataParallel(ref.DenseActionSpaceDQN(num_input_channels=4))
    sd = wrapped.state_dict()
    net = ref.DenseActionSpaceDQN(num_input_channels=4).double()
    sam_ref.deterministic_fill(net)
    with torch.no_grad():
        out = net(sam_ref.golden_input())
    assert tuple(out.shape) == (1, 1, 32, 32) and bool(torch.isfinite(out).all())
    golden = {"names": list(sd.keys()), "shapes": [list(v.shape) for v in sd.values()], "input": "sam_ref.golden_input()",
              "fill": "sam_ref.deterministic_fill", "output_shape": list(out.shape), "output": [float(v) for v in out.reshape(-1).tolist()]}
    path = os.path.join(HERE, "sam_state_dict.json")
    with open(path, "w") as f:
        json.dump(golden, f)
    print("wrote", path, len(golden["names"]), "parameters, output range", float(out.min()), float(out.max()))


if __name__ == "__main__":
    main(sys.argv[1])
