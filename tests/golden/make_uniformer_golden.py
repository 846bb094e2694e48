"""Writes tests/golden/uniformer_vectors.npz: what the REFERENCE's own UniFormer (gyre/pipeline/hinters/models/uniformer.py, loaded from
/root/reference) gives on the CPU in fp32 for the layers-(1,2,2,1), embed-(64,128,192,256) network on seeded weights at 104 x 88 - the
input and the four outputs - and the key names and shapes of the default (uniformer_small) state dict in order.  The weights are
regenerated from the seed (uniformer_ref.seeded_state_dict); their sum of magnitudes is stored to notice a generator that changed.  timm
and mmseg are not installed: the names the file imports from them and the BACKBONES.register_module() decorator are trivial stand-ins.
Build container only:

    python tests/golden/make_uniformer_golden.py"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import uniformer_ref as R  # noqa: E402
from gyre_amd import config as gcfg, weights  # noqa: E402


def reference_module(root="/root/reference"):
    def module(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
    for name in ("timm", "timm.models", "mmseg", "mmseg.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    module("timm.models.layers", DropPath=lambda p=0.0: torch.nn.Identity(),      # (eval mode: stochastic depth is the identity)
           to_2tuple=lambda v: v if isinstance(v, tuple) else (v, v), trunc_normal_=lambda t, std=1.0: torch.nn.init.normal_(t, std=std))
    module("mmseg.utils", get_root_logger=lambda: None)
    module("mmseg.models.builder", BACKBONES=types.SimpleNamespace(register_module=lambda: (lambda cls: cls)))
    spec = importlib.util.spec_from_file_location("ref_uniformer", os.path.join(root, "gyre/pipeline/hinters/models/uniformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    mod = reference_module()
    with contextlib.redirect_stdout(io.StringIO()):                          # (the constructor prints its checkpoint settings)
        full = mod.UniFormer().state_dict()
        model = mod.UniFormer(**R.TINY).eval()
    sd = R.seeded_state_dict(weights.uniformer_param_shapes(gcfg.uniformer_config(**R.TINY)))
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys)
    x = torch.rand((1, 3, 104, 88), generator=torch.Generator().manual_seed(1))
    data = {"keys": np.array(list(full)), "shapes": np.array([",".join(map(str, v.shape)) for v in full.values()]), "x": x.numpy(),
            "weight_l1": np.float64(sum(float(v.double().abs().sum()) for v in sd.values()))}
    with torch.no_grad():
        for i, y in enumerate(model(x)):
            data[f"y{i}"] = y.numpy()
    np.savez_compressed(os.path.join(HERE, "uniformer_vectors.npz"), **data)
    print(len(full), {k: v.shape for k, v in data.items()})
