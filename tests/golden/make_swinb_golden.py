"""Writes tests/golden/swinb_vectors.npz: what the REFERENCE's own SwinTransformer (gyre/pipeline/hinters/inspyrenet/backbones/
SwinTransformer.py, loaded from /root/reference) gives on the CPU in fp32 for the depth-(2,2,2,2), embed-32, heads-(1,2,4,8), window-12
network on seeded weights at 104 x 88 - the input and the five outputs - and the key names and shapes of SwinB()'s state dict in order.
The weights are regenerated from the seed (swinb_ref.seeded_state_dict); their sum of magnitudes is stored to notice a generator that
changed.  timm is not installed: the three names the file imports from it are trivial stand-ins.  Build container only:

    python tests/golden/make_swinb_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import swinb_ref as R  # noqa: E402
from gyre_amd import config as gcfg, weights  # noqa: E402


def reference_module(root="/root/reference"):
    layers = types.ModuleType("timm.models.layers")
    layers.DropPath = lambda p=0.0: torch.nn.Identity()                  # (eval mode: stochastic depth is the identity)
    layers.to_2tuple = lambda v: v if isinstance(v, tuple) else (v, v)
    layers.trunc_normal_ = lambda t, std=1.0: torch.nn.init.normal_(t, std=std)
    for name in ("timm", "timm.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["timm.models.layers"] = layers
    spec = importlib.util.spec_from_file_location("ref_swin_transformer", os.path.join(root, "gyre/pipeline/hinters/inspyrenet/backbones/SwinTransformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    mod = reference_module()
    full = mod.SwinB(pretrained=False).state_dict()
    model = mod.SwinTransformer(window_size=12, **R.TINY)
    model.eval()                                                         # (its train() override returns None)
    sd = R.seeded_state_dict(weights.swinb_param_shapes(gcfg.swinb_config(**R.TINY)))
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("relative_position_index") for k in missing.missing_keys)
    x = torch.rand((1, 3, 104, 88), generator=torch.Generator().manual_seed(1))
    data = {"keys": np.array(list(full)), "shapes": np.array([",".join(map(str, v.shape)) for v in full.values()]), "x": x.numpy(),
            "weight_l1": np.float64(sum(float(v.double().abs().sum()) for v in sd.values()))}
    with torch.no_grad():
        for i, y in enumerate(model(x)):
            data[f"y{i}"] = y.numpy()
    np.savez_compressed(os.path.join(HERE, "swinb_vectors.npz"), **data)
    print(len(full), {k: v.shape for k, v in data.items()})
