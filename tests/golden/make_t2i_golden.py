"""Build-container script: EXECUTES the reference's T2I-adapter code and records what it computed in t2i_vectors.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_t2i_golden.py

  * gyre/pipeline/t2i_adapter/adapter.py ``Adapter`` / ``Adapter_light`` on synthetic_state_dict(t2i_param_shapes(cfg), seed)
    weights and a seeded 8-bit image [1, c, 64, 96]: the state-dict key names and the four features of each case;
  * unified_pipeline.py ``UnifiedPipelineHint_T2i.standard_call`` and unet/core.py ``UNetWithT2I.__init__`` over a fake model
    that returns recorded states: the u / g / f sums the CFG wrappers receive.

The file holds inputs, seeds, configurations and outputs only; weights are regenerated from the seed (tests/test_t2i_host.py).
Third-party packages the reference imports but this path never runs are stubbed (make_golden._install).  Nothing here ships."""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CASES = [
    ("main_default", dict(type="main", ksize=1, sk=True, use_conv=False, cin=192, nums_rb=2), 11),
    ("main_conv", dict(type="main", ksize=3, sk=False, use_conv=True, cin=64, nums_rb=3, channels=(64, 64, 64, 64)), 12),   # (sk=False: one width, adapter.py:87-99)
    ("light", dict(type="light", cin=192, nums_rb=4), 13),
]
# (name, [(weight, soft_injection, cfg_only, states seed)])
HINTS = [
    ("balanced", [(0.7, False, False, 21)]),
    ("soft", [(0.7, True, False, 21)]),
    ("soft_cfg_only_two", [(0.7, True, True, 21), (1.0, True, False, 22)]),
]
STATE_SHAPES = [(1, 8, 4, 6), (1, 16, 2, 3), (1, 16, 1, 1), (1, 16, 1, 1)]


def image_u8(seed, c):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (1, c, 64, 96), generator=g, dtype=torch.uint8)


def fake_states(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in STATE_SHAPES]


def main():
    import make_golden as mg
    mg._install()
    from gyre.pipeline.t2i_adapter import adapter as A
    from gyre.pipeline import unified_pipeline as UP
    from gyre.pipeline.unet import core as UC
    from gyre_amd import config as gcfg, weights

    out = {}
    for name, kw, seed in CASES:
        cfg = gcfg.tiny_t2i(kw["type"], **{k: v for k, v in kw.items() if k != "type"})
        args = {k: (list(v) if k == "channels" else v) for k, v in cfg.items() if k != "type"}
        net = (A.Adapter_light if cfg.type == "light" else A.Adapter)(**args).eval()
        keys = sorted(net.state_dict().keys())
        net.load_state_dict(weights.synthetic_state_dict(weights.t2i_param_shapes(cfg), seed))
        img = image_u8(seed + 100, cfg.cin // 64)
        with torch.no_grad():
            feats = net(img.float() / 255)
        out[f"{name}.cfg"] = np.array(json.dumps({**cfg, "channels": list(cfg.channels)}))
        out[f"{name}.seed"] = np.array(seed)
        out[f"{name}.keys"] = np.array(keys)
        out[f"{name}.image_u8"] = img.numpy()
        for i, f in enumerate(feats):
            out[f"{name}.f{i}"] = f.numpy()

    class FakeModel:
        def __init__(self, seed):
            self.states = fake_states(seed)

        def __call__(self, image):
            return [s.clone() for s in self.states]

    for name, hints in HINTS:
        objs = []
        for weight, soft, cfg_only, seed in hints:
            h = object.__new__(UP.UnifiedPipelineHint_T2i)
            h.model, h.image, h.mask, h.weight = FakeModel(seed), torch.zeros(1, 3, 8, 8), None, weight
            h.soft_injection, h.cfg_only, h.type, h.fuser = soft, cfg_only, "standard", None
            objs.append(h)
        wrapped = UC.UNetWithT2I(None, objs)
        out[f"hint.{name}.spec"] = np.array(json.dumps(hints))
        for side in ("u", "g", "f"):
            for i, s in enumerate(wrapped.standard_states[side]):
                out[f"hint.{name}.{side}{i}"] = s.numpy()
    for seed in (21, 22):
        for i, s in enumerate(fake_states(seed)):
            out[f"states.{seed}.{i}"] = s.numpy()
    path = os.path.join(HERE, "t2i_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
