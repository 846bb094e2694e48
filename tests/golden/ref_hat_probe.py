"""Build-container probe: the REFERENCE's own HAT (gyre/pipeline/upscalers/models/hat_arch.py, loaded from /root/reference by file
path) against tests/hat_ref.py and gyre_amd on the same synthetic weights.

The file imports three names from ``basicsr``, which is not installed here; they are satisfied by stand-in modules
(``ARCH_REGISTRY.register()`` -> an identity decorator, ``to_2tuple``, ``trunc_normal_`` -> a no-op: every parameter is overwritten by
load_state_dict) - the network arithmetic is the reference's own code; ``einops`` is installed.  upscaler_loader.py is loaded the same
way for its DEFAULT_CONFIGS.

reference_outputs() is also what tests/golden/make_hat_golden.py stores.  Prints one JSON object.  Run by
tests/test_reference_hat.py; nothing here ships."""
import importlib.util
import json
import os
import sys
import types

import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hat_ref as R  # noqa: E402
from gyre_amd import config as gcfg, upscaler as U, weights  # noqa: E402

# (model case of hat_ref.MODEL_CASES, image shape)
CASES = [("tiny", (1, 3, 16, 32)), ("tiny2", (1, 3, 32, 48))]
CTOR = ("img_size", "in_chans", "embed_dim", "depths", "num_heads", "window_size", "compress_ratio", "squeeze_factor", "conv_scale",
        "overlap_ratio", "mlp_ratio", "upscale", "img_range", "upsampler", "resi_connection")


def stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Anything:
    def __init__(self, *a, **k):
        pass


class Registry:
    def register(self):
        return lambda cls: cls


def reference_modules():
    for pkg in ("basicsr", "basicsr.utils", "basicsr.archs"):
        stand_in(pkg)
    stand_in("basicsr.utils.registry", ARCH_REGISTRY=Registry())
    stand_in("basicsr.archs.arch_util", to_2tuple=lambda v: v if isinstance(v, tuple) else (v, v), trunc_normal_=lambda t, std=1.0: t)
    hat = load("gyre/pipeline/upscalers/models/hat_arch.py", "ref_hat_arch")
    for pkg in ("gyre", "gyre.pipeline", "gyre.pipeline.upscalers", "gyre.pipeline.upscalers.models"):
        stand_in(pkg)
    stand_in("huggingface_hub")
    stand_in("gyre.pipeline.model_loader_base", ModelLoaderBase=object)
    stand_in("basicsr.archs.rrdbnet_arch", RRDBNet=Anything)
    stand_in("gyre.pipeline.upscalers.models.esrgan_plus", RRDBNet_Plus=Anything)
    stand_in("gyre.pipeline.upscalers.models.hat_arch", HAT=hat.HAT)
    stand_in("gyre.pipeline.upscalers.models.network_swinir", SwinIR=Anything)
    loader = load("gyre/pipeline/upscalers/upscaler_loader.py", "ref_upscaler_loader")
    return hat, loader


def reference_model(hat, cfg, sd):
    m = hat.HAT(**{k: cfg[k] for k in CTOR}).eval()
    own = m.state_dict()
    m.load_state_dict({**{k: v for k, v in own.items() if weights.hat_is_buffer(k)}, **sd}, strict=True)
    return m


def image(name, shape):
    return R.model_case(name)[2] if shape == R.MODEL_CASES[name][1] else torch.rand(shape, generator=torch.Generator().manual_seed(1))


def reference_outputs(hat):
    out = {}
    for name, shape in CASES:
        cfg, sd, _ = R.model_case(name)
        with torch.no_grad():
            out[f"{name}_{'x'.join(map(str, shape))}"] = reference_model(hat, cfg, sd)(image(name, shape))
    return out


def main():
    hat, loader = reference_modules()
    out = {}
    shapes = {}
    for label, cfg in (("tiny", gcfg.tiny_hat()), ("tiny2", gcfg.tiny_hat(**R.MODEL_CASES["tiny2"][0])),
                       ("hat", gcfg.hat_config(**gcfg.HAT_DEFAULTS["hat"])), ("hat-l", gcfg.hat_config(**gcfg.HAT_DEFAULTS["hat-l"]))):
        ref = {k: list(v.shape) for k, v in hat.HAT(**{k: cfg[k] for k in CTOR}).state_dict().items()}
        mine = {k: list(v) for k, v in weights.hat_param_shapes(cfg).items()}
        shapes[label] = dict(n=len(ref), same=ref == mine, same_order=list(ref) == list(mine),
                             diff=sorted(set(ref) ^ set(mine))[:5] + [k for k in ref if k in mine and ref[k] != mine[k]][:5])
    out["shapes"] = shapes
    out["default_configs"] = {k: dict(ref=loader.DEFAULT_CONFIGS.get(k), mine=U.DEFAULT_CONFIGS.get(k), table=gcfg.HAT_DEFAULTS.get(k))
                              for k in ("hat", "hat-l")}
    model = hat.HAT(**{k: gcfg.tiny_hat()[k] for k in CTOR})
    out["indices"] = dict(sa=bool(torch.equal(model.relative_position_index_SA, R.rpi_sa())),
                          sa_closed=bool(torch.equal(model.relative_position_index_SA, R.sa_index_closed())),
                          oca=bool(torch.equal(model.relative_position_index_OCA, R.rpi_oca())),
                          oca_closed=bool(torch.equal(model.relative_position_index_OCA % 1521, R.oca_index_closed())),
                          mask=all(bool(torch.equal(model.calculate_mask(hw), R.region_mask(*hw))) for hw in ((16, 16), (16, 32), (32, 48), (48, 32))))
    fwd = {}
    for (name, shape), (key, want) in zip(CASES, reference_outputs(hat).items()):
        cfg, sd, _ = R.model_case(name)
        got = R.net(sd, cfg, image(name, shape))
        fwd[key] = dict(shape=list(want.shape), equal=bool(torch.equal(got, want)), max_abs=float((got - want).abs().max()),
                        ref_absmax=float(want.abs().max()))
    out["forward"] = fwd
    # the module shell loads the reference's own state dict strictly, buffers included
    cfg, sd, _ = R.model_case("tiny")
    full = reference_model(hat, cfg, sd).state_dict()
    shell = U.GyreHipHAT(cfg)
    res = shell.load_state_dict(full, strict=True)
    out["strict_load"] = dict(missing=list(res.missing_keys), unexpected=list(res.unexpected_keys),
                              same=all(torch.equal(v, full[k]) for k, v in shell.state_dict().items() if not weights.hat_is_buffer(k)))
    print("PROBE_JSON " + json.dumps(out))


if __name__ == "__main__":
    main()
