"""Build-container probe: the REFERENCE's upscaler host logic (gyre/pipeline/upscalers/utils.py ``tile`` and
gyre/pipeline/upscalers/upscaler_loader.py ``UpscalerLoader.convert_old_esrgan`` / ``DEFAULT_CONFIGS``, loaded from /root/reference by
file path) against gyre_amd.upscaler on the same toy data.

The two files import packages that are not installed here (torchvision and kornia through ``gyre.images``, basicsr, mmcv, the model
families); those imports are satisfied by empty stand-in modules, and ``gyre.images`` by one that carries the two functions ``tile``
calls - ``gaussianblur`` and ``scale_shape`` - routed to gyre_amd.images, so the BLUR is common to both sides and everything around
it is the reference's own code: tile-size clamp, padding, overlap search, offsets, feather geometry, blend order, crop.
``gyre/images.py`` itself is loaded as well, for ``rescale`` / ``resize`` / ``scale_shape`` / ``fromPIL``, with ResizeRight (an empty
submodule in the reference tree) routed to gyre_amd.resize.resize_right: the RESAMPLING is common, the factor choice, crop and pad
around it are the reference's.
Prints one JSON object.  Run by tests/test_reference_upscaler.py; nothing here ships."""
import importlib.util
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from gyre_amd import images as my_images, upscaler as U  # noqa: E402


def stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    return m


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Anything:
    def __init__(self, *a, **k):
        pass


stand_in("gyre")
stand_in("gyre.images", gaussianblur=my_images.gaussianblur, scale_shape=my_images.scale_shape)
for pkg in ("gyre.pipeline", "gyre.pipeline.upscalers", "gyre.pipeline.upscalers.models", "basicsr", "basicsr.archs"):
    stand_in(pkg)
stand_in("gyre.pipeline.model_loader_base", ModelLoaderBase=object)
stand_in("basicsr.archs.rrdbnet_arch", RRDBNet=Anything, ResidualDenseBlock=Anything)
stand_in("gyre.pipeline.upscalers.models.esrgan_plus", RRDBNet_Plus=Anything)
stand_in("gyre.pipeline.upscalers.models.hat_arch", HAT=Anything)
stand_in("gyre.pipeline.upscalers.models.network_swinir", SwinIR=Anything)
ref_utils = load("gyre/pipeline/upscalers/utils.py", "ref_upscaler_utils")
ref_loader = load("gyre/pipeline/upscalers/upscaler_loader.py", "ref_upscaler_loader")


class Toy(torch.nn.Module):
    """3x3 convolution then nearest upscaling, one sample at a time (so a stacked batch computes the same bits)"""

    def __init__(self, scale):
        super().__init__()
        torch.manual_seed(scale)
        self.c, self.scale = torch.nn.Conv2d(3, 3, 3, padding=1), scale

    def forward(self, x):
        return torch.stack([F.interpolate(self.c(s[None]), scale_factor=self.scale, mode="nearest")[0] for s in x])


class Quiet:
    def __init__(self, total=None, **kw):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self, *a):
        pass


# ---- gyre/images.py: rescale / resize / scale_shape / fromPIL
from gyre_amd.resize import resize_right as my_resize_right  # noqa: E402


def _ref_resize(input, scale_factors=None, out_shape=None, interp_method=None, antialiasing=True, pad_mode="constant", **kw):
    sf = tuple(scale_factors) if isinstance(scale_factors, (tuple, list)) else scale_factors
    return my_resize_right(input, out_shape=out_shape, scale_factors=sf, interp_method=interp_method, antialiasing=antialiasing, pad_mode=pad_mode)


for absent in ("cv2", "kornia", "torchvision"):
    try:
        __import__(absent)
    except Exception:
        stand_in(absent, getBuildInformation=lambda: "")
stand_in("gyre.images_shuffle", ContentShuffleDetector=Anything)
stand_in("gyre.match_histograms", match_histograms=None)
stand_in("gyre.resize_right", resize=_ref_resize, interp_methods=types.SimpleNamespace(lanczos3="lanczos3", lanczos2="lanczos2", cubic="cubic"))
ref_images = load("gyre/images.py", "gyre.images_real")

out = {"tile": {}, "rescale": {}}
g = torch.Generator().manual_seed(7)
for shape, (h, w) in (((1, 3, 20, 30), (40, 40)), ((2, 4, 33, 21), (50, 17)), ((1, 3, 40, 36), (80, 60)), ((1, 1, 16, 16), (16, 31)),
                      ((1, 3, 25, 25), (26, 26)), ((1, 3, 31, 18), (62, 37)), ((1, 3, 400, 360), (380, 300))):
    x = torch.rand(shape, generator=g)
    for fit in ("cover", "contain", "strict"):
        for sharp in (1, 2):
            a, b = ref_images.rescale(x, h, w, fit, sharpness=sharp), my_images.rescale(x, h, w, fit, sharpness=sharp)
            out["rescale"][f"{shape[2]}x{shape[3]}->{h}x{w} {fit} s{sharp}"] = dict(shape=list(a.shape), equal=a.shape == b.shape and bool(torch.equal(a, b)))
    a, b = ref_images.rescale(x, h), my_images.rescale(x, h)
    out["rescale"][f"{shape[2]}x{shape[3]}->{h} square"] = dict(shape=list(a.shape), equal=a.shape == b.shape and bool(torch.equal(a, b)))
out["resize_factor_forms"] = [bool(torch.equal(ref_images.resize(x[..., :24, :20], f), my_images.resize(x[..., :24, :20], f))) for f in (2, 0.5, (1.5,), (2, 0.75), [0.5, 2.0])]
out["scale_shape"] = [list(ref_images.scale_shape(s, f)) == list(my_images.scale_shape(s, f)) for s, f in (((1, 3, 5, 7), 2.5), ((2, 1, 100, 90), 4), ((9, 11), 0.3))]
try:
    from PIL import Image
    import numpy as np
    pics = [Image.fromarray(np.random.RandomState(0).randint(0, 256, (5, 7, c), dtype=np.uint8).squeeze(), mode) for c, mode in ((3, "RGB"), (4, "RGBA"))]
    out["from_pil"] = [bool(torch.equal(ref_images.fromPIL(p), my_images.from_pil(p))) for p in pics]
except ImportError:
    out["from_pil"] = []

with torch.no_grad():
    cases = {"default_300x270_x2": ((2, 3, 300, 270), 2, 256, {}), "default_512_x4": ((1, 3, 512, 512), 4, 256, {}),
             "one_axis_fits_200x300": ((1, 3, 200, 300), 2, 256, {}), "tile64_feather8_100x90": ((1, 3, 100, 90), 4, 64, dict(feather=8)),
             "untiled_64x48": ((1, 3, 64, 48), 4, 256, {}), "no_feather": ((1, 3, 140, 150), 2, 128, dict(feather=0))}
    for name, (shape, scale, ts, kw) in cases.items():
        x = torch.rand(shape, generator=torch.Generator().manual_seed(len(name)))
        m = Toy(scale)
        want = ref_utils.tile(x, m, scale, ts, progress_bar=Quiet, **kw)
        seq, stacked = U.tile(x, m, scale, ts, stacked=False, **kw), U.tile(x, m, scale, ts, **kw)
        out["tile"][name] = dict(shape=list(want.shape), same_shape=want.shape == seq.shape, seq_equal=bool(torch.equal(want, seq)),
                                 stacked_equal=bool(torch.equal(want, stacked)))
    refused = {}
    for name, fn in (("ref", lambda x: ref_utils.tile(x, Toy(4), 4, 64, progress_bar=Quiet)), ("mine", lambda x: U.tile(x, Toy(4), 4, 64))):
        try:
            fn(torch.rand(1, 3, 100, 90))
            refused[name] = "ran"
        except (AssertionError, ValueError) as e:
            refused[name] = "refused"
    out["tile64_default_feather"] = refused

# ---- old-format key conversion: shapes stand in as one-element tensors, the value says which tensor it is
for plus in (False, True):
    shapes = {k: (1,) for k in __import__("gyre_amd.weights", fromlist=["x"]).rrdb_param_shapes(
        __import__("gyre_amd.config", fromlist=["x"]).rrdb_config(plus=plus))}
    keys = list(shapes)
    old = {("module." if i % 3 == 0 else "") + U.old_esrgan_key(k, 23): torch.full((1,), float(i)) for i, k in enumerate(keys)}
    model = types.SimpleNamespace(state_dict=lambda: {k: torch.zeros(1) for k in keys})
    want = ref_loader.UpscalerLoader.convert_old_esrgan(dict(old), model)
    got = U.convert_old_esrgan(dict(old), shapes, 23)
    res = dict(same_keys=sorted(want) == sorted(got), same_tensors=all(torch.equal(want[k], got[k]) for k in want), n=len(got))
    errs = {}
    for label, bad in (("missing", {k: v for k, v in old.items() if "model.10." not in k}), ("leftover", dict(old, stray=torch.zeros(1)))):
        row = []
        for fn in (lambda d: ref_loader.UpscalerLoader.convert_old_esrgan(d, model), lambda d: U.convert_old_esrgan(d, shapes, 23)):
            try:
                fn(dict(bad))
                row.append("ran")
            except ValueError:
                row.append("ValueError")
        errs[label] = row
    res["errors"] = errs
    out["convert_plus" if plus else "convert"] = res

out["default_configs"] = {k: dict(ref=ref_loader.DEFAULT_CONFIGS.get(k), mine=U.DEFAULT_CONFIGS.get(k)) for k in ("esrgan", "esrgan-plus", "esrgan-6B")}
out["loader_surface"] = {n: [hasattr(ref_loader.UpscalerLoader, n), hasattr(U.GyreHipUpscalerLoader, n)]
                         for n in ("load", "esrgan", "esrgan_old", "esrgan_plus", "realesrgan", "realesrgan_6B", "swinir", "hat")}
print("PROBE_JSON " + json.dumps(out))
