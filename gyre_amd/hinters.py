"""The hinters on the native path: model shells and pipelines of the line-art generator and of the HED edge detector.

The reference serves ``task: edge_detection`` engines (gyre/config/models/hinters.yaml) that turn a photo into the hint image a
ControlNet or T2I adapter conditions on.  Three of them - ``hinters-lineart-anime``, ``-contour`` and ``-opensketch`` - are the
informative-drawings generator, and ``hinters-hed`` / ``hinters-hed-alt`` the holistically-nested edge detector that feeds the
scribble and soft-edge ControlNets; both are restated here:

  ``DrawingGenerator``             gyre/pipeline/hinters/models/informative_drawings.py   the network (all three: 3 -> 1 channels,
                                                                                         3 residual blocks)
  ``InformativeDrawingPipeline``   gyre/pipeline/hinters/informative_drawing_pipeline.py  channel normalisation, module, clamp, invert
  ``HED``                          gyre/pipeline/hinters/models/hed.py                    the network: a VGG-16 trunk, five side
                                                                                         outputs and their fuse, six sigmoided maps
  ``HedPipeline``                  gyre/pipeline/hinters/hed_pipeline.py                  channel normalisation, ImageNet mean, BGR x 255,
                                                                                         module, the fused map, range normalisation

The modules' parameters carry the reference's state-dict names, so its checkpoints load strictly; all compute happens in the HIP
library (gyre_lineart_forward, gyre_hed_forward) - there is no PyTorch fallback.  The other hinters (DexiNed, MiDaS / ZoeDepth, the
segmenters, ...) are not built and stay host models.
"""
from __future__ import annotations

import torch

from . import _lib
from .config import hed_config, lineart_config
from .hints import normalise_tensor
from .modules import _NativeModule
from .upscaler import MODELS_PATTERN, _NativeUpscaler, _only_match, _read_state_dict
from .weights import hed_param_shapes, lineart_param_shapes


class GyreHipDrawingGenerator(_NativeUpscaler):
    """Drop-in for the reference's ``DrawingGenerator(input_nc, output_nc, n_residual_blocks=9, sigmoid=True)``:
    ``forward(x, cond=None) -> tensor``, NCHW in and out, the output [B, 1, Ho, Wo] with Ho = 4 ceil(ceil(H / 2) / 2) - the size the
    reference's layers produce, H itself when H % 4 == 0.  Built: input_nc 3, output_nc 1, 1 to 16 residual blocks; H, W >= 5.
    The handle, workspace and call machinery is the upscalers' (``_NativeUpscaler``)."""

    _kind = "lineart"
    _param_shapes = staticmethod(lineart_param_shapes)
    _in_key, _scale_key = "input_nc", None

    def __init__(self, input_nc: int, output_nc: int, n_residual_blocks: int = 9, sigmoid: bool = True, **kw):
        _NativeModule.__init__(self)                 # (the reference's positional signature, not the upscalers' config mapping)
        self._adopt(lineart_config(input_nc, output_nc, n_residual_blocks, sigmoid, **kw))

    def _c_cfg(self):
        c, cfg = self.config, _lib.LineartCfg()
        cfg.input_nc, cfg.output_nc, cfg.n_residual_blocks, cfg.sigmoid = c.input_nc, c.output_nc, c.n_residual_blocks, int(c.sigmoid)
        return cfg

    def out_shape(self, shape):
        B, _, H, W = shape
        return (B, self.config.output_nc, -(-(-(-H // 2)) // 2) * 4, -(-(-(-W // 2)) // 2) * 4)

    def _padding(self, H, W):
        if H < 5 or W < 5:
            raise ValueError(f"the line-art generator takes images of at least 5 x 5 pixels, got {H} x {W}")
        return 0, 0

    def forward(self, x: torch.Tensor, cond=None) -> torch.Tensor:
        return super().forward(x)


def load_drawing_generator(path: str, torch_dtype=None, allow_patterns=None, ignore_patterns=None, n_residual_blocks: int = 3,
                           sigmoid: bool = True) -> GyreHipDrawingGenerator:
    """The generator with the weights of ``path``: a ``*.safetensors`` / ``*.pt`` / ``*.pth`` state dict, or a folder that holds
    exactly one (after the allow / ignore filters) - the layout of the reference's ``hinters-lineart-*`` model folders.  The load
    is strict."""
    import os
    model = GyreHipDrawingGenerator(3, 1, n_residual_blocks, sigmoid)
    file = path if os.path.isfile(path) else _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
    model.load_state_dict(_read_state_dict(file))
    return (model if torch_dtype is None else model.to(torch_dtype)).eval()


class GyreInformativeDrawingPipeline:
    """The reference's ``InformativeDrawingPipeline``: ``pipeline(tensor) -> tensor``, a float image [B, C, H, W] or [C, H, W] in
    [0, 1] -> its line drawing [B, 1, Ho, Wo], white lines on black, on the input's device and in its dtype."""

    def __init__(self, module):
        self.module = module

    def to(self, device):
        self.module.to(device)

    def pipeline_modules(self):
        return [("module", self.module)]

    @torch.no_grad()
    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor = normalise_tensor(tensor, 3)     # a batch axis for [C, H, W]; 1 or 2 channels repeat channel 0, 4 or more are cut to 3
        p = next(self.module.parameters())
        sample = tensor.to(p.device, p.dtype)
        result = self.module(sample).clamp(0, 1)
        result = 1 - result                     # white on a black background, what the ControlNets were trained on
        return result.to(tensor.device, tensor.dtype)


# ---- HED -------------------------------------------------------------------------------------------------------------------------------
IMAGENET_MEAN = [0.485, 0.456, 0.406]


class GyreHipHED(_NativeUpscaler):
    """Drop-in for the reference's ``HED()``: ``forward(x) -> [so1, so2, so3, so4, so5, fuse]``, six contiguous [B, 1, H, W] tensors,
    each already sigmoided; x NCHW [B, 3, H, W] - what ``HedPipeline`` feeds is BGR in 0 .. 255 less the mean.  Any H, W >= 1.  The
    handle, workspace and call machinery is the upscalers' (``_NativeUpscaler``); the native call fills one [6 B, 1, H, W] buffer,
    map-major, of which the six results are views."""

    _kind = "hed"
    _param_shapes = staticmethod(hed_param_shapes)
    _in_key, _scale_key = "input_nc", None

    def __init__(self, **kw):
        _NativeModule.__init__(self)                 # (the reference's constructor has no arguments)
        self._adopt(hed_config(**kw))

    def _c_cfg(self):
        return _lib.HedCfg(reserved=0)

    def out_shape(self, shape):
        B, _, H, W = shape
        return (6 * B, 1, H, W)

    def _padding(self, H, W):
        if H < 1 or W < 1:
            raise ValueError(f"HED takes images of at least 1 x 1 pixels, got {H} x {W}")
        return 0, 0

    def forward(self, x: torch.Tensor):
        out = super().forward(x)
        return list(out.split(x.shape[0], dim=0))


def load_hed(path: str, torch_dtype=None, allow_patterns=None, ignore_patterns=None) -> GyreHipHED:
    """The detector with the weights of ``path``: a ``*.safetensors`` / ``*.pt`` / ``*.pth`` state dict, or a folder that holds
    exactly one (after the allow / ignore filters) - the layout of the reference's ``hinters-hed`` model folders.  The load is
    strict."""
    import os
    model = GyreHipHED()
    file = path if os.path.isfile(path) else _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
    model.load_state_dict(_read_state_dict(file))
    return (model if torch_dtype is None else model.to(torch_dtype)).eval()


def normalise_range(tensor: torch.Tensor) -> torch.Tensor:
    """reference images.normalise_range: every sample stretched to [0, 1] over its channels and pixels (a constant sample divides by
    zero, as there)"""
    dmin = torch.amin(tensor, dim=[1, 2, 3], keepdim=True)
    dmax = torch.amax(tensor, dim=[1, 2, 3], keepdim=True)
    return (tensor - dmin) / (dmax - dmin)


class GyreHedPipeline:
    """The reference's ``HedPipeline``: ``pipeline(tensor) -> tensor``, a float image [B, C, H, W] or [C, H, W] in [0, 1] -> its
    fused edge map [B, 1, H, W] stretched to [0, 1] per sample, on the input's device and in its dtype."""

    def __init__(self, module):
        self.module = module

    def to(self, device):
        self.module.to(device)

    def pipeline_modules(self):
        return [("module", self.module)]

    @torch.no_grad()
    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor = normalise_tensor(tensor, 3)
        p = next(self.module.parameters())
        sample = tensor.to(p.device, p.dtype)
        mean = torch.tensor(IMAGENET_MEAN).to(sample).view(1, 3, 1, 1)
        sample = (sample - mean)[:, [2, 1, 0]] * 255         # the RGB mean comes off first, then BGR at 0 .. 255
        result = normalise_range(self.module(sample)[-1])
        return result.to(tensor.device, tensor.dtype)
