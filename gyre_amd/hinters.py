"""The line-art hinter on the native path: model shell and pipeline.

The reference serves ``task: edge_detection`` engines (gyre/config/models/hinters.yaml) that turn a photo into the hint image a
ControlNet or T2I adapter conditions on.  Three of them - ``hinters-lineart-anime``, ``-contour`` and ``-opensketch`` - are the
informative-drawings generator, restated here:

  ``DrawingGenerator``             gyre/pipeline/hinters/models/informative_drawings.py   the network (all three: 3 -> 1 channels,
                                                                                         3 residual blocks)
  ``InformativeDrawingPipeline``   gyre/pipeline/hinters/informative_drawing_pipeline.py  channel normalisation, module, clamp, invert

The module's parameters carry the reference's state-dict names, so its checkpoints load strictly; all compute happens in the HIP
library (gyre_lineart_forward) - there is no PyTorch fallback.  The other hinters (HED, MiDaS / ZoeDepth, the segmenters, ...) are
not built and stay host models.
"""
from __future__ import annotations

import torch

from . import _lib
from .config import lineart_config
from .hints import normalise_tensor
from .modules import _NativeModule
from .upscaler import MODELS_PATTERN, _NativeUpscaler, _only_match, _read_state_dict
from .weights import lineart_param_shapes


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
