"""The hinters on the native path: model shells and pipelines of the line-art generator, of the HED edge detector and of the MLSD line
detector.

The reference serves ``task: edge_detection`` engines (gyre/config/models/hinters.yaml) that turn a photo into the hint image a
ControlNet or T2I adapter conditions on.  Three of them - ``hinters-lineart-anime``, ``-contour`` and ``-opensketch`` - are the
informative-drawings generator, and ``hinters-hed`` / ``hinters-hed-alt`` the holistically-nested edge detector that feeds the
scribble and soft-edge ControlNets; both are restated here, and so is the MLSD network the reference vendors for the straight-line hint
of its ``controlnet/mlsd`` hintsets:

  ``DrawingGenerator``             gyre/pipeline/hinters/models/informative_drawings.py   the network (all three: 3 -> 1 channels,
                                                                                         3 residual blocks)
  ``InformativeDrawingPipeline``   gyre/pipeline/hinters/informative_drawing_pipeline.py  channel normalisation, module, clamp, invert
  ``HED``                          gyre/pipeline/hinters/models/hed.py                    the network: a VGG-16 trunk, five side
                                                                                         outputs and their fuse, six sigmoided maps
  ``HedPipeline``                  gyre/pipeline/hinters/hed_pipeline.py                  channel normalisation, ImageNet mean, BGR x 255,
                                                                                         module, the fused map, range normalisation
  ``MobileV2_MLSD_Large``          gyre/pipeline/hinters/models/mbv2_mlsd_large.py        the network: a MobileNetV2 trunk and a four-level
                                                                                         decoder, 4 -> 9 channels at half the size
  ``GyreMlsdPipeline``             (an extension: the reference wires no pipeline for it)  the upstream M-LSD decode, restated: resample,
                                                                                         module, centre map, top-k, segments, raster

The modules' parameters carry the reference's state-dict names, so its checkpoints load strictly; all compute happens in the HIP
library (gyre_lineart_forward, gyre_hed_forward, gyre_mlsd_forward) - there is no PyTorch fallback.  The other hinters (DexiNed, MiDaS / ZoeDepth, the
segmenters, ...) are not built and stay host models.
"""
from __future__ import annotations

import torch

from . import _lib
from .config import hed_config, lineart_config, mlsd_config, mlsd_size_ok
from .hints import normalise_tensor
from .modules import _NativeModule
from .upscaler import MODELS_PATTERN, _NativeUpscaler, _only_match, _read_state_dict
from .weights import hed_param_shapes, lineart_param_shapes, mlsd_is_buffer, mlsd_param_shapes


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


# ---- MLSD ------------------------------------------------------------------------------------------------------------------------------
class GyreHipMLSD(_NativeUpscaler):
    """Drop-in for the reference's ``MobileV2_MLSD_Large()``: ``forward(x) -> [B, 9, H // 2, W // 2]``, channels 7 .. 15 of the
    network's 16-channel map; x NCHW [B, 4, H, W].  H and W: at least 16 with (H // 2) % 8 == 0, the sizes at which the reference's own
    concatenations line up (a ValueError otherwise).  The BatchNorm statistics are buffers as in the reference, ``num_batches_tracked``
    included: its 362 keys load strictly; the native handle folds every BatchNorm into its convolution.  The handle, workspace and call
    machinery is the upscalers' (``_NativeUpscaler``)."""

    _kind = "mlsd"
    _param_shapes = staticmethod(mlsd_param_shapes)
    _in_key, _scale_key = "input_nc", None
    _is_buffer = staticmethod(mlsd_is_buffer)
    _buffer_dtype = staticmethod(lambda leaf: torch.long if leaf == "num_batches_tracked" else torch.float32)

    def __init__(self, **kw):
        _NativeModule.__init__(self)                 # (the reference's constructor has no arguments)
        self._adopt(mlsd_config(**kw))

    def _c_cfg(self):
        return _lib.MlsdCfg(reserved=0)

    def out_shape(self, shape):
        B, _, H, W = shape
        return (B, 9, H // 2, W // 2)

    def _padding(self, H, W):
        if not (mlsd_size_ok(H) and mlsd_size_ok(W)):
            raise ValueError(f"MLSD takes images of at least 16 x 16 pixels with (H // 2) % 8 == 0 and (W // 2) % 8 == 0, got {H} x {W}")
        return 0, 0


def load_mlsd(path: str, torch_dtype=None, allow_patterns=None, ignore_patterns=None) -> GyreHipMLSD:
    """The detector with the weights of ``path``: a ``*.safetensors`` / ``*.pt`` / ``*.pth`` state dict, or a folder that holds
    exactly one (after the allow / ignore filters).  The load is strict."""
    import os
    model = GyreHipMLSD()
    file = path if os.path.isfile(path) else _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
    model.load_state_dict(_read_state_dict(file))
    return (model if torch_dtype is None else model.to(torch_dtype)).eval()


def mlsd_decode(tp: torch.Tensor, size, input_size: int, score_threshold: float = 0.1, distance_threshold: float = 0.1, top_k: int = 200):
    """The upstream M-LSD decode of the network's map tp [B, 9, h, w] (fp32) into segments of an image of ``size`` = (H, W): a list of
    [n_i, 5] fp32 tensors (x0, y0, x1, y1, score) in image pixels.  Channel 0 is the centre logit, channels 1 .. 4 the offsets of the
    two end points (start x, start y, end x, end y) in map pixels.  A centre is a location whose sigmoided logit equals the maximum of
    its 3 x 3 neighbourhood; per sample the ``top_k`` highest centres are taken in a stable descending order (equal scores in index
    order), and those above both thresholds are kept."""
    H, W = size
    heat = torch.sigmoid(tp[:, 0])
    keep = heat == torch.nn.functional.max_pool2d(heat[:, None], 3, 1, 1)[:, 0]
    score = heat * keep
    d = tp[:, 1:5]
    length = torch.hypot(d[:, 0] - d[:, 2], d[:, 1] - d[:, 3])
    wm = tp.shape[3]
    scale = torch.tensor([W / input_size, H / input_size, W / input_size, H / input_size], dtype=torch.float32, device=tp.device)
    out = []
    for b in range(tp.shape[0]):
        order = torch.sort(score[b].flatten(), descending=True, stable=True)       # (torch.topk does not promise the order of ties)
        idx, sc = order.indices[:top_k], order.values[:top_k]
        sel = (sc > score_threshold) & (length[b].flatten()[idx] > distance_threshold)
        idx, sc = idx[sel], sc[sel]
        centre = torch.stack([idx % wm, idx // wm, idx % wm, idx // wm], 1).to(torch.float32)
        seg = (centre + d[b].flatten(1)[:, idx].t()) * 2 * scale
        out.append(torch.cat([seg, sc[:, None]], 1))
    return out


def mlsd_rasterise(lines: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[n, >= 4] segments (x0, y0, x1, y1, ...) -> [H, W] fp32, 1 on every segment and 0 elsewhere.  A segment is sampled at
    n = max(|round(x1) - round(x0)|, |round(y1) - round(y0)|) + 1 points x0 + (x1 - x0) i / (n - 1), each rounded half to even; the
    points outside the image are dropped."""
    img = torch.zeros((H, W), dtype=torch.float32, device=lines.device)
    if lines.shape[0] == 0:
        return img
    x0, y0, x1, y1 = (lines[:, k].to(torch.float32) for k in range(4))
    n = torch.maximum((torch.round(x1) - torch.round(x0)).abs(), (torch.round(y1) - torch.round(y0)).abs()).to(torch.long) + 1
    i = torch.arange(int(n.max()), device=lines.device)[None, :]
    t = i.to(torch.float32) / (n[:, None] - 1).clamp_min(1).to(torch.float32)
    px = torch.round(x0[:, None] + (x1 - x0)[:, None] * t).to(torch.long)
    py = torch.round(y0[:, None] + (y1 - y0)[:, None] * t).to(torch.long)
    ok = (i < n[:, None]) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    img[py[ok], px[ok]] = 1.0
    return img


class GyreMlsdPipeline:
    """``pipeline(tensor) -> tensor``: a float image [B, C, H, W] or [C, H, W] in [0, 1] -> its straight-line drawing [B, 1, H, W],
    white lines on black, on the input's device and in its dtype; ``pipeline.lines(tensor)`` -> the segments themselves, a list of
    [n_i, 5] fp32 tensors (x0, y0, x1, y1, score) in image pixels.

    An extension: the reference vendors the network but wires no pipeline for it, so this restates the upstream M-LSD decode
    (github.com/navervision/mlsd, ``pred_lines``): the image resampled to ``input_size`` square, RGB in [-1, 1] and a constant fourth
    plane of 1 / 127.5 - 1, the module, ``mlsd_decode`` and ``mlsd_rasterise``.  Everything behind the module is thin PyTorch on the
    module's device: it runs once per image on a map of half the input size."""

    def __init__(self, module, input_size: int = 512, score_threshold: float = 0.1, distance_threshold: float = 0.1, top_k: int = 200):
        if not mlsd_size_ok(int(input_size)):
            raise ValueError(f"input_size must be at least 16 with (input_size // 2) % 8 == 0, got {input_size}")
        if top_k < 1:
            raise ValueError(f"top_k must be at least 1, got {top_k}")
        self.module, self.input_size, self.top_k = module, int(input_size), int(top_k)
        self.score_threshold, self.distance_threshold = float(score_threshold), float(distance_threshold)

    def to(self, device):
        self.module.to(device)

    def pipeline_modules(self):
        return [("module", self.module)]

    @torch.no_grad()
    def _lines(self, tensor: torch.Tensor):
        tensor = normalise_tensor(tensor, 3)
        p = next(self.module.parameters())
        H, W = tensor.shape[2:]
        rgb = tensor.to(p.device, torch.float32)
        if (H, W) != (self.input_size, self.input_size):
            rgb = torch.nn.functional.interpolate(rgb, size=(self.input_size, self.input_size), mode="bilinear", antialias=True,
                                                  align_corners=False)
        sample = torch.cat([2 * rgb - 1, torch.full_like(rgb[:, :1], 1 / 127.5 - 1)], 1).to(p.dtype)
        tp = self.module(sample).float()
        return tensor, mlsd_decode(tp, (H, W), self.input_size, self.score_threshold, self.distance_threshold, self.top_k)

    def lines(self, tensor: torch.Tensor):
        return self._lines(tensor)[1]

    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor, lines = self._lines(tensor)
        H, W = tensor.shape[2:]
        result = torch.stack([mlsd_rasterise(l, H, W) for l in lines])[:, None]
        return result.to(tensor.device, tensor.dtype)
