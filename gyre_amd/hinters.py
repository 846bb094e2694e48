"""The hinters on the native path: model shells and pipelines of the line-art generator, of the HED edge detector and of the MLSD line
detector, the Swin-B backbone of the InSPyReNet background remover, the UniFormer backbone of the segmentation annotator and the decoder
of the BAE surface-normal estimator.

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
  ``SwinB``                        gyre/pipeline/hinters/inspyrenet/backbones/             the backbone ``InSPyReNet`` takes as a module
                                   SwinTransformer.py                                     (``task: background-removal``): 12 x 12 shifted
                                                                                         windows, five feature maps; its PAA / SICA head
                                                                                         stays the host module it is
  ``UniFormer``                    gyre/pipeline/hinters/models/uniformer.py              the backbone of ``hinters-uniformer``, the default
                                                                                         ``task: segmentation`` engine behind the
                                                                                         ``controlnet/seg`` hintsets: two convolutional
                                                                                         local-relation stages, two global-attention
                                                                                         stages, four feature maps.  The mmseg UPerNet head,
                                                                                         ``MmsegPipeline`` and ``MmLoader`` stay host code
  ``Decoder`` / ``NNET``           gyre/pipeline/hinters/baenormal/                       the decoder of ``hinters-baenormal`` behind the
                                                                                         ``controlnet/normalbae`` hintsets: four
                                                                                         UpSampleBN blocks and three fused refinement
                                                                                         stages, well over 95 % of the network's arithmetic.
                                                                                         The EfficientNet-B5 encoder (``torch.hub``) stays
                                                                                         the host module the caller supplies
  ``BaenormalPipeline``            gyre/pipeline/hinters/baenormal_pipeline.py            ImageNet mean / std, module, unit length, 0 .. 1

The modules' parameters carry the reference's state-dict names, so its checkpoints load strictly; all compute happens in the HIP
library (gyre_lineart_forward, gyre_hed_forward, gyre_mlsd_forward, gyre_swinb_forward, gyre_uniformer_forward, gyre_bae_forward) -
there is no PyTorch fallback.  The other hinters (DexiNed, MiDaS / ZoeDepth, the mmpose models, ...), the InSPyReNet head, the
segmenter's UPerNet head and the normal estimator's encoder are not built and stay host models.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from .config import bae_config, bae_size_ok, hed_config, lineart_config, mlsd_config, mlsd_size_ok, swinb_config, uniformer_config
from .hints import normalise_tensor
from .modules import _NativeModule
from .upscaler import MODELS_PATTERN, _NativeUpscaler, _only_match, _read_state_dict
from .weights import (bae_is_buffer, bae_param_shapes, hed_param_shapes, lineart_param_shapes, mlsd_is_buffer, mlsd_param_shapes,
                      swinb_is_buffer, swinb_param_shapes, uniformer_is_buffer, uniformer_param_shapes)


def _load_weights(model, path, torch_dtype, allow_patterns, ignore_patterns, prefix=None, unwrap=None):
    """What every loader below does behind its constructor: ``path`` is a state-dict file or a folder that holds exactly one (after the
    allow / ignore filters); ``unwrap``: the key a checkpoint may keep its weights under; ``prefix``: only the keys under ``prefix.``
    are taken, without it.  The load is strict; the model comes back in ``torch_dtype`` (when given) and in eval mode."""
    file = path if os.path.isfile(path) else _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
    sd = _read_state_dict(file)
    if unwrap is not None:
        sd = sd.get(unwrap, sd)
    if prefix is not None:
        sd = {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}
    model.load_state_dict(sd)
    return (model if torch_dtype is None else model.to(torch_dtype)).eval()


def _bn_buffer_dtype(leaf):
    """dtype of a BatchNorm buffer: ``num_batches_tracked`` is the one integer"""
    return torch.long if leaf == "num_batches_tracked" else torch.float32


class _HintPipeline:
    """What the pipelines below share: the module, ``to``, ``pipeline_modules`` and the way a sample reaches the module."""

    def __init__(self, module):
        self.module = module

    def to(self, device):
        self.module.to(device)

    def pipeline_modules(self):
        return [("module", self.module)]

    def _sample(self, tensor: torch.Tensor, dtype=None):
        """(the tensor with a batch axis and three channels, the same on the module's device in ``dtype`` - the module's own by default)"""
        tensor = normalise_tensor(tensor, 3)     # a batch axis for [C, H, W]; 1 or 2 channels repeat channel 0, 4 or more are cut to 3
        p = next(self.module.parameters())
        return tensor, tensor.to(p.device, dtype or p.dtype)


class _NativeBackbone(_NativeUpscaler):
    """A backbone whose native call fills one flat buffer with several feature maps: the family names their shapes (``map_shapes``),
    ``forward`` returns the maps as views of the buffer."""

    def out_shape(self, shape):
        return (sum(b * c * h * w for b, c, h, w in self.map_shapes(shape)),)

    def forward(self, x: torch.Tensor):
        flat = super().forward(x)
        maps, at = [], 0
        for s in self.map_shapes(x.shape):
            n = s[0] * s[1] * s[2] * s[3]
            maps.append(flat[at:at + n].view(s))
            at += n
        return tuple(maps)


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
    return _load_weights(GyreHipDrawingGenerator(3, 1, n_residual_blocks, sigmoid), path, torch_dtype, allow_patterns, ignore_patterns)


class GyreInformativeDrawingPipeline(_HintPipeline):
    """The reference's ``InformativeDrawingPipeline``: ``pipeline(tensor) -> tensor``, a float image [B, C, H, W] or [C, H, W] in
    [0, 1] -> its line drawing [B, 1, Ho, Wo], white lines on black, on the input's device and in its dtype."""

    @torch.no_grad()
    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor, sample = self._sample(tensor)
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
    return _load_weights(GyreHipHED(), path, torch_dtype, allow_patterns, ignore_patterns)


def normalise_range(tensor: torch.Tensor) -> torch.Tensor:
    """reference images.normalise_range: every sample stretched to [0, 1] over its channels and pixels (a constant sample divides by
    zero, as there)"""
    dmin = torch.amin(tensor, dim=[1, 2, 3], keepdim=True)
    dmax = torch.amax(tensor, dim=[1, 2, 3], keepdim=True)
    return (tensor - dmin) / (dmax - dmin)


class GyreHedPipeline(_HintPipeline):
    """The reference's ``HedPipeline``: ``pipeline(tensor) -> tensor``, a float image [B, C, H, W] or [C, H, W] in [0, 1] -> its
    fused edge map [B, 1, H, W] stretched to [0, 1] per sample, on the input's device and in its dtype."""

    @torch.no_grad()
    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor, sample = self._sample(tensor)
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
    _buffer_dtype = staticmethod(_bn_buffer_dtype)

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
    return _load_weights(GyreHipMLSD(), path, torch_dtype, allow_patterns, ignore_patterns)


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


class GyreMlsdPipeline(_HintPipeline):
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
        super().__init__(module)
        self.input_size, self.top_k = int(input_size), int(top_k)
        self.score_threshold, self.distance_threshold = float(score_threshold), float(distance_threshold)

    @torch.no_grad()
    def _lines(self, tensor: torch.Tensor):
        tensor, rgb = self._sample(tensor, torch.float32)          # (the resampling runs in fp32, whatever the module's dtype)
        H, W = tensor.shape[2:]
        if (H, W) != (self.input_size, self.input_size):
            rgb = torch.nn.functional.interpolate(rgb, size=(self.input_size, self.input_size), mode="bilinear", antialias=True,
                                                  align_corners=False)
        sample = torch.cat([2 * rgb - 1, torch.full_like(rgb[:, :1], 1 / 127.5 - 1)], 1).to(next(self.module.parameters()).dtype)
        tp = self.module(sample).float()
        return tensor, mlsd_decode(tp, (H, W), self.input_size, self.score_threshold, self.distance_threshold, self.top_k)

    def lines(self, tensor: torch.Tensor):
        return self._lines(tensor)[1]

    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor, lines = self._lines(tensor)
        H, W = tensor.shape[2:]
        result = torch.stack([mlsd_rasterise(l, H, W) for l in lines])[:, None]
        return result.to(tensor.device, tensor.dtype)


# ---- Swin-B backbone of InSPyReNet ------------------------------------------------------------------------------------------------------
class GyreHipSwinB(_NativeBackbone):
    """Drop-in for the reference's ``SwinB(pretrained=False)``, the backbone module ``InSPyReNet(backbone, ...)`` takes:
    ``forward(x) -> tuple`` of five contiguous NCHW tensors, the normed patch embedding [B, C, ceil(H / 4), ceil(W / 4)] and the four
    stage outputs at C, 2 C, 4 C, 8 C channels, each stage half the size of the one before (rounded up) - 128, 128, 256, 512, 1024
    channels for Swin-B.  x NCHW [B, 3, H, W], H, W >= 4.  The parameters carry the reference's state-dict names and every attention's
    ``relative_position_index`` is a buffer as there, so the ``backbone.`` part of an InSPyReNet checkpoint loads strictly; the buffer
    is never read - the kernel computes the index.  ``depths`` / ``embed_dim`` / ``num_heads`` build smaller networks of the same
    form; anything else is refused by ``config.swinb_config``.  The native call fills one flat buffer of which the five maps are views,
    in the module's dtype: the caller casts them to the head's.  The handle, workspace and call machinery is the upscalers'."""

    _kind = "swinb"
    _param_shapes = staticmethod(swinb_param_shapes)
    _in_key, _scale_key = "in_chans", None
    _is_buffer = staticmethod(swinb_is_buffer)

    def __init__(self, **kw):
        _NativeModule.__init__(self)                 # (the reference's constructor takes keywords, not a configuration mapping)
        self._adopt(swinb_config(**kw))

    def _c_cfg(self):
        c, cfg = self.config, _lib.SwinBCfg()
        cfg.embed_dim, cfg.window_size = c.embed_dim, c.window_size
        for i, (d, h) in enumerate(zip(c.depths, c.num_heads)):
            cfg.depths[i], cfg.num_heads[i] = d, h
        cfg.ape, cfg.patch_norm, cfg.qkv_bias = int(c.ape), int(c.patch_norm), int(c.qkv_bias)
        return cfg

    def map_shapes(self, shape):
        """The five output shapes for an input of ``shape``."""
        B, _, H, W = shape
        E, h, w = self.config.embed_dim, -(-H // 4), -(-W // 4)
        shapes = [(B, E, h, w)]
        for i in range(4):
            shapes.append((B, E << i, h, w))
            h, w = -(-h // 2), -(-w // 2)
        return shapes

    def _padding(self, H, W):
        if H < 4 or W < 4:
            raise ValueError(f"the Swin-B backbone takes images of at least 4 x 4 pixels, got {H} x {W}")
        return 0, 0


def load_inspyrenet_backbone(path: str, torch_dtype=None, allow_patterns=None, ignore_patterns=None, **kw) -> GyreHipSwinB:
    """The backbone with the ``backbone.`` weights of the InSPyReNet checkpoint at ``path``: a ``*.safetensors`` / ``*.pt`` / ``*.pth``
    state dict, or a folder that holds exactly one (after the allow / ignore filters) - the layout of the reference's
    ``background-removal`` model folders.  The head's keys are left to the caller's host module; the backbone's load is strict."""
    return _load_weights(GyreHipSwinB(**kw), path, torch_dtype, allow_patterns, ignore_patterns, prefix="backbone")


# ---- UniFormer backbone of the segmentation annotator ---------------------------------------------------------------------------------
class GyreHipUniFormer(_NativeBackbone):
    """Drop-in for the reference's ``UniFormer(...)`` (windows=False, hybrid=False), the backbone of the mmseg segmentor behind
    ``hinters-uniformer``: ``forward(x) -> tuple`` of four contiguous NCHW tensors, ``norm1 .. norm4`` of the four stages at
    ``embed_dim`` channels (64, 128, 320, 512) and 1/4, 1/8, 1/16, 1/32 of the image (floor division at every step).  x NCHW
    [B, 3, H, W], H, W >= 32.  The parameters carry the reference's state-dict names in its order, the BatchNorm statistics of the
    convolutional blocks are buffers as there (``num_batches_tracked`` included), so the ``backbone.`` part of a segmentor checkpoint
    loads strictly; the native handle folds each BatchNorm into the 1x1 convolution behind it.  ``layers`` / ``embed_dim[2:]`` build
    uniformer_small, uniformer_base and smaller networks of the same form; anything else is refused by ``config.uniformer_config``.
    The native call fills one flat buffer of which the four maps are views, in the module's dtype.  The UPerNet head, ``MmsegPipeline``
    and ``MmLoader`` stay host code.  The handle, workspace and call machinery is the upscalers'."""

    _kind = "uniformer"
    _param_shapes = staticmethod(uniformer_param_shapes)
    _in_key, _scale_key = "in_chans", None
    _is_buffer = staticmethod(uniformer_is_buffer)
    _buffer_dtype = staticmethod(_bn_buffer_dtype)

    def __init__(self, **kw):
        _NativeModule.__init__(self)                 # (the reference's constructor takes keywords, not a configuration mapping)
        self._adopt(uniformer_config(**kw))

    def _c_cfg(self):
        c, cfg = self.config, _lib.UniFormerCfg()
        for i, (d, e) in enumerate(zip(c.layers, c.embed_dim)):
            cfg.layers[i], cfg.embed_dim[i] = d, e
        cfg.head_dim, cfg.mlp_ratio, cfg.qkv_bias = c.head_dim, int(c.mlp_ratio), int(c.qkv_bias)
        cfg.windows, cfg.hybrid = int(c.windows), int(c.hybrid)
        return cfg

    def map_shapes(self, shape):
        """The four output shapes for an input of ``shape``."""
        B, _, H, W = shape
        h, w, shapes = H // 4, W // 4, []
        for e in self.config.embed_dim:
            shapes.append((B, e, h, w))
            h, w = h // 2, w // 2
        return shapes

    def _padding(self, H, W):
        if H < 32 or W < 32:
            raise ValueError(f"the UniFormer backbone takes images of at least 32 x 32 pixels, got {H} x {W}")
        return 0, 0


def load_uniformer_backbone(path: str, torch_dtype=None, allow_patterns=None, ignore_patterns=None, **kw) -> GyreHipUniFormer:
    """The backbone with the ``backbone.`` weights of the mmseg segmentor checkpoint at ``path``: a ``*.safetensors`` / ``*.pt`` /
    ``*.pth`` file (an mmcv checkpoint keeps its weights under ``state_dict``), or a folder that holds exactly one (after the allow /
    ignore filters) - the layout of the reference's ``hinters-uniformer`` model folder.  The decode and auxiliary heads' keys are left to
    the caller's host module; the backbone's load is strict."""
    return _load_weights(GyreHipUniFormer(**kw), path, torch_dtype, allow_patterns, ignore_patterns, prefix="backbone", unwrap="state_dict")


# ---- BAE surface-normal estimator -------------------------------------------------------------------------------------------------------
IMAGENET_STD = [0.229, 0.224, 0.225]


class GyreHipBaeDecoder(_NativeUpscaler):
    """Drop-in for the reference's ``Decoder(args)`` with ``args.architecture == "BN"``: ``forward(features, gt_norm_mask=None,
    mode='test')`` takes the encoder's feature list, reads its entries 4, 5, 6, 8 and 11 (x_block0 .. x_block4) as the reference does
    and returns the reference's triple ``([out_res8, out_res4, out_res2, out_res1], [out_res8, None, None, None], [None] * 4)``: four
    contiguous [B, 4, h, w] tensors - unit normal and kappa - at 1/4 of x_block0's size doubling up to twice it, views of one flat
    buffer in the module's dtype.  The sides of x_block0 must be multiples of 4, the sizes at which the reference's own concatenations
    line up (a ValueError otherwise); ``mode='train'`` (uncertainty-guided point sampling) and architecture "GN" are refused with
    NotImplementedError.  The parameters carry the reference's state-dict names in its order and the BatchNorm statistics are buffers
    as there (``num_batches_tracked`` included), so the ``decoder.`` part of an NNET checkpoint loads strictly; the native handle folds
    every BatchNorm into its convolution.  The handle, workspace and call machinery is the upscalers'."""

    _kind = "bae"
    _param_shapes = staticmethod(bae_param_shapes)
    _in_key, _scale_key = "num_features", None
    _is_buffer = staticmethod(bae_is_buffer)
    _buffer_dtype = staticmethod(_bn_buffer_dtype)
    BLOCKS = (4, 5, 6, 8, 11)                        # the encoder's feature-list entries the decoder reads

    def __init__(self, architecture: str = "BN", **kw):
        _NativeModule.__init__(self)                 # (the reference's constructor takes an args namespace, not a configuration mapping)
        self._adopt(bae_config(architecture=getattr(architecture, "architecture", architecture), **kw))

    def _c_cfg(self):
        c, cfg = self.config, _lib.BaeCfg()
        cfg.num_features, cfg.architecture = c.num_features, 0
        for i, s in enumerate(c.skip_features):
            cfg.skip[i] = s
        return cfg

    def block_shapes(self, B, H, W):
        """The five input shapes for an x_block0 of H x W (the encoder's ceil halving)."""
        shapes = []
        for c in (*self.config.skip_features, self.config.num_features):
            shapes.append((B, c, H, W))
            H, W = -(-H // 2), -(-W // 2)
        return shapes

    def _padding(self, H, W):
        if not (bae_size_ok(H) and bae_size_ok(W)):
            raise ValueError(f"the BAE decoder takes an x_block0 whose sides are multiples of 4 (an image whose sides are multiples of 8), "
                             f"got {H} x {W}")
        return 0, 0

    @torch.no_grad()
    def forward(self, features, gt_norm_mask=None, mode="test"):
        if mode != "test":
            raise NotImplementedError(f"Decoder: mode {mode!r} is outside the native path (mode='test' is built; the training-mode point "
                                      f"sampling is not)")
        blocks = [features[i] for i in self.BLOCKS]
        B, _, H, W = blocks[0].shape
        self._padding(H, W)
        want = self.block_shapes(B, H, W)
        if [tuple(b.shape) for b in blocks] != want:
            raise ValueError(f"expected feature maps of shapes {want}, got {[tuple(b.shape) for b in blocks]}")
        dev = blocks[0].device
        h = self._sync(dev)
        dt = blocks[0].dtype if blocks[0].dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32
        flat = torch.cat([b.to(dt).reshape(-1) for b in blocks])
        _lib.require_gpu_tensor(flat, "features")
        L = self._L()
        h4, w4 = H // 4, W // 4
        shapes = [(B, 4, h4 << s, w4 << s) for s in range(4)]
        with torch.cuda.device(dev):
            need = self._native("workspace_bytes")(C.c_void_p(h), B, H, W)
            if need == 0:
                _lib.check(-1, L)
            ws = self._workspace(need, dev)
            wp = (ws.data_ptr() + 255) & ~255
            out = torch.empty(sum(b * c * y * x for b, c, y, x in shapes), dtype=self.dtype, device=dev)
            _lib.check(self._native("forward")(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(flat.data_ptr()),
                                               _lib.dtype_code(flat), B, H, W, C.c_void_p(wp), need, C.c_void_p(out.data_ptr()),
                                               _lib.dtype_code(out)), L)
        maps, at = [], 0
        for s in shapes:
            n = s[0] * s[1] * s[2] * s[3]
            maps.append(out[at:at + n].view(s))
            at += n
        return maps, [maps[0], None, None, None], [None] * 4


class GyreHipNNET(torch.nn.Module):
    """The reference's ``NNET``: the caller's host ``encoder`` module (``tf_efficientnet_b5_ap`` behind the reference's ``Encoder``,
    about 3 % of the network's arithmetic; its program text comes through ``torch.hub`` and is not restated here) and the native
    decoder, under the reference's submodule names ``encoder`` / ``decoder``: ``forward(img, **kwargs)`` ->
    ``decoder(encoder(img), **kwargs)``."""

    def __init__(self, encoder: torch.nn.Module, **kw):
        super().__init__()
        self.encoder = encoder
        self.decoder = GyreHipBaeDecoder(**kw)

    def forward(self, img, **kwargs):
        return self.decoder(self.encoder(img), **kwargs)


def load_baenormal(path: str, encoder: torch.nn.Module, torch_dtype=None, allow_patterns=None, ignore_patterns=None, **kw) -> GyreHipNNET:
    """``NNET`` with the weights of ``path``: a ``*.safetensors`` / ``*.pt`` / ``*.pth`` checkpoint, or a folder that holds exactly one
    (after the allow / ignore filters) - the layout of the reference's ``hinters-baenormal`` model folder.  As the reference's loader:
    a checkpoint may keep its weights under ``model`` and its keys may carry a ``module.`` prefix.  The ``decoder.`` entries load
    strictly into the native decoder, the ``encoder.`` entries (strictly) into the given encoder."""
    file = path if os.path.isfile(path) else _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
    sd = _read_state_dict(file)
    sd = sd.get("model", sd)
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    model = GyreHipNNET(encoder, **kw)
    for name, part in (("decoder", model.decoder), ("encoder", model.encoder)):
        part.load_state_dict({k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")})
    return (model if torch_dtype is None else model.to(torch_dtype)).eval()


class GyreBaenormalPipeline(_HintPipeline):
    """The reference's ``BaenormalPipeline``: ``pipeline(tensor) -> tensor``, a float image [B, C, H, W] or [C, H, W] in [0, 1] -> its
    normal map [B, 3, H, W] in [0, 1], on the input's device and in its dtype: ImageNet mean / std, the module (``GyreHipNNET``), the
    first three channels of the last map, unit length, ``* 0.5 + 0.5``, clip.  (The reference's debug print is dropped.)"""

    @torch.no_grad()
    def __call__(self, tensor: torch.Tensor) -> torch.Tensor:
        tensor, sample = self._sample(tensor)
        mean = torch.tensor(IMAGENET_MEAN).to(sample).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD).to(sample).view(1, 3, 1, 1)
        norm_out_list, _, _ = self.module((sample - mean) / std)
        norm_out = norm_out_list[-1][:, :3]
        norm_out = norm_out / (norm_out ** 2.0).sum(dim=1, keepdim=True) ** 0.5
        result = (norm_out * 0.5 + 0.5).clip(0, 1)
        return result.to(tensor.device, tensor.dtype)
