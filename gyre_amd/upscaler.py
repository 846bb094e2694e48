"""The ESRGAN, SwinIR and HAT families of upscaler engines on the native path: model shells, loader and pipeline.

The reference serves ``task: upscaler`` engines (gyre/config/engines/upscaler.yaml) through three pieces whose behaviour is
restated here:

  ``UpscalerLoader``     gyre/pipeline/upscalers/upscaler_loader.py   folder -> model: default configurations, ``params_ema``,
                                                                      old-format ESRGAN checkpoints
  ``UpscalerPipeline``   gyre/pipeline/upscalers/upscaler_pipeline.py alpha split, tiled module calls, clamp, alpha, rescale
  ``tile``               gyre/pipeline/upscalers/utils.py             reflect pad, overlap search, feathered sequential blend

The model is BasicSR's ``RRDBNet`` (``esrgan``, ``esrgan_old``, ``realesrgan``, ``realesrgan_6B``) or the reference's ``RRDBNet_Plus``
(``esrgan_plus``); its parameters carry BasicSR's state-dict names and all compute happens in the HIP library (gyre_rrdb_forward) -
there is no PyTorch fallback.  The second family is the reference's vendored ``SwinIR`` (``swinir``, ``swinir_l``;
gyre/pipeline/upscalers/models/network_swinir.py) in its "nearest+conv" form, on gyre_swinir_forward; SwinIR's pixel-shuffle and
denoising forms are not built.  The third is the reference's vendored ``HAT`` (``hat``, ``hat_l``; .../models/hat_arch.py) in its
"pixelshuffle" / "1conv" form at window 16, on gyre_hat_forward.

One native liberty: the tiles of a request go through the module as stacked batches (up to 16 tiles each, so the 9 tiles of a
512 x 512 request are ONE call) and are then blended in the reference's order.  The module is batch-independent (a sample's result does not depend on the batch it runs in), so the result is the same; a
single 256 x 256 tile alone would leave half of the GPU idle.
"""
from __future__ import annotations

import ctypes as C
import fnmatch
import glob
import os
import re
from typing import Optional

import numpy as np
import torch

from . import _lib, images
from .config import HAT_DEFAULTS, RRDB_DEFAULTS, SWINIR_DEFAULTS, hat_config, rrdb_config, swinir_config
from .modules import _NativeModule, _build_tree
from .weights import hat_is_buffer, hat_param_shapes, rrdb_param_shapes, swinir_is_buffer, swinir_param_shapes

PATHS = {"auto": 0, "generic": 1, "fused": 2}
_UNSHUFFLE = {4: 1, 2: 2, 1: 4}          # model scale -> pixel-unshuffle factor in front of conv_first


class _NativeUpscaler(_NativeModule):
    """What the three upscaler shells share: the configuration merge, the parameter tree with the family's buffers, the workspace
    query and the native call (gyre_{kind}_workspace_bytes / gyre_{kind}_forward).  A family names its configuration
    (``_make_config``, ``_param_shapes``, the keys of its channel count and scale - ``_scale_key = None``: the output has the input's scale), its buffers (``_is_buffer``, ``_buffer_dtype``) and
    its size rule (``_padding``), and builds its C configuration (``_c_cfg``)."""

    _make_config = _param_shapes = None
    _in_key, _scale_key = "in_chans", "upscale"
    _is_buffer = staticmethod(lambda key: False)
    _buffer_dtype = staticmethod(lambda leaf: torch.long)

    def __init__(self, config: Optional[dict] = None, **kw):
        super().__init__()
        cfg = dict(config or {})
        cfg.update(kw)
        self._adopt(type(self)._make_config(**cfg))

    def _adopt(self, config) -> None:
        """The checked configuration -> what a pipeline reads from the module (``_scale``: 1 for a family that names no scale key;
        ``_window_size``) and the parameter tree with the family's buffers.  A family whose constructor has its own signature calls
        this after ``_NativeModule.__init__``."""
        self.config = config
        self._scale = config[self._scale_key] if self._scale_key else 1
        self._window_size = config.get("window_size", 32)
        shapes = self._shapes()
        _build_tree(self, {k: v for k, v in shapes.items() if not self._is_buffer(k)})
        for key, shape in shapes.items():
            if self._is_buffer(key):
                node = self
                *path, leaf = key.split(".")
                for part in path:
                    node = node._modules[part]
                node.register_buffer(leaf, torch.zeros(shape, dtype=self._buffer_dtype(leaf)))

    def _shapes(self):
        return type(self)._param_shapes(self.config)

    def _prepare(self, h) -> None:
        """Per-handle switches to apply before a native call."""

    def _padding(self, H: int, W: int):
        """The family's size rule: (rows, columns) to reflect-pad on the bottom / right before the call, cropped from the result;
        a size it does not take is a ValueError."""
        raise NotImplementedError

    def _native(self, name: str):
        return getattr(self._L(), f"gyre_{self._kind}_{name}")

    def workspace_bytes(self, B: int, H: int, W: int, device) -> int:
        h = self._sync(torch.device(device))
        self._prepare(h)
        with torch.cuda.device(device):
            return int(self._native("workspace_bytes")(C.c_void_p(h), B, H, W))

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        cin = self.config[self._in_key]
        if x.ndim != 4 or x.shape[1] != cin:
            raise ValueError(f"expected an image [B,{cin},H,W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        ph, pw = self._padding(H, W)
        dev = x.device
        h = self._sync(dev)
        self._prepare(h)
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            x = x.to(torch.float32)
        if ph or pw:                                                     # check_image_size: reflect on the bottom / right
            x = torch.nn.functional.pad(x, (0, pw, 0, ph), "reflect")
        x = x.contiguous()
        _lib.require_gpu_tensor(x, "image")
        L = self._L()
        Hp, Wp = H + ph, W + pw
        with torch.cuda.device(dev):
            need = self._native("workspace_bytes")(C.c_void_p(h), B, Hp, Wp)
            if need == 0:
                _lib.check(-1, L)
            ws = self._workspace(need, dev)
            wp = (ws.data_ptr() + 255) & ~255
            out = torch.empty(self.out_shape(x.shape), dtype=self.dtype, device=dev)
            _lib.check(self._native("forward")(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()),
                                               _lib.dtype_code(x), B, Hp, Wp, C.c_void_p(wp), need, C.c_void_p(out.data_ptr()),
                                               _lib.dtype_code(out)), L)
        return out[:, :, :H * self._scale, :W * self._scale] if ph or pw else out


class GyreHipRRDBNet(_NativeUpscaler):
    """Drop-in for BasicSR's RRDBNet / the reference's RRDBNet_Plus (``plus=True``): ``forward(x) -> tensor``, NCHW in and out."""

    _kind = "rrdb"
    _make_config, _param_shapes = staticmethod(rrdb_config), staticmethod(rrdb_param_shapes)
    _in_key, _scale_key = "num_in_ch", "scale"
    _path = 0

    def __init__(self, config: Optional[dict] = None, plus: bool = False, **kw):
        cfg = dict(config or {})
        cfg.update(kw)
        cfg["plus"] = bool(cfg.pop("plus", plus))
        super().__init__(cfg)

    def _c_cfg(self):
        c, cfg = self.config, _lib.RRDBCfg()
        cfg.num_in_ch, cfg.num_out_ch, cfg.num_feat, cfg.num_block = c.num_in_ch, c.num_out_ch, c.num_feat, c.num_block
        cfg.num_grow_ch, cfg.scale, cfg.plus = c.num_grow_ch, c.scale, int(bool(c.plus))
        return cfg

    def set_path(self, path) -> None:
        """Which kernel the 3x3 convolutions take: "auto", "generic" (the planner's GEMM kernels + the epilogue kernel) or "fused"
        (the dense-block kernel everywhere) - a tuning switch, results stay within the same error bound."""
        tuning = isinstance(path, int) and (path & ~0x1f) == 0x100      # 0x100 | mask of shape groups (include/gyre_hip.h)
        if path not in PATHS and path not in PATHS.values() and not tuning:
            raise ValueError(f"path must be one of {sorted(PATHS)}, got {path!r}")
        self._path = PATHS.get(path, path)
        self._path_applied = None

    def _prepare(self, h) -> None:
        if getattr(self, "_path_applied", None) != (h, self._path):
            _lib.check(self._L().gyre_rrdb_set_path(C.c_void_p(h), self._path), self._L())
            self._path_applied = (h, self._path)

    def _destroy(self):
        super()._destroy()
        self._path_applied = None

    def out_shape(self, shape):
        B, _, H, W = shape
        r = _UNSHUFFLE[self.config.scale]
        return (B, self.config.num_out_ch, H // r * 4, W // r * 4)

    def _padding(self, H, W):
        r = _UNSHUFFLE[self.config.scale]
        if H % r or W % r or H < r or W < r:
            raise ValueError(f"image height and width must be multiples of {r} for scale {self.config.scale}, got {H} x {W}")
        return 0, 0


class _WindowUpscaler(_NativeUpscaler):
    """The two window transformers: the same output shape and the same head of the C configuration."""

    def _c_trunk(self, cfg):
        c = self.config
        cfg.in_chans, cfg.embed_dim, cfg.num_layers = c.in_chans, c.embed_dim, len(c.depths)
        for i, (d, h) in enumerate(zip(c.depths, c.num_heads)):
            cfg.depths[i], cfg.num_heads[i] = d, h
        cfg.window_size, cfg.mlp_hidden, cfg.upscale = c.window_size, int(c.embed_dim * c.mlp_ratio), c.upscale
        cfg.img_range = float(c.img_range)
        return cfg

    def out_shape(self, shape):
        B, _, H, W = shape
        return (B, self.config.in_chans, H * self.config.upscale, W * self.config.upscale)


class GyreHipSwinIR(_WindowUpscaler):
    """Drop-in for the reference's ``SwinIR`` with upsampler "nearest+conv": ``forward(x) -> tensor``, NCHW in and out.  The state
    dict carries the reference's names, its buffers included (``attn.relative_position_index``, the shifted blocks' ``attn_mask``), so
    a real checkpoint loads strictly; the buffers' values are never read - the kernel computes index and mask from the window position."""

    _kind = "swinir"
    _make_config, _param_shapes = staticmethod(swinir_config), staticmethod(swinir_param_shapes)
    _is_buffer = staticmethod(swinir_is_buffer)
    _buffer_dtype = staticmethod(lambda leaf: torch.long if leaf == "relative_position_index" else torch.float32)

    def _c_cfg(self):
        cfg = self._c_trunk(_lib.SwinIRCfg())
        cfg.resi_3conv = int(self.config.resi_connection == "3conv")
        return cfg

    def _padding(self, H, W):
        ph, pw = -H % 8, -W % 8
        if ph >= H or pw >= W:                                           # (torch's reflect padding needs pad < size)
            raise ValueError(f"an image of {H} x {W} is too small to reflect-pad to a multiple of the window size 8")
        return ph, pw


class GyreHipHAT(_WindowUpscaler):
    """Drop-in for the reference's ``HAT`` with upsampler "pixelshuffle": ``forward(x) -> tensor``, NCHW in and out.  The state dict
    carries the reference's names, its two global buffers included (``relative_position_index_SA`` / ``_OCA``), so a real checkpoint
    loads strictly; the buffers' values are never read - the kernel computes both indices and the mask from the window position.
    Like the reference, the model has no padding: H and W must be multiples of the window size 16 (``tile()`` cuts multiples of 32)."""

    _kind = "hat"
    _make_config, _param_shapes = staticmethod(hat_config), staticmethod(hat_param_shapes)
    _is_buffer = staticmethod(hat_is_buffer)

    def _c_cfg(self):
        c, cfg = self.config, self._c_trunk(_lib.HATCfg())
        cfg.compress_ratio, cfg.squeeze_factor = c.compress_ratio, c.squeeze_factor
        cfg.conv_scale, cfg.overlap_ratio = float(c.conv_scale), float(c.overlap_ratio)
        return cfg

    def _padding(self, H, W):
        if H < 16 or W < 16 or H % 16 or W % 16:
            raise ValueError(f"HAT takes images whose height and width are multiples of the window size 16, got {H} x {W}")
        return 0, 0


# ---- loader ----------------------------------------------------------------------------------------------------------------------------
CONFIG_PATTERN = ["*.yaml"]
MODELS_PATTERN = ["*.safetensors", "*.pt", "*.pth"]
# default configuration per name, the values the reference uses for the family (the published inference settings of ESRGAN and
# Real-ESRGAN, of SwinIR's real-world x4 models and of HAT / HAT-L x4)
DEFAULT_CONFIGS = {k: dict(v) for k, v in {**RRDB_DEFAULTS, **SWINIR_DEFAULTS, **HAT_DEFAULTS}.items()}

# Old-format ESRGAN checkpoints (the original xinntao/ESRGAN release) name the same tensors by their position in an nn.Sequential:
# the trunk convolutions sit at fixed indices, the RRDBs under model.1.sub.{i}, the convolution that closes the trunk right behind
# the last RRDB, and every dense-block convolution is wrapped in a one-element Sequential (hence the ".0").
_OLD_TRUNK = {"conv_first": "model.0", "conv_up1": "model.3", "conv_up2": "model.6", "conv_hr": "model.8", "conv_last": "model.10"}
_DENSE_KEY = re.compile(r"body\.(\d+)\.rdb([123])\.(conv[1-5]|conv1x1)")


def old_esrgan_key(key: str, num_block: int) -> str:
    """The old-format name of the tensor BasicSR calls ``key`` in a net of ``num_block`` RRDBs."""
    layer, _, leaf = key.rpartition(".")
    m = _DENSE_KEY.fullmatch(layer)
    if m:
        i, j, conv = m.groups()
        wrapped = "" if conv == "conv1x1" else ".0"
        return f"model.1.sub.{i}.RDB{j}.{conv}{wrapped}.{leaf}"
    if layer == "conv_body":
        return f"model.1.sub.{num_block}.{leaf}"
    return f"{_OLD_TRUNK[layer]}.{leaf}"


def convert_old_esrgan(state_dict: dict, shapes: dict, num_block: int) -> dict:
    """A state dict for ``shapes`` ({BasicSR key: shape}) out of an old-format one.  A ``module.`` prefix (DataParallel) is dropped;
    a tensor already stored under its BasicSR name with the right shape is taken as it is; everything else is looked up under
    its old name.  A tensor that is missing, or one the model has no use for, is a ValueError naming it."""
    source = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    converted, missing = {}, []
    for key, shape in shapes.items():
        have = source.get(key)
        name = key if have is not None and tuple(have.shape) == tuple(shape) else old_esrgan_key(key, num_block)
        if name in source:
            converted[key] = source.pop(name)
        else:
            missing.append(name)
    problems = [f"Missing tensor: {n} not found" for n in missing]
    if source:
        problems.append(f"Unconverted tensors remain after converting: {sorted(source)}")
    if problems:
        raise ValueError("\n".join(problems))
    return converted


def _only_match(folder, what, patterns, allow_patterns, ignore_patterns) -> str:
    """The one file of ``folder`` that matches a pattern and passes the allow / ignore filters; none or several: FileNotFoundError."""
    as_list = lambda v: [v] if isinstance(v, str) else list(v)
    names = sorted({os.path.basename(p) for pat in patterns for p in glob.glob(os.path.join(folder, pat))})
    if allow_patterns is not None:
        names = [n for n in names if any(fnmatch.fnmatch(n, a) for a in as_list(allow_patterns))]
    if ignore_patterns is not None:
        names = [n for n in names if not any(fnmatch.fnmatch(n, a) for a in as_list(ignore_patterns))]
    if len(names) != 1:
        raise FileNotFoundError(f"No {what} found at {folder}" if not names else
                                f"Several {what}s found at {folder} ({names}): narrow it with allow_patterns or ignore_patterns")
    return os.path.join(folder, names[0])


def _read_state_dict(path: str) -> dict:
    if path.endswith(".safetensors"):
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as f:
            return {k: f.get_tensor(k) for k in f.keys()}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd["state_dict"] if "meta" in sd and "state_dict" in sd else sd


def _merged_config(folder, network, config, allow_patterns, ignore_patterns) -> dict:
    """The constructor arguments of a load, weakest first: the caller's keywords, the default table entry named by the keyword
    ``config`` (or else by the network), the one ``*.yaml`` of the folder when there is one - the reference's precedence."""
    merged = dict(config)
    merged.update(DEFAULT_CONFIGS.get(merged.pop("config", network), {}))
    try:
        yaml_path = _only_match(folder, "config", CONFIG_PATTERN, allow_patterns, ignore_patterns)
    except FileNotFoundError:
        return merged
    import yaml
    with open(yaml_path) as f:
        merged.update(yaml.safe_load(f) or {})
    return merged


class GyreHipUpscalerLoader:
    """The reference ``UpscalerLoader``'s surface for the ESRGAN, SwinIR and HAT families: ``load`` and one classmethod per engine ``class:`` name
    (ENTRY_POINTS below).  The model's ``_scale`` and ``_window_size`` - what the pipeline reads - come from the model itself."""

    convert_old_esrgan = staticmethod(convert_old_esrgan)

    @classmethod
    def load(cls, path, torch_dtype="auto", low_cpu_mem_usage=False, allow_patterns=None, ignore_patterns=None,
             network="esrgan", converter=None, **config):
        if network not in ("esrgan", "esrgan-plus", "swinir", "hat"):
            raise ValueError(f"Unknown upscaler network kind {network}")
        if converter not in (None, "esrgan-old"):
            raise ValueError(f"Unknown converter {converter}")
        merged = _merged_config(path, network, config, allow_patterns, ignore_patterns)
        if network == "hat":
            model = GyreHipHAT(**merged)
        else:
            model = GyreHipSwinIR(**merged) if network == "swinir" else GyreHipRRDBNet(plus=network == "esrgan-plus", **merged)
        weights_file = _only_match(path, "model", MODELS_PATTERN, allow_patterns, ignore_patterns)
        tensors = _read_state_dict(weights_file)
        tensors = tensors.get("params_ema", tensors)               # Real-ESRGAN training files keep the EMA weights under this key
        if converter == "esrgan-old":
            tensors = convert_old_esrgan(tensors, rrdb_param_shapes(model.config), model.config.num_block)
        model.load_state_dict(tensors)
        model._source = path
        return (model if torch_dtype == "auto" else model.to(torch_dtype)).eval()


# engine ``class:`` name -> the arguments of load() it fixes
ENTRY_POINTS = {"esrgan": dict(network="esrgan"),
                "esrgan_old": dict(network="esrgan", converter="esrgan-old"),
                "esrgan_plus": dict(network="esrgan-plus", converter="esrgan-old"),
                "realesrgan": dict(network="esrgan"),
                "realesrgan_6B": dict(network="esrgan", config="esrgan-6B"),
                "swinir": dict(network="swinir"), "swinir_l": dict(network="swinir", config="swinir-l"),
                "hat": dict(network="hat"), "hat_l": dict(network="hat", config="hat-l")}


def _entry_point(fixed):
    def call(cls, *args, **kwargs):
        return cls.load(*args, **fixed, **kwargs)
    return classmethod(call)


for _name, _fixed in ENTRY_POINTS.items():
    setattr(GyreHipUpscalerLoader, _name, _entry_point(_fixed))


# ---- tiling ----------------------------------------------------------------------------------------------------------------------------
def _tile_count(tile_size: int, padded: int, min_overlap: float) -> int:
    """Fewest tiles (at least two when one does not cover the padded side) whose even spread overlaps by min_overlap pixels."""
    if tile_size >= padded:
        return 1
    n = 2
    while (tile_size * n - padded) / (n - 1) < min_overlap:
        n += 1
    return n


def tile_plan(ih: int, iw: int, scale, tile_size: int, tile_overlap=0.25, window_size: int = 32, pad_size=None, feather=None):
    """Geometry of a tiled call over an ih x iw image that does not fit one tile, as the reference lays it out: the tile shrinks
    to the largest multiple of window_size inside the image, the image is padded by pad_size (default window_size) per side, each
    axis gets the fewest evenly spread tiles that overlap by tile_overlap of a tile, and the blend feathers over `feather` input
    pixels (default pad_size).  Returns (tile_size, pad_size, half feather width in OUTPUT pixels, y offsets, x offsets)."""
    if tile_size % window_size:
        raise ValueError(f"Tile size {tile_size} needs to be multiple of {window_size}")
    tile_size = min(tile_size, ih // window_size * window_size, iw // window_size * window_size)
    pad_size = window_size if pad_size is None else pad_size
    feather = pad_size if feather is None else feather
    if pad_size < feather:
        raise ValueError("Pad size must equal or exceed feather size")
    if tile_overlap * tile_size < feather:
        raise ValueError(f"Tile overlap ({tile_overlap * tile_size}) must equal or exceed feather size {feather}")
    offsets = []
    for side in (ih, iw):
        padded = side + 2 * pad_size
        n = _tile_count(tile_size, padded, tile_overlap * tile_size)
        offsets.append([int(v) for v in np.linspace(0, padded - tile_size, n).round().astype(np.uint32)])
    # the feather is laid out on the output; the blur spreads it to both sides of the edge of the white square, so that square
    # reaches to the middle of the feather band
    half = round(feather * scale) // 2 if feather else 0
    return tile_size, pad_size, half, offsets[0], offsets[1]


def feather_map(out_tile: int, half: int, like: torch.Tensor) -> Optional[torch.Tensor]:
    """[1, 1, out_tile, out_tile] blend weight of a new tile over what is already there: ones with a zero border of `half` pixels,
    blurred with sigma = half / 3."""
    if not half:
        return None
    inner = out_tile - 2 * half
    fm = torch.nn.functional.pad(torch.ones([1, 1, inner, inner]).to(like), (half,) * 4, "constant", 0)
    return images.gaussianblur(fm, half / 3)


def tile(input: torch.Tensor, module, scale, tile_size: int, tile_overlap=0.25, window_size: int = 32, pad_size=None,
         pad_mode="reflect", feather=None, stacked: bool = True, max_stack: int = 16) -> torch.Tensor:
    """``module`` over ``input`` [B, C, H, W] in overlapping tiles, blended one after the other in row-major order (what the
    reference's ``tile`` computes, fp32 bit for bit on a torch module).  An image that fits one tile goes through untiled.
    stacked: the tiles go through the module as stacked batches (tile-major) of at most max_stack tiles - the module's workspace
    grows with the batch, about 0.27 GB per 256 x 256 tile at x4 - then the same sequential blend; False calls it tile by tile."""
    if input.ndim != 4:
        raise ValueError("Tile input must be in BCHW format")
    if tile_size % window_size:
        raise ValueError(f"Tile size {tile_size} needs to be multiple of {window_size}")
    ih, iw = input.shape[-2:]
    if tile_size >= ih and tile_size >= iw:
        return module(input)
    tile_size, pad_size, half, ys, xs = tile_plan(ih, iw, scale, tile_size, tile_overlap, window_size, pad_size, feather)
    padded = torch.nn.functional.pad(input, (pad_size,) * 4, pad_mode)
    out_tile, B = tile_size * scale, input.shape[0]
    fmap = feather_map(out_tile, half, input)
    windows = [(y, x) for y in ys for x in xs]
    cut = lambda y, x: padded[:, :, y:y + tile_size, x:x + tile_size]
    if stacked:
        pieces, group = [], max(1, int(max_stack))
        for k0 in range(0, len(windows), group):
            part = module(torch.cat([cut(y, x) for y, x in windows[k0:k0 + group]], dim=0).contiguous())
            pieces += list(part.split(B, dim=0))
    else:
        pieces = [module(cut(y, x).contiguous()) for y, x in windows]
    first = pieces[0]
    canvas = torch.zeros(first.shape[0], first.shape[1], *images.scale_shape(padded.shape, scale)[-2:]).to(first)
    for (y, x), new in zip(windows, pieces):
        if new.shape[:2] != first.shape[:2]:
            raise ValueError("the module changed its batch or channel count between tiles")
        region = (slice(None), slice(None), slice(y * scale, y * scale + out_tile), slice(x * scale, x * scale + out_tile))
        canvas[region] = new if fmap is None else new * fmap + canvas[region] * (1 - fmap)
    o = pad_size * scale
    return canvas[:, :, o:o + ih * scale, o:o + iw * scale]


class GyreUpscalerPipeline:
    """The reference's ``UpscalerPipeline``: ``pipeline(image, width, height) -> (tensor,)`` over a float image in [0, 1] with 3 or
    4 channels.  tile_size (the reference fixes 256), the other keywords of ``tile`` (tile_overlap, pad_size, feather) and stacked
    are keywords for tests and tuning.  Like the reference, a tile whose overlap (a quarter of it) is smaller than the 32-pixel
    feather is refused: with the defaults that is every tile size below 128, which an image between 64 and 127 pixels on its
    shorter side and larger than the tile on the other reaches - the reference fails on those images too."""

    _meta = {"offload_capable": False}

    def __init__(self, module):
        self.module = module

    def to(self, device):
        self.module.to(device)
        return self

    @torch.no_grad()
    def __call__(self, image=None, width=None, height=None, tile_size: int = 256, stacked: bool = True, tile_overlap=0.25,
                 pad_size=None, feather=None, max_stack: int = 16, **kwargs):
        if image is not None and not torch.is_tensor(image) and hasattr(image, "getbands"):      # a PIL image, as the reference accepts
            image = images.from_pil(image)
        if not torch.is_tensor(image) or image.ndim != 4:
            raise ValueError("the upscaler pipeline takes a PIL image or a float image tensor [B, 3 or 4, H, W] in [0, 1]")
        if height == image.shape[-2] and width == image.shape[-1]:
            height = width = None                     # a requested size equal to the input's means "no final rescale"
        p = next(self.module.parameters())
        sample = image.to(p.device, p.dtype)
        colour, alpha = sample[:, 0:3], (sample[:, [3]] if sample.shape[1] == 4 else None)
        scale = getattr(self.module, "_scale", 4)
        result = tile(colour, self.module, scale, tile_size, tile_overlap=tile_overlap, pad_size=pad_size, feather=feather,
                      stacked=stacked, max_stack=max_stack).clamp(0, 1)
        if alpha is not None:
            levels = alpha.unique_consecutive()
            if len(levels) == 1:                      # a constant plane is replicated, not resampled
                up = torch.ones(images.scale_shape(alpha.shape, scale)).to(result) * levels[0]
            else:
                up = images.resize(alpha, scale).to(result)
            result = torch.cat([result, up], dim=1)
        if width is not None and height is not None:
            result = images.rescale(result, height, width, "cover")
        return (result.to(image),)
