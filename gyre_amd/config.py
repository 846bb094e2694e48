"""Model hyper-parameters for the native UNet / VAE.

The SD1.x constants are the ones the reference pins in-tree at
``gyre/ldm_config/v1-inference.yaml:29-64`` (UNet: model_channels 320,
channel_mult [1,2,4,4], 2 res blocks, attention at the first three levels,
8 heads, context_dim 768; VAE: ch 128, ch_mult [1,2,4,4], z=4, double_z).
Field names follow the diffusers ``config.json`` keys the reference reads
(``unified_pipeline.py:186`` in_channels, ``:1318`` sample_size,
``:1402`` block_out_channels).
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Tuple


@dataclass(frozen=True)
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    attn_levels: Tuple[bool, ...] = (True, True, True, False)
    num_heads: Tuple[int, ...] = (8, 8, 8, 8)
    cross_attention_dim: int = 768
    norm_num_groups: int = 32
    transformer_depth: Tuple[int, ...] = (1, 1, 1, 1)
    use_linear_projection: bool = False
    sample_size: int = 64
    flip_sin_to_cos: bool = True
    freq_shift: float = 0.0
    # SDXL "text_time" added conditioning (None for SD1.x/2.x)
    addition_embed_type: str | None = None
    addition_time_embed_dim: int = 256
    projection_class_embeddings_input_dim: int = 2816
    _diffusers_version: str = "0.16.0"

    @property
    def time_embed_dim(self) -> int:
        return self.block_out_channels[0] * 4

    def to_dict(self):
        return asdict(self)


@dataclass(frozen=True)
class VAEConfig:
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215
    sample_size: int = 512

    def to_dict(self):
        return asdict(self)


def sd15_unet(in_channels: int = 4) -> UNetConfig:
    """SD1.x UNet (in_channels=9 for the runway inpainting variant,
    reference unified_pipeline.py:648-696)."""
    return UNetConfig(in_channels=in_channels)


def sd15_vae() -> VAEConfig:
    return VAEConfig()


def tiny_unet(in_channels: int = 4) -> UNetConfig:
    """Same topology as SD1.x at 1/10 width - for parity tests that must run in
    seconds on the CPU oracle.  Channels stay multiples of 32 (GroupNorm groups)
    and head dims multiples of 8 (vector loads)."""
    return UNetConfig(in_channels=in_channels, block_out_channels=(32, 64, 128, 128),
                      num_heads=(2, 2, 4, 4), cross_attention_dim=64, sample_size=16)


def sdxl_unet() -> UNetConfig:
    """SDXL-base UNet (BASELINE config 4; not in the reference - an extension on the same kernel set): 3 levels,
    transformer depth 0/2/10, head dim 64, context 2048, linear projections, text_time added conditioning."""
    return UNetConfig(block_out_channels=(320, 640, 1280), attn_levels=(False, True, True), num_heads=(5, 10, 20),
                      transformer_depth=(1, 2, 10), cross_attention_dim=2048, use_linear_projection=True,
                      sample_size=128, addition_embed_type="text_time")


def tiny_sdxl_unet() -> UNetConfig:
    return UNetConfig(block_out_channels=(32, 64, 128), attn_levels=(False, True, True), num_heads=(2, 2, 4),
                      transformer_depth=(1, 2, 3), cross_attention_dim=64, use_linear_projection=True, sample_size=16,
                      addition_embed_type="text_time", addition_time_embed_dim=8,
                      projection_class_embeddings_input_dim=32 + 6 * 8)


def sdxl_vae() -> VAEConfig:
    """SDXL's AutoencoderKL: same topology as SD1.x, latent scaling 0.13025, 1024 px sample size."""
    return VAEConfig(scaling_factor=0.13025, sample_size=1024)


def tiny_vae() -> VAEConfig:
    return VAEConfig(block_out_channels=(32, 64, 64, 64), sample_size=64)


@dataclass(frozen=True)
class ControlNetConfig:
    """diffusers ``ControlNetModel`` config.json fields the native control model reads: the encoder half of the UNet's, the channels
    of the hint image and the widths of its conditioning embedding.  Also answers ``config.get(name, default)`` - the reference asks
    ``controlnet.config.get("global_pool_conditions", False)`` (unified_pipeline.py:983)."""
    in_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    attn_levels: Tuple[bool, ...] = (True, True, True, False)
    num_heads: Tuple[int, ...] = (8, 8, 8, 8)
    cross_attention_dim: int = 768
    norm_num_groups: int = 32
    transformer_depth: Tuple[int, ...] = (1, 1, 1, 1)
    use_linear_projection: bool = False
    flip_sin_to_cos: bool = True
    freq_shift: float = 0.0
    conditioning_channels: int = 3
    conditioning_embedding_out_channels: Tuple[int, ...] = (16, 32, 96, 256)
    controlnet_conditioning_channel_order: str = "rgb"
    global_pool_conditions: bool = False
    _diffusers_version: str = "0.16.0"

    @property
    def time_embed_dim(self) -> int:
        return self.block_out_channels[0] * 4

    @property
    def n_residuals(self) -> int:
        """down residuals: conv_in, one per layer, one per downsampler (12 for SD1.x); the mid residual comes on top"""
        n = len(self.block_out_channels)
        return 1 + n * self.layers_per_block + (n - 1)

    def get(self, name, default=None):
        return getattr(self, name, default)

    def __contains__(self, name):
        return hasattr(self, name)

    def to_dict(self):
        return asdict(self)


def sd15_controlnet(**kw) -> ControlNetConfig:
    """The SD1.x ControlNet (lllyasviel/sd-controlnet-*, control_v11*): SD1.x encoder, 3-channel hint, embedding 16/32/96/256."""
    return ControlNetConfig(**kw)


def tiny_controlnet(**kw) -> ControlNetConfig:
    """The same topology at the widths of tiny_unet, conditioning embedding 16/32/48/64."""
    return ControlNetConfig(**{**dict(block_out_channels=(32, 64, 128, 128), num_heads=(2, 2, 4, 4), cross_attention_dim=64,
                                      conditioning_embedding_out_channels=(16, 32, 48, 64)), **kw})


class _AttrDict(dict):
    """A mapping that also reads as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class T2IConfig(_AttrDict):
    """Configuration of a T2I adapter: a mapping that also reads as attributes - the reference asks both ``"cin" in
    model.config`` and ``model.config.cin`` (unified_pipeline.py:869)."""


# the reference's per-type defaults (t2i_adapter/models.py:82-89, 187-191)
T2I_DEFAULTS = {"main": dict(cin=192, channels=(320, 640, 1280, 1280), nums_rb=2, ksize=1, sk=True, use_conv=False),
                "light": dict(cin=192, channels=(320, 640, 1280, 1280), nums_rb=4)}


def t2i_config(type: str = "main", **kw) -> T2IConfig:
    if type not in T2I_DEFAULTS:
        raise NotImplementedError(f"T2I adapter type {type!r} (style adapters and the co-adapter fuser are outside the native path)")
    cfg = T2IConfig(type=type, **{**T2I_DEFAULTS[type], **kw})
    cfg["channels"] = tuple(cfg["channels"])
    return cfg


def tiny_t2i(kind: str = "main", **kw) -> T2IConfig:
    """The reference's default adapter of the given kind at the widths of tiny_unet."""
    return t2i_config(kind, **{"channels": (32, 64, 128, 128), **kw})


# the reference's defaults for its two token-sequence networks (t2i_adapter/models.py: T2iAdapter_style, CoAdapterFuser; adapter.py:175, 267)
T2I_STYLE_DEFAULTS = dict(width=1024, context_dim=768, num_head=8, n_layes=3, num_token=8)
T2I_FUSER_DEFAULTS = dict(unet_channels=(320, 640, 1280, 1280), width=768, num_head=8, n_layes=3)
T2I_SEQ_HEAD_DIMS = (32, 64, 96, 128)            # what the attention kernel is built for (csrc/kernels_seq.hip)
# adapter.py ExtraCondition: the row of the fuser's task_embedding a co-adapter of that kind adds
EXTRA_CONDITION = {"sketch": 0, "keypose": 1, "seg": 2, "depth": 3, "canny": 4, "style": 5, "color": 6, "openpose": 7}


def _t2i_seq_config(type: str, defaults: dict, kw: dict) -> T2IConfig:
    unknown = set(kw) - set(defaults)
    if unknown:
        raise TypeError(f"unknown {type} configuration keys: {sorted(unknown)}")
    cfg = T2IConfig(type=type, **{**defaults, **kw})
    if cfg["num_head"] < 1 or cfg["width"] % cfg["num_head"] or cfg["width"] // cfg["num_head"] not in T2I_SEQ_HEAD_DIMS:
        raise NotImplementedError(f"{type}: width / num_head must be one of {T2I_SEQ_HEAD_DIMS}, got {cfg['width']} / {cfg['num_head']}")
    return cfg


def t2i_style_config(**kw) -> T2IConfig:
    """StyleAdapter(width, context_dim, num_head, n_layes, num_token) at the reference's defaults."""
    return _t2i_seq_config("style", T2I_STYLE_DEFAULTS, kw)


def t2i_fuser_config(**kw) -> T2IConfig:
    """CoAdapterFuser(unet_channels, width, num_head, n_layes) at the reference's defaults."""
    cfg = _t2i_seq_config("fuser", T2I_FUSER_DEFAULTS, kw)
    cfg["unet_channels"] = tuple(cfg["unet_channels"])
    if len(cfg["unet_channels"]) != 4 or any(c < 8 or c % 8 for c in cfg["unet_channels"]):
        raise NotImplementedError("fuser: four channel counts, each a positive multiple of 8")
    return cfg


def tiny_t2i_style(**kw) -> T2IConfig:
    return t2i_style_config(**{**dict(width=64, context_dim=64, num_head=2, n_layes=2, num_token=3), **kw})


def tiny_t2i_fuser(**kw) -> T2IConfig:
    return t2i_fuser_config(**{**dict(unet_channels=(32, 64, 128, 128), width=64, num_head=2, n_layes=2), **kw})


class RRDBConfig(_AttrDict):
    """Configuration of an RRDBNet upscaler (BasicSR ``RRDBNet(num_in_ch, num_out_ch, scale, num_feat, num_block, num_grow_ch)``
    plus ``plus`` for the reference's ESRGAN+ blocks): a mapping that also reads as attributes."""


# the reference's default configurations (gyre/pipeline/upscalers/upscaler_loader.py:22-40)
RRDB_DEFAULTS = {"esrgan": dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32, scale=4),
                 "esrgan-6B": dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=6, num_grow_ch=32, scale=4)}
RRDB_DEFAULTS["esrgan-plus"] = RRDB_DEFAULTS["esrgan"]


def rrdb_config(plus: bool = False, **kw) -> RRDBConfig:
    """BasicSR's own constructor defaults (scale=4, num_feat=64, num_block=23, num_grow_ch=32) under ``kw``.  Only num_feat = 64
    and num_grow_ch = 32 are built natively - the widths of every configuration the reference ships."""
    cfg = RRDBConfig(**{**dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32), **kw}, plus=bool(plus))
    if cfg["num_feat"] != 64 or cfg["num_grow_ch"] != 32:
        raise NotImplementedError("RRDBNet: num_feat = 64 and num_grow_ch = 32 are the only widths on the native path")
    if cfg["scale"] not in (1, 2, 4):
        raise NotImplementedError(f"RRDBNet: scale must be 1, 2 or 4, got {cfg['scale']}")
    return cfg


def tiny_rrdb(**kw) -> RRDBConfig:
    """Two RRDBs (six dense blocks, the third-block epilogue included) at the only widths the family has."""
    return rrdb_config(**{"num_block": 2, **kw})


class LineartConfig(_AttrDict):
    """Configuration of the line-art hinter - the arguments of the reference's ``DrawingGenerator`` constructor
    (gyre/pipeline/hinters/models/informative_drawings.py:57): a mapping that also reads as attributes."""


def lineart_config(input_nc: int, output_nc: int, n_residual_blocks: int = 9, sigmoid: bool = True, **kw) -> LineartConfig:
    """The constructor's defaults, refused (NotImplementedError) outside what the native path builds: input_nc 3, output_nc 1 and
    1 to 16 residual blocks (every configuration the reference ships is 3 / 1 / 3).  A keyword that is not a constructor argument
    is refused too."""
    if kw:
        raise NotImplementedError(f"DrawingGenerator: {sorted(kw)} are not arguments of the DrawingGenerator constructor "
                                  f"(a configuration of another model family?)")
    cfg = LineartConfig(input_nc=int(input_nc), output_nc=int(output_nc), n_residual_blocks=int(n_residual_blocks), sigmoid=bool(sigmoid))
    if cfg["input_nc"] != 3 or cfg["output_nc"] != 1:
        raise NotImplementedError(f"DrawingGenerator: input_nc {input_nc} / output_nc {output_nc} is outside the native path (3 / 1 is built)")
    if not 1 <= cfg["n_residual_blocks"] <= 16:
        raise NotImplementedError(f"DrawingGenerator: n_residual_blocks {n_residual_blocks} is outside the native path (1 to 16 are built)")
    return cfg


def tiny_lineart(**kw) -> LineartConfig:
    """One residual block, no sigmoid: every kind of layer the generator has, once."""
    return lineart_config(**{**dict(input_nc=3, output_nc=1, n_residual_blocks=1, sigmoid=False), **kw})


class HedConfig(_AttrDict):
    """Configuration of the HED edge detector: the reference's ``HED`` (gyre/pipeline/hinters/models/hed.py) takes no constructor
    arguments, so the mapping holds the one fact its shell asks for - the three input channels."""


def hed_config(**kw) -> HedConfig:
    if kw:
        raise NotImplementedError(f"HED: {sorted(kw)} are not arguments of the HED constructor, which has none "
                                  f"(a configuration of another model family?)")
    return HedConfig(input_nc=3)


class MlsdConfig(_AttrDict):
    """Configuration of the MLSD line detector: the reference's ``MobileV2_MLSD_Large`` (gyre/pipeline/hinters/models/
    mbv2_mlsd_large.py) takes no constructor arguments, so the mapping holds the one fact its shell asks for - the four input channels
    (RGB and a constant plane)."""


def mlsd_config(**kw) -> MlsdConfig:
    if kw:
        raise NotImplementedError(f"MobileV2_MLSD_Large: {sorted(kw)} are not arguments of its constructor, which has none "
                                  f"(a configuration of another model family?)")
    return MlsdConfig(input_nc=4)


# the MobileNetV2 trunk of MLSD, cut after features[13]: (t, c, n, s) = expansion, width, repeats, stride of the first repeat
MLSD_SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1))


def mlsd_size_ok(n: int) -> bool:
    """the image sides the network takes: those at which the reference's own concatenations line up"""
    return n >= 16 and (n // 2) % 8 == 0


# the VGG trunk of HED: convolutions per stage and their width
HED_STAGES = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
HED_BORDER = 34                    # conv1_1's padding 35, less the ordinary 1


class SwinIRConfig(_AttrDict):
    """Configuration of a SwinIR upscaler - the keyword arguments of the reference's ``SwinIR`` constructor
    (gyre/pipeline/upscalers/models/network_swinir.py:651-657): a mapping that also reads as attributes."""


# the reference's default configurations (gyre/pipeline/upscalers/upscaler_loader.py:43-69)
SWINIR_DEFAULTS = {
    "swinir": dict(upscale=4, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6, 6, 6, 6, 6, 6], embed_dim=180,
                   num_heads=[6, 6, 6, 6, 6, 6], mlp_ratio=2, upsampler="nearest+conv", resi_connection="1conv"),
    "swinir-l": dict(upscale=4, in_chans=3, img_size=64, window_size=8, img_range=1.0, depths=[6, 6, 6, 6, 6, 6, 6, 6, 6], embed_dim=240,
                     num_heads=[8, 8, 8, 8, 8, 8, 8, 8, 8], mlp_ratio=2, upsampler="nearest+conv", resi_connection="3conv")}

# SwinIR.__init__'s own defaults: what a key the caller leaves out means
_SWINIR_CTOR = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=[6, 6, 6, 6], num_heads=[6, 6, 6, 6], window_size=7,
                    mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=None,
                    ape=False, patch_norm=True, use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="1conv")


def _window_transformer_config(cls, family, ctor, window, kw, before_patch, before_flags):
    """What swinir_config and hat_config share: the constructor's defaults under ``kw`` (a key that is no constructor argument is
    refused), then the refusals in the order the two families always made them - the window, the family's ``before_patch(cfg,
    refuse)``, patch_size / in_chans, the family's ``before_flags(cfg, refuse)`` (upsampler and residual connection), and what the
    trunk of both needs: ape / patch_norm / qkv_bias / qk_scale, the norm layer, depths and heads, the MLP width, img_range."""
    unknown = sorted(set(kw) - set(ctor))
    if unknown:
        raise NotImplementedError(f"{family}: {unknown} are not arguments of the {family} constructor (a configuration of another model family?)")
    cfg = cls(**{**ctor, **kw})
    cfg["depths"], cfg["num_heads"] = [int(d) for d in cfg["depths"]], [int(h) for h in cfg["num_heads"]]

    def refuse(why):
        raise NotImplementedError(f"{family}: {why} is outside the native path")

    if cfg["window_size"] != window:
        refuse(f"window_size {cfg['window_size']} ({window} is built)")
    before_patch(cfg, refuse)
    if cfg["patch_size"] != 1 or cfg["in_chans"] != 3:
        refuse("patch_size other than 1 or in_chans other than 3")
    before_flags(cfg, refuse)
    if cfg["ape"] or not cfg["patch_norm"] or not cfg["qkv_bias"] or cfg["qk_scale"] is not None:
        refuse("ape=True, patch_norm=False, qkv_bias=False or a qk_scale")
    if cfg["norm_layer"] is not None and cfg["norm_layer"] is not __import__("torch").nn.LayerNorm:
        refuse("a norm_layer other than LayerNorm")
    heads, depths = cfg["num_heads"], cfg["depths"]
    if not depths or len(depths) != len(heads) or len(depths) > 16 or min(depths) < 1:
        refuse(f"depths {depths} with num_heads {heads} (1 to 16 layers, one head count per layer)")
    if len(set(heads)) != 1 or not 1 <= heads[0] <= 8 or cfg["embed_dim"] != 30 * heads[0]:
        refuse(f"embed_dim {cfg['embed_dim']} with num_heads {heads} (embed_dim = 30 * heads, the same 1 to 8 heads in every layer)")
    hidden = int(cfg["embed_dim"] * cfg["mlp_ratio"])
    if hidden < 8 or hidden % 8:
        refuse(f"an MLP width of {hidden} (multiples of 8 are built)")
    if not float(cfg["img_range"]) > 0:
        raise ValueError(f"{family}: img_range must be positive")
    return cfg


def swinir_config(**kw) -> SwinIRConfig:
    """The constructor's defaults under ``kw``, refused (NotImplementedError) outside what the native path builds: window 8,
    embed_dim = 30 * heads with one head count (at most 8) for all layers, an MLP width that is a multiple of 8, "nearest+conv" with
    upscale 2 or 4, "1conv" / "3conv", ape=False, patch_norm=True, qkv_bias=True, in_chans=3.  A key that is not a constructor
    argument is refused too - the reference swallows it in ``**kwargs``; here a folder of another model family fails at its
    configuration instead of at load_state_dict."""
    def img_size(cfg, refuse):
        size = cfg["img_size"]
        size = (size, size) if isinstance(size, int) else tuple(size)
        if min(size) <= 8 or size[0] % 8 or size[1] % 8:
            refuse(f"img_size {cfg['img_size']} (multiples of the window above it are built)")

    def upsampler(cfg, refuse):
        if cfg["upsampler"] != "nearest+conv" or cfg["upscale"] not in (2, 4):
            refuse(f"upsampler {cfg['upsampler']!r} at upscale {cfg['upscale']} (nearest+conv at 2 or 4 is built; pixelshuffle, pixelshuffledirect and the denoising form are not)")
        if cfg["resi_connection"] not in ("1conv", "3conv"):
            refuse(f"resi_connection {cfg['resi_connection']!r}")

    return _window_transformer_config(SwinIRConfig, "SwinIR", _SWINIR_CTOR, 8, kw, img_size, upsampler)


def tiny_swinir(**kw) -> SwinIRConfig:
    """Two RSTBs of two blocks (plain and shifted windows, both residual levels) at embed 60 / 2 heads, x4, built for 16 x 16 images."""
    return swinir_config(**{**dict(upscale=4, img_size=16, window_size=8, depths=[2, 2], embed_dim=60, num_heads=[2, 2], mlp_ratio=2,
                                   upsampler="nearest+conv", resi_connection="1conv"), **kw})


class HATConfig(_AttrDict):
    """Configuration of a HAT upscaler - the keyword arguments of the reference's ``HAT`` constructor
    (gyre/pipeline/upscalers/models/hat_arch.py:743-769): a mapping that also reads as attributes."""


# the reference's default configurations (gyre/pipeline/upscalers/upscaler_loader.py DEFAULT_CONFIGS "hat" / "hat-l")
HAT_DEFAULTS = {
    "hat": dict(upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01,
                overlap_ratio=0.5, img_range=1.0, depths=[6, 6, 6, 6, 6, 6], embed_dim=180, num_heads=[6, 6, 6, 6, 6, 6], mlp_ratio=2,
                upsampler="pixelshuffle", resi_connection="1conv"),
    "hat-l": dict(upscale=4, in_chans=3, img_size=64, window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01,
                  overlap_ratio=0.5, img_range=1.0, depths=[6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6], embed_dim=180,
                  num_heads=[6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6, 6], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")}

# HAT.__init__'s own defaults: what a key the caller leaves out means
_HAT_CTOR = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=96, depths=(6, 6, 6, 6), num_heads=(6, 6, 6, 6), window_size=7,
                 compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, norm_layer=None, ape=False, patch_norm=True,
                 use_checkpoint=False, upscale=2, img_range=1.0, upsampler="", resi_connection="1conv")


def hat_config(**kw) -> HATConfig:
    """The constructor's defaults under ``kw``, refused (NotImplementedError) outside what the native path builds: window 16,
    overlap_ratio 0.5, compress_ratio 3, squeeze_factor 30, embed_dim = 30 * heads with one head count (at most 8) for all layers, an
    MLP width that is a multiple of 8, "pixelshuffle" with upscale 2 or 4, "1conv", ape=False, patch_norm=True, qkv_bias=True,
    in_chans=3.  A key that is not a constructor argument is refused too - the reference swallows it in ``**kwargs``; here a folder of
    another model family fails at its configuration instead of at load_state_dict."""
    def ratios(cfg, refuse):
        if cfg["overlap_ratio"] != 0.5 or cfg["compress_ratio"] != 3 or cfg["squeeze_factor"] != 30:
            refuse("an overlap_ratio other than 0.5, a compress_ratio other than 3 or a squeeze_factor other than 30")

    def upsampler(cfg, refuse):
        if cfg["upsampler"] != "pixelshuffle" or cfg["upscale"] not in (2, 4):
            refuse(f"upsampler {cfg['upsampler']!r} at upscale {cfg['upscale']} (pixelshuffle at 2 or 4 is built)")
        if cfg["resi_connection"] != "1conv":
            refuse(f"resi_connection {cfg['resi_connection']!r}")

    return _window_transformer_config(HATConfig, "HAT", _HAT_CTOR, 16, kw, ratios, upsampler)


def tiny_hat(**kw) -> HATConfig:
    """Two RHAGs of two HABs (plain and shifted windows) and their OCABs at embed 60 / 2 heads, x4."""
    return hat_config(**{**dict(upscale=4, window_size=16, depths=[2, 2], embed_dim=60, num_heads=[2, 2], mlp_ratio=2,
                                upsampler="pixelshuffle", resi_connection="1conv"), **kw})
