"""Parameter inventory (diffusers key names + shapes) and seeded synthetic weights.

State-dict keys equal the checkpoint's diffusers names because the reference's
loader falls back to ``Class(**config)`` + ``load_state_dict`` of the single
``*.safetensors`` in the model dir (reference gyre/manager.py:1068-1112), and
``ckpt_utils.py:259-285`` converts ``.ckpt`` files into that key space.

There are no SD weights on the build/bench machines (no network), so benches
and parity tests use ``synthetic_state_dict``: every tensor is drawn from its
own generator seeded by ``seed ^ crc32(key)`` so the values do not depend on
enumeration order.  Fan-in scaling keeps activations O(1) through the whole
network so that parity errors are meaningful (a N(0, 0.02) init would collapse
the signal to zero after a few layers and hide kernel bugs).
"""
from __future__ import annotations

import zlib
from collections import OrderedDict
from typing import Dict, Tuple

import torch

from .config import UNetConfig, VAEConfig

Shapes = "OrderedDict[str, Tuple[int, ...]]"


def _resnet(shapes, p, cin, cout, temb_dim):
    shapes[p + ".norm1.weight"] = (cin,)
    shapes[p + ".norm1.bias"] = (cin,)
    shapes[p + ".conv1.weight"] = (cout, cin, 3, 3)
    shapes[p + ".conv1.bias"] = (cout,)
    if temb_dim:
        shapes[p + ".time_emb_proj.weight"] = (cout, temb_dim)
        shapes[p + ".time_emb_proj.bias"] = (cout,)
    shapes[p + ".norm2.weight"] = (cout,)
    shapes[p + ".norm2.bias"] = (cout,)
    shapes[p + ".conv2.weight"] = (cout, cout, 3, 3)
    shapes[p + ".conv2.bias"] = (cout,)
    if cin != cout:
        shapes[p + ".conv_shortcut.weight"] = (cout, cin, 1, 1)
        shapes[p + ".conv_shortcut.bias"] = (cout,)


def _transformer(shapes, p, c, ctx_dim, depth, linear_proj):
    shapes[p + ".norm.weight"] = (c,)
    shapes[p + ".norm.bias"] = (c,)
    shapes[p + ".proj_in.weight"] = (c, c) if linear_proj else (c, c, 1, 1)
    shapes[p + ".proj_in.bias"] = (c,)
    for d in range(depth):
        b = f"{p}.transformer_blocks.{d}"
        for n in ("norm1", "norm2", "norm3"):
            shapes[f"{b}.{n}.weight"] = (c,)
            shapes[f"{b}.{n}.bias"] = (c,)
        for a, kv in (("attn1", c), ("attn2", ctx_dim)):
            shapes[f"{b}.{a}.to_q.weight"] = (c, c)
            shapes[f"{b}.{a}.to_k.weight"] = (c, kv)
            shapes[f"{b}.{a}.to_v.weight"] = (c, kv)
            shapes[f"{b}.{a}.to_out.0.weight"] = (c, c)
            shapes[f"{b}.{a}.to_out.0.bias"] = (c,)
        shapes[f"{b}.ff.net.0.proj.weight"] = (8 * c, c)
        shapes[f"{b}.ff.net.0.proj.bias"] = (8 * c,)
        shapes[f"{b}.ff.net.2.weight"] = (c, 4 * c)
        shapes[f"{b}.ff.net.2.bias"] = (c,)
    shapes[p + ".proj_out.weight"] = (c, c) if linear_proj else (c, c, 1, 1)
    shapes[p + ".proj_out.bias"] = (c,)


def unet_param_shapes(cfg: UNetConfig) -> Shapes:
    s: Shapes = OrderedDict()
    boc = cfg.block_out_channels
    td = cfg.time_embed_dim
    s["time_embedding.linear_1.weight"] = (td, boc[0])
    s["time_embedding.linear_1.bias"] = (td,)
    s["time_embedding.linear_2.weight"] = (td, td)
    s["time_embedding.linear_2.bias"] = (td,)
    if getattr(cfg, "addition_embed_type", None) == "text_time":
        s["add_embedding.linear_1.weight"] = (td, cfg.projection_class_embeddings_input_dim)
        s["add_embedding.linear_1.bias"] = (td,)
        s["add_embedding.linear_2.weight"] = (td, td)
        s["add_embedding.linear_2.bias"] = (td,)
    s["conv_in.weight"] = (boc[0], cfg.in_channels, 3, 3)
    s["conv_in.bias"] = (boc[0],)
    n = len(boc)
    skip_ch = [boc[0]]
    cin = boc[0]
    for i in range(n):
        for j in range(cfg.layers_per_block):
            _resnet(s, f"down_blocks.{i}.resnets.{j}", cin, boc[i], td)
            cin = boc[i]
            if cfg.attn_levels[i]:
                _transformer(s, f"down_blocks.{i}.attentions.{j}", cin, cfg.cross_attention_dim,
                             cfg.transformer_depth[i], cfg.use_linear_projection)
            skip_ch.append(cin)
        if i < n - 1:
            s[f"down_blocks.{i}.downsamplers.0.conv.weight"] = (cin, cin, 3, 3)
            s[f"down_blocks.{i}.downsamplers.0.conv.bias"] = (cin,)
            skip_ch.append(cin)
    _resnet(s, "mid_block.resnets.0", cin, cin, td)
    _transformer(s, "mid_block.attentions.0", cin, cfg.cross_attention_dim, cfg.transformer_depth[-1],
                 cfg.use_linear_projection)
    _resnet(s, "mid_block.resnets.1", cin, cin, td)
    for i in range(n):
        lvl = n - 1 - i
        for j in range(cfg.layers_per_block + 1):
            sk = skip_ch.pop()
            _resnet(s, f"up_blocks.{i}.resnets.{j}", cin + sk, boc[lvl], td)
            cin = boc[lvl]
            if cfg.attn_levels[lvl]:
                _transformer(s, f"up_blocks.{i}.attentions.{j}", cin, cfg.cross_attention_dim,
                             cfg.transformer_depth[lvl], cfg.use_linear_projection)
        if i < n - 1:
            s[f"up_blocks.{i}.upsamplers.0.conv.weight"] = (cin, cin, 3, 3)
            s[f"up_blocks.{i}.upsamplers.0.conv.bias"] = (cin,)
    s["conv_norm_out.weight"] = (cin,)
    s["conv_norm_out.bias"] = (cin,)
    s["conv_out.weight"] = (cfg.out_channels, cin, 3, 3)
    s["conv_out.bias"] = (cfg.out_channels,)
    return s


def controlnet_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the diffusers ``ControlNetModel`` (reference gyre/pipeline/controlnet/models.py): the UNet's
    conv_in / time_embedding / down_blocks / mid_block, the conditioning embedding of the hint image (8 convolutions), one 1x1 zero
    convolution per skip connection and one for the mid block.  cfg: gyre_amd.config.ControlNetConfig."""
    s: Shapes = OrderedDict()
    boc = cfg.block_out_channels
    td = cfg.time_embed_dim
    s["time_embedding.linear_1.weight"] = (td, boc[0])
    s["time_embedding.linear_1.bias"] = (td,)
    s["time_embedding.linear_2.weight"] = (td, td)
    s["time_embedding.linear_2.bias"] = (td,)
    s["conv_in.weight"] = (boc[0], cfg.in_channels, 3, 3)
    s["conv_in.bias"] = (boc[0],)

    def conv(p, o, i, k):
        s[p + ".weight"] = (o, i, k, k)
        s[p + ".bias"] = (o,)

    ce = tuple(cfg.conditioning_embedding_out_channels)
    conv("controlnet_cond_embedding.conv_in", ce[0], cfg.conditioning_channels, 3)
    for i in range(len(ce) - 1):
        conv(f"controlnet_cond_embedding.blocks.{2 * i}", ce[i], ce[i], 3)
        conv(f"controlnet_cond_embedding.blocks.{2 * i + 1}", ce[i + 1], ce[i], 3)
    conv("controlnet_cond_embedding.conv_out", boc[0], ce[-1], 3)
    n = len(boc)
    skip_ch = [boc[0]]
    cin = boc[0]
    for i in range(n):
        for j in range(cfg.layers_per_block):
            _resnet(s, f"down_blocks.{i}.resnets.{j}", cin, boc[i], td)
            cin = boc[i]
            if cfg.attn_levels[i]:
                _transformer(s, f"down_blocks.{i}.attentions.{j}", cin, cfg.cross_attention_dim,
                             cfg.transformer_depth[i], cfg.use_linear_projection)
            skip_ch.append(cin)
        if i < n - 1:
            conv(f"down_blocks.{i}.downsamplers.0.conv", cin, cin, 3)
            skip_ch.append(cin)
    _resnet(s, "mid_block.resnets.0", cin, cin, td)
    _transformer(s, "mid_block.attentions.0", cin, cfg.cross_attention_dim, cfg.transformer_depth[-1], cfg.use_linear_projection)
    _resnet(s, "mid_block.resnets.1", cin, cin, td)
    for k, c in enumerate(skip_ch):
        conv(f"controlnet_down_blocks.{k}", c, c, 1)
    conv("controlnet_mid_block", cin, cin, 1)
    return s


def _vae_attn(s, p, c):
    # diffusers 0.16 AttentionBlock names (reference pins diffusers ~= 0.16.0)
    s[p + ".group_norm.weight"] = (c,)
    s[p + ".group_norm.bias"] = (c,)
    for n in ("query", "key", "value", "proj_attn"):
        s[f"{p}.{n}.weight"] = (c, c)
        s[f"{p}.{n}.bias"] = (c,)


def vae_param_shapes(cfg: VAEConfig, encoder: bool = True, decoder: bool = True) -> Shapes:
    s: Shapes = OrderedDict()
    boc = cfg.block_out_channels
    z = cfg.latent_channels
    if encoder:
        s["encoder.conv_in.weight"] = (boc[0], cfg.in_channels, 3, 3)
        s["encoder.conv_in.bias"] = (boc[0],)
        cin = boc[0]
        for i, c in enumerate(boc):
            for j in range(cfg.layers_per_block):
                _resnet(s, f"encoder.down_blocks.{i}.resnets.{j}", cin, c, 0)
                cin = c
            if i < len(boc) - 1:
                s[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = (c, c, 3, 3)
                s[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = (c,)
        _resnet(s, "encoder.mid_block.resnets.0", cin, cin, 0)
        _vae_attn(s, "encoder.mid_block.attentions.0", cin)
        _resnet(s, "encoder.mid_block.resnets.1", cin, cin, 0)
        s["encoder.conv_norm_out.weight"] = (cin,)
        s["encoder.conv_norm_out.bias"] = (cin,)
        s["encoder.conv_out.weight"] = (2 * z, cin, 3, 3)
        s["encoder.conv_out.bias"] = (2 * z,)
        s["quant_conv.weight"] = (2 * z, 2 * z, 1, 1)
        s["quant_conv.bias"] = (2 * z,)
    if decoder:
        rb = list(reversed(boc))
        s["post_quant_conv.weight"] = (z, z, 1, 1)
        s["post_quant_conv.bias"] = (z,)
        s["decoder.conv_in.weight"] = (rb[0], z, 3, 3)
        s["decoder.conv_in.bias"] = (rb[0],)
        cin = rb[0]
        _resnet(s, "decoder.mid_block.resnets.0", cin, cin, 0)
        _vae_attn(s, "decoder.mid_block.attentions.0", cin)
        _resnet(s, "decoder.mid_block.resnets.1", cin, cin, 0)
        for i, c in enumerate(rb):
            for j in range(cfg.layers_per_block + 1):
                _resnet(s, f"decoder.up_blocks.{i}.resnets.{j}", cin, c, 0)
                cin = c
            if i < len(rb) - 1:
                s[f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"] = (c, c, 3, 3)
                s[f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"] = (c,)
        s["decoder.conv_norm_out.weight"] = (cin,)
        s["decoder.conv_norm_out.bias"] = (cin,)
        s["decoder.conv_out.weight"] = (cfg.out_channels, cin, 3, 3)
        s["decoder.conv_out.bias"] = (cfg.out_channels,)
    return s


# branch-closing layers get a smaller gain so the residual stream stays O(1)
_BRANCH_OUT = (".conv2.weight", ".to_out.0.weight", ".ff.net.2.weight", ".proj_out.weight", ".proj_attn.weight")


def synthetic_tensor(key: str, shape: Tuple[int, ...], seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed((seed * 1000003) ^ zlib.crc32(key.encode()))
    is_norm = ".norm" in key or "group_norm" in key or key.startswith("conv_norm_out") or "conv_norm_out" in key
    if key.endswith(".bias"):
        std = 0.1 if is_norm else 0.05
        return torch.randn(shape, generator=g) * std
    if is_norm:
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    fan_in = 1
    for d in shape[1:]:
        fan_in *= d
    gain = 0.5 if key.endswith(_BRANCH_OUT) else 1.0
    return torch.randn(shape, generator=g) * (gain / fan_in ** 0.5)


def synthetic_state_dict(shapes: Shapes, seed: int = 0) -> Dict[str, torch.Tensor]:
    return OrderedDict((k, synthetic_tensor(k, shp, seed)) for k, shp in shapes.items())


def t2i_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's T2I adapters (gyre/pipeline/t2i_adapter/adapter.py ``Adapter`` for
    ``type == "main"``, ``Adapter_light`` for ``"light"``); cfg: a mapping as gyre_amd.config.tiny_t2i returns."""
    s: Shapes = OrderedDict()
    ch, nums_rb, cin = tuple(cfg["channels"]), cfg["nums_rb"], cfg["cin"]

    def conv(p, o, i, k):
        s[p + ".weight"] = (o, i, k, k)
        s[p + ".bias"] = (o,)

    if cfg.get("type", "main") == "light":
        for i, c in enumerate(ch):
            inter = c // 4
            conv(f"body.{i}.in_conv", inter, ch[i - 1] if i else cin, 1)
            for j in range(nums_rb):
                conv(f"body.{i}.body.{j}.block1", inter, inter, 3)
                conv(f"body.{i}.body.{j}.block2", inter, inter, 3)
            conv(f"body.{i}.out_conv", c, inter, 1)
        return s
    k, sk, use_conv = cfg["ksize"], cfg["sk"], cfg["use_conv"]
    for i, c in enumerate(ch):
        for j in range(nums_rb):
            p = f"body.{i * nums_rb + j}"
            down = i != 0 and j == 0
            in_c = ch[i - 1] if down else c
            if in_c != c or not sk:
                conv(p + ".in_conv", c, in_c, k)
            conv(p + ".block1", c, c, 3)
            conv(p + ".block2", c, c, k)
            if not sk:
                conv(p + ".skep", c, in_c, k)
            if down and use_conv:
                conv(p + ".down_opt.op", in_c, in_c, 3)
    conv("conv_in", ch[0], cin, 3)
    return s


def _residual_attention_shapes(s: Shapes, width: int, n_layes: int) -> None:
    """adapter.py:150-170 ResidualAttentionBlock in the order torch registers its parameters"""
    for i in range(n_layes):
        p = f"transformer_layes.{i}"
        s[p + ".attn.in_proj_weight"] = (3 * width, width)
        s[p + ".attn.in_proj_bias"] = (3 * width,)
        s[p + ".attn.out_proj.weight"] = (width, width)
        s[p + ".attn.out_proj.bias"] = (width,)
        s[p + ".ln_1.weight"] = (width,)
        s[p + ".ln_1.bias"] = (width,)
        s[p + ".mlp.c_fc.weight"] = (4 * width, width)
        s[p + ".mlp.c_fc.bias"] = (4 * width,)
        s[p + ".mlp.c_proj.weight"] = (width, 4 * width)
        s[p + ".mlp.c_proj.bias"] = (width,)
        s[p + ".ln_2.weight"] = (width,)
        s[p + ".ln_2.bias"] = (width,)


def t2i_style_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's ``StyleAdapter`` (adapter.py:173-185); cfg: gyre_amd.config.t2i_style_config."""
    s: Shapes = OrderedDict()
    w = cfg["width"]
    s["style_embedding"] = (1, cfg["num_token"], w)
    s["proj"] = (w, cfg["context_dim"])
    _residual_attention_shapes(s, w, cfg["n_layes"])
    for n in ("ln_post", "ln_pre"):
        s[n + ".weight"] = (w,)
        s[n + ".bias"] = (w,)
    return s


def t2i_fuser_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's ``CoAdapterFuser`` (adapter.py:266-285); cfg: gyre_amd.config.t2i_fuser_config."""
    s: Shapes = OrderedDict()
    w, ch = cfg["width"], tuple(cfg["unet_channels"])
    s["task_embedding"] = (16, w)
    s["positional_embedding"] = (len(ch), w)
    s["seq_proj"] = (w, w)
    for i, c in enumerate(ch):
        s[f"spatial_feat_mapping.{i}.1.weight"] = (w, c)
        s[f"spatial_feat_mapping.{i}.1.bias"] = (w,)
    _residual_attention_shapes(s, w, cfg["n_layes"])
    for n in ("ln_post", "ln_pre"):
        s[n + ".weight"] = (w,)
        s[n + ".bias"] = (w,)
    for i, c in enumerate(ch):
        s[f"spatial_ch_projs.{i}.weight"] = (c, w)
        s[f"spatial_ch_projs.{i}.bias"] = (c,)
    return s


def rrdb_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of BasicSR's ``RRDBNet`` (and of the reference's ``RRDBNet_Plus`` when cfg["plus"]: one bias-free
    ``conv1x1`` per dense block); cfg: a mapping as gyre_amd.config.tiny_rrdb returns."""
    s: Shapes = OrderedDict()
    nf, gc, scale = cfg["num_feat"], cfg["num_grow_ch"], cfg["scale"]
    cin = cfg["num_in_ch"] * (4 if scale == 2 else 16 if scale == 1 else 1)

    def conv(p, o, i):
        s[p + ".weight"] = (o, i, 3, 3)
        s[p + ".bias"] = (o,)

    conv("conv_first", nf, cin)
    for i in range(cfg["num_block"]):
        for j in (1, 2, 3):
            p = f"body.{i}.rdb{j}"
            for k in range(5):
                conv(f"{p}.conv{k + 1}", nf if k == 4 else gc, nf + k * gc)
            if cfg.get("plus", False):
                s[p + ".conv1x1.weight"] = (gc, nf, 1, 1)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, nf, nf)
    conv("conv_last", cfg["num_out_ch"], nf)
    return s


def lineart_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's ``DrawingGenerator`` (gyre/pipeline/hinters/models/informative_drawings.py) in
    state_dict() order; the ``model3`` weights have ConvTranspose2d's [Cin, Cout, 3, 3] layout, the affine-free instance
    normalisations have no entries.  cfg: a mapping as gyre_amd.config.lineart_config returns."""
    s: Shapes = OrderedDict()

    def conv(p, o, i, k, transposed=False):
        s[p + ".weight"] = (i, o, k, k) if transposed else (o, i, k, k)
        s[p + ".bias"] = (o,)

    conv("model0.1", 64, cfg["input_nc"], 7)
    conv("model1.0", 128, 64, 3)
    conv("model1.3", 256, 128, 3)
    for i in range(cfg["n_residual_blocks"]):
        conv(f"model2.{i}.conv_block.1", 256, 256, 3)
        conv(f"model2.{i}.conv_block.5", 256, 256, 3)
    conv("model3.0", 128, 256, 3, transposed=True)
    conv("model3.3", 64, 128, 3, transposed=True)
    conv("model4.1", cfg["output_nc"], 64, 7)
    return s


def hed_param_shapes(cfg=None) -> Shapes:
    """State-dict keys and shapes of the reference's ``HED`` (gyre/pipeline/hinters/models/hed.py) in state_dict() order: the 13 VGG
    convolutions, the five side scores and ``score_final`` - 38 entries; the bilinear ``weight_deconv*`` buffers are not persistent.
    The network has no configuration (cfg is accepted and ignored, for the shells that pass theirs)."""
    from .config import HED_STAGES
    s: Shapes = OrderedDict()

    def conv(p, o, i, k):
        s[p + ".weight"] = (o, i, k, k)
        s[p + ".bias"] = (o,)

    cin = 3
    for k, (n, width) in enumerate(HED_STAGES):
        for j in range(n):
            conv(f"conv{k + 1}_{j + 1}", width, cin, 3)
            cin = width
    for k, (_, width) in enumerate(HED_STAGES):
        conv(f"score_dsn{k + 1}", 1, width, 1)
    conv("score_final", 1, 5, 1)
    return s


MLSD_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def mlsd_is_buffer(key: str) -> bool:
    return key.endswith(MLSD_BUFFERS)


def mlsd_param_shapes(cfg=None) -> Shapes:
    """State-dict keys and shapes of the reference's ``MobileV2_MLSD_Large`` (gyre/pipeline/hinters/models/mbv2_mlsd_large.py) in
    state_dict() order, 362 entries: the bias-free backbone convolutions, the biased decoder convolutions, and per BatchNorm its weight,
    bias, running_mean, running_var and the scalar num_batches_tracked (accepted by a strict load, never uploaded).  The network has no
    configuration (cfg is accepted and ignored, for the shells that pass theirs)."""
    from .config import MLSD_SETTING
    s: Shapes = OrderedDict()

    def bn(p, c):
        s[p + ".weight"] = (c,)
        s[p + ".bias"] = (c,)
        s[p + ".running_mean"] = (c,)
        s[p + ".running_var"] = (c,)
        s[p + ".num_batches_tracked"] = ()

    def conv_bn(conv, norm, o, i, k, bias):
        s[conv + ".weight"] = (o, i, k, k)
        if bias:
            s[conv + ".bias"] = (o,)
        bn(norm, o)

    conv_bn("backbone.features.0.0", "backbone.features.0.1", 32, 4, 3, False)
    cin, f = 32, 1
    for t, c, n, _ in MLSD_SETTING:
        for _ in range(n):
            p, hid, j = f"backbone.features.{f}.conv", t * cin, 0
            if t != 1:
                conv_bn(f"{p}.0.0", f"{p}.0.1", hid, cin, 1, False)
                j = 1
            conv_bn(f"{p}.{j}.0", f"{p}.{j}.1", hid, 1, 3, False)          # depthwise
            conv_bn(f"{p}.{j + 1}", f"{p}.{j + 2}", c, hid, 1, False)
            cin, f = c, f + 1
    for k, (in_c1, in_c2) in enumerate(((64, 96), (32, 64), (24, 64), (16, 64))):
        a, b = f"block{15 + 2 * k}", f"block{16 + 2 * k}"
        conv_bn(a + ".conv1.0", a + ".conv1.1", 64, in_c2, 1, True)
        conv_bn(a + ".conv2.0", a + ".conv2.1", 64, in_c1, 1, True)
        conv_bn(b + ".conv1.0", b + ".conv1.1", 128, 128, 3, True)
        conv_bn(b + ".conv2.0", b + ".conv2.1", 64, 128, 3, True)
    conv_bn("block23.conv1.0", "block23.conv1.1", 64, 64, 3, True)
    conv_bn("block23.conv2.0", "block23.conv2.1", 64, 64, 3, True)
    s["block23.conv3.weight"] = (16, 64, 1, 1)
    s["block23.conv3.bias"] = (16,)
    return s


class _WindowShapes:
    """The entries the SwinIR and HAT state dicts are made of, appended to ``s`` in call order: cfg gives the width and the MLP ratio."""

    def __init__(self, s: Shapes, cfg):
        self.s, self.C, self.hidden = s, cfg["embed_dim"], int(cfg["embed_dim"] * cfg["mlp_ratio"])

    def conv(self, p, o, i, k=3):
        self.s[p + ".weight"] = (o, i, k, k)
        self.s[p + ".bias"] = (o,)

    def lin(self, p, o, i):
        self.s[p + ".weight"] = (o, i)
        self.s[p + ".bias"] = (o,)

    def norm(self, p):
        self.s[p + ".weight"] = (self.C,)
        self.s[p + ".bias"] = (self.C,)

    def qkv_proj(self, p):
        self.lin(p + ".qkv", 3 * self.C, self.C)
        self.lin(p + ".proj", self.C, self.C)

    def mlp(self, p):
        self.norm(p + ".norm2")
        self.lin(p + ".mlp.fc1", self.hidden, self.C)
        self.lin(p + ".mlp.fc2", self.C, self.hidden)


SWINIR_BUFFERS = ("attn.relative_position_index", "attn_mask")      # state-dict entries that are buffers: loaded, never read


def swinir_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's ``SwinIR`` (gyre/pipeline/upscalers/models/network_swinir.py) with
    upsampler "nearest+conv", in state_dict() order and with its two kinds of buffers (SWINIR_BUFFERS): every attention's
    ``relative_position_index`` and the ``attn_mask`` of the shifted (odd) blocks, built for cfg["img_size"]; cfg: a mapping as
    gyre_amd.config.tiny_swinir returns."""
    s: Shapes = OrderedDict()
    b = _WindowShapes(s, cfg)
    C, heads, upscale = cfg["embed_dim"], cfg["num_heads"], cfg["upscale"]
    size = cfg["img_size"]
    size = (size, size) if isinstance(size, int) else tuple(size)
    three = cfg["resi_connection"] == "3conv"

    def resi(p):
        if not three:
            return b.conv(p, C, C)
        b.conv(p + ".0", C // 4, C)
        b.conv(p + ".2", C // 4, C // 4, 1)
        b.conv(p + ".4", C, C // 4)

    b.conv("conv_first", C, cfg["in_chans"])
    b.norm("patch_embed.norm")
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}"
            if j % 2:
                s[p + ".attn_mask"] = (size[0] // 8 * (size[1] // 8), 64, 64)
            b.norm(p + ".norm1")
            s[p + ".attn.relative_position_bias_table"] = (225, heads[i])
            s[p + ".attn.relative_position_index"] = (64, 64)
            b.qkv_proj(p + ".attn")
            b.mlp(p)
        resi(f"layers.{i}.conv")
    b.norm("norm")
    resi("conv_after_body")
    b.conv("conv_before_upsample.0", 64, C)
    b.conv("conv_up1", 64, 64)
    if upscale == 4:
        b.conv("conv_up2", 64, 64)
    b.conv("conv_hr", 64, 64)
    b.conv("conv_last", cfg["in_chans"], 64)
    return s


def swinir_is_buffer(key: str) -> bool:
    return key.endswith(SWINIR_BUFFERS)


HAT_BUFFERS = ("relative_position_index_SA", "relative_position_index_OCA")      # state-dict entries that are buffers: loaded, never read


def hat_param_shapes(cfg) -> Shapes:
    """State-dict keys and shapes of the reference's ``HAT`` (gyre/pipeline/upscalers/models/hat_arch.py) with upsampler
    "pixelshuffle" and "1conv", in state_dict() order, its two global index buffers (HAT_BUFFERS) first; cfg: a mapping as
    gyre_amd.config.tiny_hat returns."""
    s: Shapes = OrderedDict()
    b = _WindowShapes(s, cfg)
    C, heads, upscale = cfg["embed_dim"], cfg["num_heads"], cfg["upscale"]
    mid, sq = C // cfg["compress_ratio"], C // cfg["squeeze_factor"]
    s["relative_position_index_SA"] = (256, 256)
    s["relative_position_index_OCA"] = (256, 576)
    b.conv("conv_first", C, cfg["in_chans"])
    b.norm("patch_embed.norm")
    for i, depth in enumerate(cfg["depths"]):
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}"
            b.norm(p + ".norm1")
            s[p + ".attn.relative_position_bias_table"] = (961, heads[i])
            b.qkv_proj(p + ".attn")
            b.conv(p + ".conv_block.cab.0", mid, C)
            b.conv(p + ".conv_block.cab.2", C, mid)
            b.conv(p + ".conv_block.cab.3.attention.1", sq, C, 1)
            b.conv(p + ".conv_block.cab.3.attention.3", C, sq, 1)
            b.mlp(p)
        p = f"layers.{i}.residual_group.overlap_attn"
        s[p + ".relative_position_bias_table"] = (1521, heads[i])
        b.norm(p + ".norm1")
        b.qkv_proj(p)
        b.mlp(p)
        b.conv(f"layers.{i}.conv", C, C)
    b.norm("norm")
    b.conv("conv_after_body", C, C)
    b.conv("conv_before_upsample.0", 64, C)
    b.conv("upsample.0", 256, 64)
    if upscale == 4:
        b.conv("upsample.2", 256, 64)
    b.conv("conv_last", cfg["in_chans"], 64)
    return s


def hat_is_buffer(key: str) -> bool:
    return key in HAT_BUFFERS
