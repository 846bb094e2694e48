"""Reference side of the VAE graph tests (tests/test_vae_graph_ref_host.py on the CPU, tests/test_gpu_vae_graph_nodes.py on the GPU):
the configs without the one-channel-per-group blind spot, the storage emulation of encode, decode and the decode VJP, the catalogue of
seeded wiring mistakes, the verdict and the table of emulation floors.  The UNet's counterpart is tests/graph_ref.py; its Ctl
(roundings and the one seeded mistake of an evaluation), rel_l2, worst_ratio and batch-pair swap are used from there.

OBSERVABLES.  Encode: the moments and the output of every encoder node.  Decode: the image, d_z (the gradient of sum(image * cot)),
the output of every decoder node and the complete gradient of every decoder node's output.  Nodes carry their state-dict prefix - the
names of oracle.models_ref.vae_encode_moments / vae_decode (taps=) and of gyre_vae_debug_tap / gyre_vae_debug_grad_tap.

`oracle_*()` is the fp32 reference (oracle/models_ref.py itself, node tensors taken with retain_grad()).  `emulate_*()` is this file's
own restatement of the same graph (pinned to the oracle bit for bit by the host test) with the weight matrices rounded to the storage
type and a rounding wherever the native encode / decode / decode VJP stores a tensor (gyre_vae::run_encode, run_decode, Exec::resnet,
gyre_vae::vattn -> Exec::mha, gyre_vae_run_decode_vjp): the input on entry; every conv, shortcut and residual sum; the output of every
GroupNorm (a launch of its own everywhere in the VAE); q, k, v, the attention output and proj_attn + residual.  The image, the moments
and d_z leave in fp32.  A rounding's backward rounds the gradient, which is where the sweep stores one; the cotangent is rounded on
entry.  `fused=True` rounds less often: no store after a GroupNorm and none of a shortcut conv's output (Exec::resnet folds the 1x1
shortcut into conv2 where the tile allows it).  FLOORS holds the plain emulation's distances from the oracle; the gate of every
observable is TWICE its floor (the rule of tests/graph_ref.py).  Gates never come from a native output."""
from __future__ import annotations

import contextlib
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from graph_ref import DT_NAME, DTYPES, Ctl, _other, rel_l2, worst_ratio       # noqa: F401  (re-exported for the two test files)
from gyre_amd import config as gcfg
from gyre_amd import weights
from oracle import models_ref as M

CONFIGS = {"vae_graph": gcfg.VAEConfig(block_out_channels=(64, 128, 128), sample_size=32),
           # the mid attention at D = 512 (SD1.5's row of the attention table), forward and sweep; nothing else is asked of it
           "vae_wide": gcfg.VAEConfig(block_out_channels=(64, 128, 512), layers_per_block=1, sample_size=32),
           "tiny": gcfg.tiny_vae()}
SIZES = ((8, 12), (5, 7))            # latent sizes; 5x7: 35 tokens in the mid attention (no multiple of 8), odd at every level but the last
PATHS = ("encode", "decode")
WRONG_HEADS = 8


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def state_dict(cfg):
    return weights.synthetic_state_dict(weights.vae_param_shapes(cfg), 0)


def scale(cfg):
    return 2 ** (len(cfg.block_out_channels) - 1)


def inputs(cfg, h, w, B=2):
    """(z, image, cot): latents [B, 4, h, w], an image in -1..1 and an image cotangent of f times the size"""
    f = scale(cfg)
    return (_randn(B, cfg.latent_channels, h, w, seed=5), _randn(B, cfg.in_channels, f * h, f * w, seed=6).clamp(-1, 1),
            _randn(B, cfg.out_channels, f * h, f * w, seed=7))


# ---- topology ----------------------------------------------------------------------------------------------------------------------------
def node_names(cfg, path):
    """Node names of a path in the order the forward produces them (the sweep meets the decoder's back to front)."""
    n, mid = len(cfg.block_out_channels), ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
    if path == "encode":
        out = ["encoder.conv_in"]
        for i in range(n):
            out += [f"encoder.down_blocks.{i}.resnets.{j}" for j in range(cfg.layers_per_block)]
            if i < n - 1:
                out.append(f"encoder.down_blocks.{i}.downsamplers.0")
        return out + ["encoder." + m for m in mid] + ["encoder.conv_out"]
    out = ["post_quant_conv", "decoder.conv_in"] + ["decoder." + m for m in mid]
    for i in range(n):
        out += [f"decoder.up_blocks.{i}.resnets.{j}" for j in range(cfg.layers_per_block + 1)]
        if i < n - 1:
            out.append(f"decoder.up_blocks.{i}.upsamplers.0")
    return out


def path_of(site):
    return "encode" if site.startswith("encoder") or site == "quant_conv" else "decode"


def sites(cfg, sd):
    """site lists by kind of place"""
    names = node_names(cfg, "encode") + node_names(cfg, "decode")
    res = [k for k in names if ".resnets." in k]
    dec = lambda ks: [k for k in ks if k.startswith("decoder.")]
    short = [k for k in res if (k + ".conv_shortcut.weight") in sd]
    ident = [k for k in res if k not in short]
    attn = [k for k in names if ".attentions." in k]
    return {"resnet": res, "shortcut": short, "sampler": [k for k in names if "samplers.0" in k], "attn": attn,
            "down_sampler": [k for k in names if "downsamplers.0" in k], "up_sampler": [k for k in names if "upsamplers.0" in k],
            "quant_conv": ["quant_conv"], "post_quant_conv": ["post_quant_conv"], "conv_in": ["encoder.conv_in", "decoder.conv_in"],
            "conv_out": ["encoder.conv_out", "decoder.conv_out"], "conv_norm_out": ["encoder.conv_norm_out", "decoder.conv_norm_out"],
            "half": ["encoder", "decoder"], "dec_identity": dec(ident), "dec_shortcut": dec(short), "dec_attn": dec(attn)}


# ---- the graph, restated with hooks ------------------------------------------------------------------------------------------------------
def _resnet(x, sd, p, g, eps, c):
    h = c.rd_norm(F.silu(M._gn(x, sd, p + ".norm1", g, eps)))
    h = c.rd(M._conv(h, sd, p + ".conv1"))
    h = c.rd_norm(F.silu(M._gn(h, sd, p + ".norm2", g, eps)))
    h = M._conv(h, sd, p + ".conv2")
    if (p + ".conv_shortcut.weight") in sd:
        x = M._conv(x.detach() if c.hit("shortcut-conv gradient dropped", p) else x, sd, p + ".conv_shortcut", padding=0)
        x = x if c.fused else c.rd(x)                    # fused: the shortcut's K steps run inside conv2's launch, nothing is stored
    elif c.hit("identity-shortcut gradient dropped", p):
        x = x.detach()
    return c.rd(x + h)


def _attn(x, sd, p, g, eps, c):
    B, C, H, W = x.shape
    src = _other(x) if c.hit("the other sample's tensor fed to the attention", p) else x
    h = c.rd_norm(M._gn(src, sd, p + ".group_norm", g, eps))
    h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
    q, k, v = (c.rd(M._lin(h, sd, f"{p}.{n}")) for n in ("query", "key", "value"))        # (the oracle's order)
    if c.hit("softmax scale for the wrong head count", p):
        q = q * math.sqrt(WRONG_HEADS)                   # (C / heads)^-1/2 in place of C^-1/2
    a = M._lin(c.rd(M.attention(q, k, v, 1)), sd, p + ".proj_attn")
    a = a.reshape(B, H, W, C).permute(0, 3, 1, 2)
    if c.hit("gradient blocked through the attention branch", p):
        a = a.detach()
    if c.hit("attention residual dropped", p):
        return c.rd(a)
    return c.rd((x.detach() if c.hit("attention residual's gradient dropped", p) else x) + a)


def _mid(h, sd, p, g, eps, c, node):
    h = node(p + ".resnets.0", _resnet(h, sd, p + ".resnets.0", g, eps, c))
    h = node(p + ".attentions.0", _attn(h, sd, p + ".attentions.0", g, eps, c))
    return node(p + ".resnets.1", _resnet(h, sd, p + ".resnets.1", g, eps, c))


def _noder(nodes):
    def node(name, y):
        nodes[name] = y
        return y
    return node


def encode(sd, cfg, image, c):
    """(moments, {node name: tensor of the graph}) - oracle.models_ref.vae_encode_moments restated over the same leaf functions, with
    Ctl's roundings and seeded mistakes.  With Ctl() it is the oracle bit for bit."""
    g, n = cfg.norm_num_groups, len(cfg.block_out_channels)
    eps = 1e-5 if c.hit("every norm's eps 1e-5 for 1e-6", "encoder") else 1e-6
    nodes = OrderedDict()
    node = _noder(nodes)
    h = node("encoder.conv_in", c.rd(M._conv(c.rd_value(image), sd, "encoder.conv_in")))
    for i in range(n):
        for j in range(cfg.layers_per_block):
            p = f"encoder.down_blocks.{i}.resnets.{j}"
            h = node(p, _resnet(h, sd, p, g, eps, c))
        if i < n - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0"
            if c.hit("explicit pad made circular under tiling", p):
                h = F.pad(h, (0, 1, 0, 1), mode="circular")
            else:
                h = F.pad(h, (1, 0, 1, 0) if c.hit("downsampler's pad on the wrong side", p) else (0, 1, 0, 1))
            h = node(p, c.rd(M._conv(h, sd, p + ".conv", stride=2, padding=0)))
    h = _mid(h, sd, "encoder.mid_block", g, eps, c, node)
    h = M._gn(h, sd, "encoder.conv_norm_out", g, eps)
    h = c.rd_norm(h if c.hit("SiLU after conv_norm_out dropped", "encoder.conv_norm_out") else F.silu(h))
    h = node("encoder.conv_out", c.rd(M._conv(h, sd, "encoder.conv_out")))
    m = M._conv(h, sd, "quant_conv", padding=0)                    # the moments leave in fp32
    if c.hit("mean and logvar halves swapped", "quant_conv"):
        m = torch.cat(m.chunk(2, dim=1)[::-1], dim=1)
    return m, nodes


def _upsample(h, p, c):
    if c.hit("nearest upsampling shifted by one source pixel in x", p):
        h = torch.cat([h[..., 1:], h[..., -1:]], dim=-1)
    if c.hit("nearest upsampling shifted by one source pixel in y", p):
        h = torch.cat([h[..., 1:, :], h[..., -1:, :]], dim=-2)
    u = F.interpolate(h, scale_factor=2.0, mode="nearest")
    if c.hit("upsampler backward with one source contribution lost", p):
        lost = torch.zeros_like(u)
        lost[..., 1::2, 1::2] = 1.0                       # the (1, 1) pixel of every 2x2 cell sends nothing back to its source
        u = u * (1 - lost) + (u * lost).detach()
    return u


def decode(sd, cfg, z, c):
    """(image, {node name: tensor of the graph}) - oracle.models_ref.vae_decode restated likewise."""
    g, n = cfg.norm_num_groups, len(cfg.block_out_channels)
    eps = 1e-5 if c.hit("every norm's eps 1e-5 for 1e-6", "decoder") else 1e-6
    nodes = OrderedDict()
    node = _noder(nodes)
    h = node("post_quant_conv", c.rd(M._conv(c.rd_value(z), sd, "post_quant_conv", padding=0)))
    h = node("decoder.conv_in", c.rd(M._conv(h, sd, "decoder.conv_in")))
    h = _mid(h, sd, "decoder.mid_block", g, eps, c, node)
    for i in range(n):
        for j in range(cfg.layers_per_block + 1):
            p = f"decoder.up_blocks.{i}.resnets.{j}"
            h = node(p, _resnet(h, sd, p, g, eps, c))
        if i < n - 1:
            p = f"decoder.up_blocks.{i}.upsamplers.0"
            h = node(p, c.rd(M._conv(_upsample(h, p, c), sd, p + ".conv")))
    h = M._gn(h, sd, "decoder.conv_norm_out", g, eps)
    h = c.rd_norm(h if c.hit("SiLU after conv_norm_out dropped", "decoder.conv_norm_out") else F.silu(h))
    return c.rd_grad(M._conv(h, sd, "decoder.conv_out")), nodes          # the image leaves in fp32; the cotangent is rounded on entry


def _tiling(mode):
    return M.tiling(mode) if mode else contextlib.nullcontext()


def _finish_encode(m, nodes):
    return {"moments": m.detach(), "out": {k: v.detach() for k, v in nodes.items()}}


def _finish_decode(img, zr, nodes, cot):
    if cot is None:                                          # forward only (tiling: the sweep has no circular convolutions)
        return {"image": img.detach(), "out": {k: v.detach() for k, v in nodes.items()}}
    for v in nodes.values():
        v.retain_grad()
    (img * cot).sum().backward()
    return {"image": img.detach(), "d_z": zr.grad, "out": {k: v.detach() for k, v in nodes.items()},
            "grad": {k: v.grad for k, v in nodes.items()}}


def oracle_encode(sd, cfg, image, tiling=None):
    taps = {}
    with torch.no_grad(), _tiling(tiling):
        m = M.vae_encode_moments(sd, cfg, image, taps=taps)
    return _finish_encode(m, OrderedDict((k, taps[k]) for k in node_names(cfg, "encode")))


def oracle_decode(sd, cfg, z, cot, tiling=None):
    """The fp32 reference: oracle/models_ref.py with its node taps, differentiated with the cotangent cot (None: forward only)."""
    zr, taps = z.clone().requires_grad_(cot is not None), {}
    with _tiling(tiling):
        img = M.vae_decode(sd, cfg, zr, taps=taps)
        return _finish_decode(img, zr, OrderedDict((k, taps[k]) for k in node_names(cfg, "decode")), cot)


def _prepare(sd, cfg, dtype, fused, mistake):
    c = Ctl(dtype, fused, mistake)
    if mistake is not None and MISTAKES[mistake[0]][1] is not None:
        sd = MISTAKES[mistake[0]][1](sd, mistake[1], cfg)
    if dtype is not None:
        sd = {k: (c.rd(v) if v.ndim > 1 else v) for k, v in sd.items()}          # matrices are stored in dtype, biases / norm vectors in fp32
    return sd, c


def emulate_encode(sd, cfg, image, dtype, fused=False, mistake=None, tiling=None):
    """The encoder with the weights and every stored tensor rounded to dtype (None: fp32, nothing rounded); fused / mistake: see the
    module docstring and MISTAKES."""
    sd, c = _prepare(sd, cfg, dtype, fused, mistake)
    with torch.no_grad(), _tiling(tiling):
        return _finish_encode(*encode(sd, cfg, image, c))


def emulate_decode(sd, cfg, z, cot, dtype, fused=False, mistake=None, tiling=None):
    sd, c = _prepare(sd, cfg, dtype, fused, mistake)
    zr = z.clone().requires_grad_(cot is not None)
    with _tiling(tiling):
        img, nodes = decode(sd, cfg, zr, c)
        return _finish_decode(img, zr, nodes, cot)


# ---- mistakes ------------------------------------------------------------------------------------------------------------------------------
def _zero(*suffixes):
    def edit(sd, site, cfg):
        sd = dict(sd)
        for s in suffixes:
            sd[site + s] = torch.zeros_like(sd[site + s])
        return sd
    return edit


# kind -> (site list key of sites(), state-dict edit or None when the mistake is a hook of encode() / decode())
MISTAKES = OrderedDict([
    # forward, as state-dict edits
    ("conv1 bias dropped", ("resnet", _zero(".conv1.bias"))),
    ("conv2 bias dropped", ("resnet", _zero(".conv2.bias"))),
    ("resnet norm2 beta dropped", ("resnet", _zero(".norm2.bias"))),
    ("shortcut bias dropped", ("shortcut", _zero(".conv_shortcut.bias"))),
    ("sampler conv bias dropped", ("sampler", _zero(".conv.bias"))),
    ("attention group_norm beta dropped", ("attn", _zero(".group_norm.bias"))),
    ("attention query bias dropped", ("attn", _zero(".query.bias"))),
    ("attention value bias dropped", ("attn", _zero(".value.bias"))),
    ("attention proj_attn bias dropped", ("attn", _zero(".proj_attn.bias"))),
    ("quant_conv bias dropped", ("quant_conv", _zero(".bias"))),
    ("post_quant_conv bias dropped", ("post_quant_conv", _zero(".bias"))),
    ("conv_in bias dropped", ("conv_in", _zero(".bias"))),
    ("conv_out bias dropped", ("conv_out", _zero(".bias"))),
    ("conv_norm_out beta dropped", ("conv_norm_out", _zero(".bias"))),
    # forward, as hooks
    ("attention residual dropped", ("attn", None)),
    ("softmax scale for the wrong head count", ("attn", None)),
    ("SiLU after conv_norm_out dropped", ("conv_norm_out", None)),
    ("downsampler's pad on the wrong side", ("down_sampler", None)),
    ("nearest upsampling shifted by one source pixel in x", ("up_sampler", None)),
    ("nearest upsampling shifted by one source pixel in y", ("up_sampler", None)),
    ("mean and logvar halves swapped", ("quant_conv", None)),
    ("the other sample's tensor fed to the attention", ("attn", None)),
    ("every norm's eps 1e-5 for 1e-6", ("half", None)),
    ("explicit pad made circular under tiling", ("down_sampler", None)),
    # gradient only, as detached branches (decoder: the only sweep)
    ("identity-shortcut gradient dropped", ("dec_identity", None)),
    ("shortcut-conv gradient dropped", ("dec_shortcut", None)),
    ("gradient blocked through the attention branch", ("dec_attn", None)),
    ("attention residual's gradient dropped", ("dec_attn", None)),
    ("upsampler backward with one source contribution lost", ("up_sampler", None)),
])
TILING_KINDS = ("explicit pad made circular under tiling",)          # evaluated under tiling "xy" on both sides
# kinds of which no pair may be listed in BLIND
NEVER_BLIND = [k for k in MISTAKES if any(w in k for w in ("bias", "beta", "residual", "pad", "upsampl", "shortcut"))]

# (kind, site) pairs the fp16 criteria cannot see, each with its reason.
BLIND = {("every norm's eps 1e-5 for 1e-6", s): "group variance of order 1: eps 1e-5 against 1e-6 changes rstd by 5e-6, far below one fp16 rounding"
         for s in ("encoder", "decoder")}

# A mistake that is blind by construction and therefore not in the catalogue: the attention's KEY bias.  q . (k_j + b) = q . k_j + q . b
# adds the same number to every logit of a query's row, and the softmax removes a per-row constant exactly; only the rounding of
# that subtraction is left (tests/test_vae_graph_ref_host.py::test_key_bias_is_invisible_by_construction).  A native path may
# therefore skip it; this one applies it (gyre_vae::reg_vattn keeps query.bias | key.bias in the fused projection's bias vector).
KEY_BIAS = "attention key bias dropped"


def catalogue(cfg, sd):
    """every (kind, site) pair of the config"""
    s = sites(cfg, sd)
    return [(kind, site) for kind, (where, _) in MISTAKES.items() for site in s[where]]


# ---- verdict -------------------------------------------------------------------------------------------------------------------------------
def distances(got, ref):
    """rel-L2 of every observable, in the layout of the results: a number per outer tensor, {node: number} per group of nodes"""
    return {k: ({n: rel_l2(got[k][n], t) for n, t in v.items()} if isinstance(v, dict) else rel_l2(got[k], v)) for k, v in ref.items()}


def verdict(got, ref, floors):
    """Per observable rel-L2(got, ref) / (2 x floor); passes iff every ratio is <= 1.  floors: a FLOORS row as floors_for() gives it (or
    a fresh `distances`).  Returns (passed, ratios in the layout of `distances`, {group: (worst ratio, name)})."""
    d = distances(got, ref)
    ratios, worst = {}, {}
    for k, v in d.items():
        if isinstance(v, dict):
            ratios[k] = {n: x / (2 * floors[k][n]) for n, x in v.items()}
            n = max(ratios[k], key=lambda m: ratios[k][m] if not math.isnan(ratios[k][m]) else float("inf"))
            worst[k] = (ratios[k][n], n)
        else:
            ratios[k] = v / (2 * floors[k])
            worst[k] = (ratios[k], k)
    return all(w[0] <= 1.0 for w in worst.values()), ratios, worst           # NaN compares false: a NaN observable fails


def outer_ratio(ratios):
    """the worst ratio when only the outer tensors (moments; image and d_z) are judged"""
    vals = [v for v in ratios.values() if not isinstance(v, dict)]
    return float("inf") if any(math.isnan(v) for v in vals) else max(vals)


# ---- cases and floors ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case(name, size, path, tiling=None):
    """(cfg, state dict, inputs (z, image, cot), fp32 oracle result) - computed once per key and shared, never changed"""
    key = (name, tuple(size), path, tiling)
    if key not in _CASES:
        cfg = CONFIGS[name]
        sd = state_dict(cfg)
        z, img, cot = inputs(cfg, *size)
        ref = oracle_encode(sd, cfg, img, tiling) if path == "encode" else oracle_decode(sd, cfg, z, None if tiling else cot, tiling)
        _CASES[key] = (cfg, sd, (z, img, cot), ref)
    return _CASES[key]


def emulate(name, size, path, dtype, tiling=None, **kw):
    cfg, sd, (z, img, cot), _ = case(name, size, path, tiling)
    if path == "encode":
        return emulate_encode(sd, cfg, img, dtype, tiling=tiling, **kw)
    return emulate_decode(sd, cfg, z, None if tiling else cot, dtype, tiling=tiling, **kw)


def floor_key(name, size, path, dtype, tiling=None):
    return (name, tuple(size), path, tiling or "plain", DT_NAME[dtype])


def compact(d, cfg, path):
    """a `distances` dict as the literal stored below: node values as lists in node_names order"""
    names = node_names(cfg, path)
    return {k: ([v[n] for n in names] if isinstance(v, dict) else v) for k, v in d.items()}


def floors_for(name, size, path, dtype, tiling=None):
    """the stored FLOORS row as a `distances`-shaped dict"""
    names = node_names(CONFIGS[name], path)
    return {k: (dict(zip(names, v)) if isinstance(v, list) else v) for k, v in FLOORS[floor_key(name, size, path, dtype, tiling)].items()}


def floor_keys():
    """every key the table must hold: vae_graph at both sizes and vae_wide at 8x12, both paths, both storage types; tiling xy at 8x12"""
    out = []
    for dt in DTYPES:
        for path in PATHS:
            out += [floor_key("vae_graph", s, path, dt) for s in SIZES]
            out += [floor_key("vae_wide", SIZES[0], path, dt), floor_key("vae_graph", SIZES[0], path, dt, "xy")]
    return out


# Emulation distances: plain emulate() against the fp32 oracle, rel-L2 per observable; node lists in node_names() order.
# Re-measured and compared (10 %) by tests/test_vae_graph_ref_host.py::test_floor_table_is_current, whose printed `FLOORS[...] = ...`
# lines are the way to update this table.
# ---- FLOORS begin (the lines tests/test_vae_graph_ref_host.py::test_floor_table_is_current prints) ----
FLOORS = {}
FLOORS[('vae_graph', (8, 12), 'encode', 'plain', 'bf16')] = {'moments': 9.474e-03,
    'out': [2.530e-03, 3.449e-03, 4.137e-03, 4.737e-03, 5.711e-03, 6.130e-03, 6.529e-03, 6.879e-03, 7.191e-03, 7.551e-03, 7.728e-03, 7.989e-03, 9.725e-03]}
FLOORS[('vae_graph', (5, 7), 'encode', 'plain', 'bf16')] = {'moments': 9.467e-03,
    'out': [2.535e-03, 3.448e-03, 4.150e-03, 4.743e-03, 5.682e-03, 6.094e-03, 6.498e-03, 6.855e-03, 7.199e-03, 7.494e-03, 7.820e-03, 8.147e-03, 9.287e-03]}
FLOORS[('vae_wide', (8, 12), 'encode', 'plain', 'bf16')] = {'moments': 8.086e-03,
    'out': [2.530e-03, 3.449e-03, 4.174e-03, 5.239e-03, 5.716e-03, 6.531e-03, 6.931e-03, 7.149e-03, 7.457e-03, 8.605e-03]}
FLOORS[('vae_graph', (8, 12), 'encode', 'xy', 'bf16')] = {'moments': 9.799e-03,
    'out': [2.529e-03, 3.433e-03, 4.112e-03, 4.732e-03, 5.745e-03, 6.159e-03, 6.527e-03, 6.864e-03, 7.194e-03, 7.533e-03, 7.686e-03, 7.896e-03, 1.016e-02]}
FLOORS[('vae_graph', (8, 12), 'decode', 'plain', 'bf16')] = {'image': 1.119e-02,
    'd_z': 1.251e-02,
    'out': [3.344e-03, 4.139e-03, 4.652e-03, 5.041e-03, 5.412e-03, 5.843e-03, 6.203e-03, 6.516e-03, 6.802e-03, 7.121e-03, 7.395e-03, 7.639e-03, 7.906e-03, 8.390e-03, 8.618e-03, 8.870e-03],
    'grad': [1.218e-02, 1.195e-02, 1.163e-02, 1.132e-02, 1.105e-02, 1.072e-02, 1.039e-02, 1.006e-02, 9.653e-03, 9.270e-03, 8.904e-03, 8.528e-03, 8.164e-03, 7.413e-03, 6.877e-03, 6.282e-03]}
FLOORS[('vae_graph', (5, 7), 'decode', 'plain', 'bf16')] = {'image': 1.147e-02,
    'd_z': 1.536e-02,
    'out': [3.656e-03, 4.398e-03, 4.850e-03, 5.275e-03, 5.671e-03, 6.091e-03, 6.469e-03, 6.739e-03, 7.019e-03, 7.308e-03, 7.646e-03, 7.887e-03, 8.128e-03, 8.583e-03, 8.805e-03, 9.013e-03],
    'grad': [1.457e-02, 1.240e-02, 1.201e-02, 1.152e-02, 1.117e-02, 1.084e-02, 1.043e-02, 9.998e-03, 9.995e-03, 9.592e-03, 9.175e-03, 8.743e-03, 8.375e-03, 7.632e-03, 7.082e-03, 6.448e-03]}
FLOORS[('vae_wide', (8, 12), 'decode', 'plain', 'bf16')] = {'image': 1.038e-02,
    'd_z': 1.220e-02,
    'out': [3.344e-03, 4.130e-03, 4.605e-03, 5.024e-03, 5.441e-03, 5.824e-03, 6.205e-03, 6.664e-03, 7.404e-03, 7.673e-03, 8.024e-03, 8.500e-03, 8.749e-03],
    'grad': [1.245e-02, 1.093e-02, 1.063e-02, 1.031e-02, 9.991e-03, 9.696e-03, 9.364e-03, 9.014e-03, 8.454e-03, 8.009e-03, 7.710e-03, 6.839e-03, 6.198e-03]}
FLOORS[('vae_graph', (8, 12), 'decode', 'xy', 'bf16')] = {'image': 1.087e-02,
    'out': [3.344e-03, 4.118e-03, 4.631e-03, 4.973e-03, 5.353e-03, 5.768e-03, 6.149e-03, 6.479e-03, 6.777e-03, 7.079e-03, 7.387e-03, 7.624e-03, 7.909e-03, 8.368e-03, 8.602e-03, 8.825e-03]}
FLOORS[('vae_graph', (8, 12), 'encode', 'plain', 'fp16')] = {'moments': 1.218e-03,
    'out': [3.166e-04, 4.304e-04, 5.163e-04, 5.903e-04, 7.069e-04, 7.575e-04, 8.102e-04, 8.520e-04, 8.948e-04, 9.429e-04, 9.683e-04, 1.002e-03, 1.179e-03]}
FLOORS[('vae_graph', (5, 7), 'encode', 'plain', 'fp16')] = {'moments': 1.263e-03,
    'out': [3.169e-04, 4.342e-04, 5.169e-04, 5.902e-04, 7.112e-04, 7.611e-04, 8.022e-04, 8.533e-04, 9.029e-04, 9.407e-04, 9.747e-04, 1.016e-03, 1.193e-03]}
FLOORS[('vae_wide', (8, 12), 'encode', 'plain', 'fp16')] = {'moments': 1.045e-03,
    'out': [3.166e-04, 4.304e-04, 5.171e-04, 6.498e-04, 7.059e-04, 8.041e-04, 8.544e-04, 8.821e-04, 9.238e-04, 1.077e-03]}
FLOORS[('vae_graph', (8, 12), 'encode', 'xy', 'fp16')] = {'moments': 1.199e-03,
    'out': [3.162e-04, 4.302e-04, 5.140e-04, 5.882e-04, 7.102e-04, 7.598e-04, 8.119e-04, 8.604e-04, 9.077e-04, 9.542e-04, 9.762e-04, 1.008e-03, 1.265e-03]}
FLOORS[('vae_graph', (8, 12), 'decode', 'plain', 'fp16')] = {'image': 1.305e-03,
    'd_z': 1.538e-03,
    'out': [3.715e-04, 4.754e-04, 5.445e-04, 5.923e-04, 6.374e-04, 6.908e-04, 7.387e-04, 7.774e-04, 8.197e-04, 8.586e-04, 8.978e-04, 9.286e-04, 9.680e-04, 1.017e-03, 1.045e-03, 1.076e-03],
    'grad': [1.514e-03, 1.448e-03, 1.414e-03, 1.380e-03, 1.351e-03, 1.313e-03, 1.273e-03, 1.230e-03, 1.182e-03, 1.136e-03, 1.089e-03, 1.043e-03, 1.003e-03, 9.078e-04, 8.419e-04, 7.691e-04]}
FLOORS[('vae_graph', (5, 7), 'decode', 'plain', 'fp16')] = {'image': 1.386e-03,
    'd_z': 1.648e-03,
    'out': [4.037e-04, 4.956e-04, 5.586e-04, 6.112e-04, 6.525e-04, 6.987e-04, 7.509e-04, 7.885e-04, 8.269e-04, 8.671e-04, 9.070e-04, 9.423e-04, 9.855e-04, 1.031e-03, 1.060e-03, 1.088e-03],
    'grad': [1.678e-03, 1.448e-03, 1.405e-03, 1.354e-03, 1.321e-03, 1.308e-03, 1.272e-03, 1.219e-03, 1.229e-03, 1.178e-03, 1.128e-03, 1.077e-03, 1.037e-03, 9.387e-04, 8.655e-04, 7.806e-04]}
FLOORS[('vae_wide', (8, 12), 'decode', 'plain', 'fp16')] = {'image': 1.251e-03,
    'd_z': 1.453e-03,
    'out': [3.715e-04, 4.758e-04, 5.403e-04, 5.915e-04, 6.446e-04, 6.930e-04, 7.386e-04, 7.959e-04, 8.904e-04, 9.262e-04, 9.717e-04, 1.034e-03, 1.064e-03],
    'grad': [1.464e-03, 1.320e-03, 1.285e-03, 1.249e-03, 1.212e-03, 1.175e-03, 1.133e-03, 1.108e-03, 1.036e-03, 9.830e-04, 9.484e-04, 8.409e-04, 7.597e-04]}
FLOORS[('vae_graph', (8, 12), 'decode', 'xy', 'fp16')] = {'image': 1.365e-03,
    'out': [3.715e-04, 4.734e-04, 5.377e-04, 5.835e-04, 6.337e-04, 6.835e-04, 7.286e-04, 7.642e-04, 8.095e-04, 8.490e-04, 8.890e-04, 9.209e-04, 9.653e-04, 1.020e-03, 1.048e-03, 1.080e-03]}
# ---- FLOORS end ----
