"""Reference side of the UNet graph tests (tests/test_graph_ref_host.py on the CPU, tests/test_gpu_graph_nodes.py on the GPU): the
three-level config without the one-channel-per-group blind spot, the storage emulation, the catalogue of seeded wiring mistakes, the
verdict and the table of emulation floors.

OBSERVABLES of one forward + input-gradient evaluation: eps, d_x, the output of every node and the complete gradient of every node's
output.  Nodes carry their state-dict prefix: conv_in, every resnet, every Transformer2D (after proj_out and its residual), every
resampling conv - the names of oracle.models_ref.unet_forward(taps=) and of gyre_unet_debug_tap / gyre_unet_debug_grad_tap.

`oracle()` is the fp32 reference (oracle/models_ref.py itself, node tensors taken with retain_grad()).  `emulate()` is this file's own
restatement of the same graph (pinned to the oracle bit for bit by the host test) with the weights rounded to the storage type and a
rounding wherever the native activation-keeping pass stores a tensor; the rounding's backward rounds the gradient, which is where the
reverse sweep stores one.  FLOORS holds its distances from the fp32 oracle; the gate of every observable is TWICE its floor: the native
graph sums in another order and rounds at most as often, so it should sit at or below the emulation (the rule of
tests/test_gpu_rrdb_model.py).  Gates never come from a native output."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from gyre_amd import config as gcfg
from gyre_amd import weights
from oracle import models_ref as M
from oracle import tome_ref

GRAPH_CFG = gcfg.UNetConfig(block_out_channels=(64, 128, 128), attn_levels=(True, True, False), num_heads=(2, 4, 4),
                            transformer_depth=(1, 2, 1), cross_attention_dim=64, sample_size=16)
GRAPH_LIN_CFG = gcfg.UNetConfig(block_out_channels=(64, 128, 128), attn_levels=(True, True, False), num_heads=(2, 4, 4),
                                transformer_depth=(1, 2, 1), cross_attention_dim=64, sample_size=16, use_linear_projection=True)
CONFIGS = {"graph": GRAPH_CFG, "graph_lin": GRAPH_LIN_CFG, "tiny_sdxl": gcfg.tiny_sdxl_unet(), "tiny": gcfg.tiny_unet()}
SIZES = ((16, 16), (9, 15))
DTYPES = (torch.bfloat16, torch.float16)
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
TOME_R = 40


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def state_dict(cfg):
    return weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 0)


def inputs(cfg, H, W, B=2, S=77):
    """(x, t, ctx, cot, added_cond or None): B = 2, t = (981, 17), S = 77 - the inputs of every graph test."""
    t = torch.tensor([981, 17] * (B // 2))
    added = None
    if getattr(cfg, "addition_embed_type", None) == "text_time":
        added = {"text_embeds": _randn(B, 32, seed=4), "time_ids": torch.tensor([[128., 128, 0, 0, 128, 128]] * B)}
    return (_randn(B, cfg.in_channels, H, W, seed=1), t, _randn(B, S, cfg.cross_attention_dim, seed=2),
            _randn(B, cfg.out_channels, H, W, seed=3), added)


# ---- topology ----------------------------------------------------------------------------------------------------------------------------
def node_names(cfg):
    """Node names in the order the forward produces them (the reverse sweep meets them back to front)."""
    n, out = len(cfg.block_out_channels), ["conv_in"]

    def level(p, resnets, attn, sampler):
        for j in range(resnets):
            out.append(f"{p}.resnets.{j}")
            if attn:
                out.append(f"{p}.attentions.{j}")
        if sampler:
            out.append(p + sampler)
    for i in range(n):
        level(f"down_blocks.{i}", cfg.layers_per_block, cfg.attn_levels[i], ".downsamplers.0" if i < n - 1 else None)
    out.extend(["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"])
    for i in range(n):
        level(f"up_blocks.{i}", cfg.layers_per_block + 1, cfg.attn_levels[n - 1 - i], ".upsamplers.0" if i < n - 1 else None)
    return out


def level_taps(cfg, nodes):
    """The old per-level observables ("down<i>", "mid", "up<i>": the last tensor of a level) out of a dict of node tensors."""
    n, names, out = len(cfg.block_out_channels), node_names(cfg), {}
    for i in range(n):
        for kind, key in ((f"down_blocks.{i}.", f"down{i}"), (f"up_blocks.{i}.", f"up{i}")):
            out[key] = nodes[[k for k in names if k.startswith(kind)][-1]]
    out["mid"] = nodes["mid_block.resnets.1"]
    return out


def sites(cfg, sd):
    """site lists by kind of place: resnets, Transformer2Ds, transformer blocks, samplers, up resnets (the ones that read a skip)."""
    names = node_names(cfg)
    res = [k for k in names if ".resnets." in k]
    tr = [k for k in names if ".attentions." in k]
    blocks = [k[:-len(".attn2.to_out.0.weight")] for k in sd if k.endswith(".attn2.to_out.0.weight")]
    return {"resnet": res, "trans": tr, "block": blocks, "sampler": [k for k in names if "samplers.0" in k],
            "up": [k for k in res if k.startswith("up_blocks.")], "shortcut": [k for k in res if (k + ".conv_shortcut.weight") in sd],
            "identity": [k for k in res if (k + ".conv_shortcut.weight") not in sd],
            "down_sampler": [k for k in names if "downsamplers.0" in k]}


# ---- the graph, restated with hooks ------------------------------------------------------------------------------------------------------
class _GradRound(torch.autograd.Function):
    """identity whose backward rounds the gradient: a place where only the reverse sweep stores a tensor"""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


class Ctl:
    """What one evaluation changes: the storage type (None = fp32, no rounding), the fused form, one seeded mistake (kind, site)."""

    def __init__(self, dtype=None, fused=False, mistake=None):
        self.dtype, self.fused, self.mistake = dtype, fused, mistake

    def rd(self, t):                         # a stored tensor (forward value and, on the way back, its gradient)
        return t if self.dtype is None else t.to(self.dtype).to(torch.float32)

    def rd_norm(self, t):                    # the output of a GroupNorm / LayerNorm: not stored where the consumer folds the norm in
        return t if self.fused else self.rd(t)

    def rd_value(self, t):                   # forward value only (an input the library rounds on entry)
        return t if self.dtype is None else t + (self.rd(t) - t).detach()

    def rd_grad(self, t):                    # gradient only
        return t if self.dtype is None else _GradRound.apply(t, self.dtype)

    def hit(self, kind, site):
        return self.mistake is not None and self.mistake == (kind, site)


def _other(t):
    """the tensor of the OTHER sample in each sample's place (batch pairs swapped)"""
    return t.reshape(-1, 2, *t.shape[1:]).flip(1).reshape(t.shape)


def _resnet(x, skip, temb, sd, p, g, c):
    if skip is not None:
        if c.hit("dskip dropped", p):
            skip = skip.detach()
        x = torch.cat([x, skip], dim=1)
    h = c.rd_norm(F.silu(M._gn(x, sd, p + ".norm1", g, 1e-5)))
    h = M._conv(h, sd, p + ".conv1")
    te = _other(temb) if c.hit("timestep of the other sample", p) else temb
    h = c.rd(h + M._lin(F.silu(te), sd, p + ".time_emb_proj")[:, :, None, None])
    h = c.rd_norm(F.silu(M._gn(h, sd, p + ".norm2", g, 1e-5)))
    h = M._conv(h, sd, p + ".conv2")
    if (p + ".conv_shortcut.weight") in sd:
        x = c.rd(M._conv(x, sd, p + ".conv_shortcut", padding=0))
    elif c.hit("identity-shortcut gradient dropped", p):
        x = x.detach()
    return c.rd(x + h)


def _tome_merge(k, v, r, dtype):
    """oracle.tome_ref.tome_merge_kv with the two roundings of the SELECTION (normalised keys, similarity scores) in the storage
    type: kernels_tome.hip keeps both in it, so the fp16 build matches on fp16 values where the oracle's restatement rounds to
    bf16.  Near-ties then fall differently - a discrete difference that belongs to the floor of the fp16 + ToMe rows."""
    if dtype != torch.float16:
        return tome_ref.tome_merge_kv(k, v, r)
    half = k.shape[1] // 2
    r = max(0, min(int(r), half))
    if r == 0:
        return k, v
    with torch.no_grad():
        rd = lambda t: t.to(dtype).to(torch.float32)
        metric = rd(k / k.norm(dim=-1, keepdim=True).clamp_min(1e-15))
        scores = rd(metric[:, 0:2 * half:2] @ metric[:, 1:2 * half:2].transpose(-1, -2))
        node_max, node_idx = scores.max(dim=-1)
        order = torch.sort(-node_max, dim=-1, stable=True).indices
    return tome_ref.merge_wavg(k, order, node_idx, r), tome_ref.merge_wavg(v, order, node_idx, r)


def _block(x, ctx, sd, p, heads, tome_r, c, last):
    C = x.shape[-1]

    def branch(kind, y):
        return y.detach() if c.hit(kind, p) else y
    h = c.rd_norm(F.layer_norm(x, (C,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5))
    k1, v1, q = (c.rd(M._lin(h, sd, p + ".attn1.to_" + n)) for n in "kvq")         # (the oracle's order: gradients then add up in its order)
    if tome_r > 0 and h.shape[1] % 16 == 0:
        k1, v1 = _tome_merge(k1, v1, tome_r, c.dtype)
        if c.hit("ToMe unmerge bypassed", p):
            k1, v1 = k1.detach(), v1.detach()
        k1, v1 = c.rd(k1), c.rd(v1)
    a = c.rd(M.attention(q, k1, v1, heads))
    x = c.rd(x + branch("gradient blocked through attn1 branch", M._lin(a, sd, p + ".attn1.to_out.0")))
    h = c.rd_norm(F.layer_norm(x, (C,), sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-5))
    cx = _other(ctx) if c.hit("context of the other sample", p) else ctx
    a = c.rd(M.attention(c.rd(M._lin(h, sd, p + ".attn2.to_q")), c.rd(M._lin(cx, sd, p + ".attn2.to_k")),
                         c.rd(M._lin(cx, sd, p + ".attn2.to_v")), heads))
    x = c.rd(x + branch("gradient blocked through attn2 branch", M._lin(a, sd, p + ".attn2.to_out.0")))
    h = c.rd_norm(F.layer_norm(x, (C,), sd[p + ".norm3.weight"], sd[p + ".norm3.bias"], 1e-5))
    val, gate = c.rd_grad(M._lin(h, sd, p + ".ff.net.0.proj")).chunk(2, dim=-1)       # the sweep stores d(pre-activation), the forward only the product
    h = c.rd(val * F.gelu(gate))
    x = x + branch("gradient blocked through FF branch", M._lin(h, sd, p + ".ff.net.2"))
    return x if (c.fused and last) else c.rd(x)      # fused: the last FF2 runs inside proj_out's launch, nothing is stored in between


def _transformer(x, ctx, sd, p, heads, g, depth, linear_proj, tome_r, c):
    B, C, H, W = x.shape
    res = x.detach() if c.hit("Transformer2D outer residual's gradient dropped", p) else x
    h = c.rd_norm(M._gn(x, sd, p + ".norm", g, 1e-5 if c.hit("Transformer2D GroupNorm eps 1e-5 for 1e-6", p) else 1e-6))
    if not linear_proj:
        h = M._conv(h, sd, p + ".proj_in", padding=0).permute(0, 2, 3, 1).reshape(B, H * W, C)
    else:
        h = M._lin(h.permute(0, 2, 3, 1).reshape(B, H * W, C), sd, p + ".proj_in")
    h = c.rd(h)
    for d in range(depth):
        h = _block(h, ctx, sd, f"{p}.transformer_blocks.{d}", heads, tome_r, c, d == depth - 1)
    if not linear_proj:
        h = M._conv(h.reshape(B, H, W, C).permute(0, 3, 1, 2), sd, p + ".proj_out", padding=0)
    else:
        h = M._lin(h, sd, p + ".proj_out").reshape(B, H, W, C).permute(0, 3, 1, 2)
    return c.rd(h + res)


def forward(sd, cfg, x, t, ctx, c, tome_r=0, added_cond=None):
    """(eps, {node name: tensor of the graph}) - oracle.models_ref.unet_forward restated over the same leaf functions, with Ctl's
    roundings and seeded mistakes.  With Ctl() it is the oracle bit for bit (tests/test_graph_ref_host.py)."""
    g, boc, nlev = cfg.norm_num_groups, cfg.block_out_channels, len(cfg.block_out_channels)
    nodes = OrderedDict()

    def node(name, y):
        nodes[name] = y
        return y
    temb = M.timestep_embedding(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(x.dtype)
    temb = M._lin(F.silu(M._lin(temb, sd, "time_embedding.linear_1")), sd, "time_embedding.linear_2")     # fp32 rows natively
    if added_cond is not None:
        temb = temb + M.added_cond_embedding(sd, cfg, added_cond["text_embeds"], added_cond["time_ids"])
    ctx = c.rd_value(ctx)

    def trans(h, p, lvl):
        return node(p, _transformer(h, ctx, sd, p, cfg.num_heads[lvl], g, cfg.transformer_depth[lvl], cfg.use_linear_projection, tome_r, c))
    h = node("conv_in", c.rd(M._conv(c.rd_value(x), sd, "conv_in")))
    skips = [h]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            h = node(f"down_blocks.{i}.resnets.{j}", _resnet(h, None, temb, sd, f"down_blocks.{i}.resnets.{j}", g, c))
            if cfg.attn_levels[i]:
                h = trans(h, f"down_blocks.{i}.attentions.{j}", i)
            skips.append(h)
        if i < nlev - 1:
            p = f"down_blocks.{i}.downsamplers.0"
            h = node(p, c.rd(M._conv(h, sd, p + ".conv", stride=2, padding=1)))
            skips.append(h)
    h = node("mid_block.resnets.0", _resnet(h, None, temb, sd, "mid_block.resnets.0", g, c))
    h = trans(h, "mid_block.attentions.0", nlev - 1)
    h = node("mid_block.resnets.1", _resnet(h, None, temb, sd, "mid_block.resnets.1", g, c))
    for i in range(nlev):
        lvl = nlev - 1 - i
        for j in range(cfg.layers_per_block + 1):
            h = node(f"up_blocks.{i}.resnets.{j}", _resnet(h, skips.pop(), temb, sd, f"up_blocks.{i}.resnets.{j}", g, c))
            if cfg.attn_levels[lvl]:
                h = trans(h, f"up_blocks.{i}.attentions.{j}", lvl)
        if i < nlev - 1:
            p = f"up_blocks.{i}.upsamplers.0"
            h = F.interpolate(h, size=skips[-1].shape[-2:], mode="nearest")
            h = node(p, c.rd(M._conv(h, sd, p + ".conv")))
    h = c.rd_norm(F.silu(M._gn(h, sd, "conv_norm_out", g, 1e-5)))
    return c.rd_grad(M._conv(h, sd, "conv_out")), nodes          # eps leaves in fp32; the cotangent is rounded on entry


def _finish(eps, xr, nodes, cot):
    for v in nodes.values():
        v.retain_grad()
    (eps * cot).sum().backward()
    return {"eps": eps.detach(), "d_x": xr.grad, "out": {k: v.detach() for k, v in nodes.items()},
            "grad": {k: v.grad for k, v in nodes.items()}}


def oracle(sd, cfg, x, t, ctx, cot, tome_r=0, added_cond=None):
    """The fp32 reference: oracle/models_ref.py with its node taps, differentiated with the cotangent cot."""
    xr, taps = x.clone().requires_grad_(), {}
    eps = M.unet_forward(sd, cfg, xr, t, ctx, taps=taps, tome_r=tome_r, added_cond=added_cond)
    return _finish(eps, xr, OrderedDict((k, taps[k]) for k in node_names(cfg)), cot)


def emulate(sd, cfg, x, t, ctx, cot, dtype, fused=False, mistake=None, tome_r=0, added_cond=None):
    """The graph with the weights and every stored tensor rounded to dtype (None: fp32, nothing rounded).  fused=True leaves out the
    roundings the inference path's fusions skip: no store after a GroupNorm / LayerNorm folded into its consumer, none between the last
    FF2 and a folded proj_out.  mistake = (kind, site): one seeded mistake of MISTAKES."""
    c = Ctl(dtype, fused, mistake)
    if mistake is not None and MISTAKES[mistake[0]][1] is not None:
        sd = MISTAKES[mistake[0]][1](sd, mistake[1], cfg)
    if dtype is not None:
        sd = {k: (c.rd(v) if v.ndim > 1 else v) for k, v in sd.items()}          # matrices are stored in dtype, biases / norm vectors in fp32
    if mistake is not None and mistake[0] == "stride-2 downsampler's addend dropped":
        c.mistake = ("dskip dropped", _reader_of_input_of(cfg, mistake[1]))
    xr = x.clone().requires_grad_()
    eps, nodes = forward(sd, cfg, xr, t, ctx, c, tome_r=tome_r, added_cond=added_cond)
    return _finish(eps, xr, nodes, cot)


def _reader_of_input_of(cfg, sampler):
    """The up resnet that reads, as its skip, the tensor the given downsampler reads: where the reverse sweep's addend of that
    stride-2 adjoint comes from."""
    n = len(cfg.block_out_channels)
    i = int(sampler.split(".")[1])
    # skips in production order: conv_in, then per level its layers_per_block outputs and its downsampler's output
    k = (i + 1) * cfg.layers_per_block + i                 # index of the level's last resnet / transformer output
    ups = [f"up_blocks.{a}.resnets.{j}" for a in range(n) for j in range(cfg.layers_per_block + 1)]
    return ups[len(ups) - 1 - k]


# ---- mistakes ------------------------------------------------------------------------------------------------------------------------------
def _zero(*suffixes):
    def edit(sd, site, cfg):
        sd = dict(sd)
        for s in suffixes:
            sd[site + s] = torch.zeros_like(sd[site + s])
        return sd
    return edit


def _swap_concat(sd, site, cfg):
    """norm1 / conv1 / conv_shortcut of an up resnet read cat[skip, h] in place of cat[h, skip]: input channels rotated by the skip's width"""
    sd = dict(sd)
    cout = sd[site + ".conv1.weight"].shape[0]
    cin = sd[site + ".conv1.weight"].shape[1]
    # the resnet's first operand has as many channels as the previous node's output; use the rotation by half where both halves are
    # equal and by cout otherwise - any rotation that is not the identity is a wrong concat order
    sh = cin // 2 if cin == 2 * cout else cout
    perm = torch.arange(cin).roll(sh)
    for k in (".norm1.weight", ".norm1.bias"):
        sd[site + k] = sd[site + k][perm]
    for k in (".conv1.weight", ".conv_shortcut.weight"):
        sd[site + k] = sd[site + k][:, perm]
    return sd


# kind -> (site list key of sites(), state-dict edit or None when the mistake is a hook of forward())
MISTAKES = OrderedDict([
    # the 18 kinds of the sensitivity table: forward mistakes as state-dict edits, gradient-only mistakes as detached branches
    ("time_emb_proj dropped", ("resnet", _zero(".time_emb_proj.weight", ".time_emb_proj.bias"))),
    ("conv1 bias dropped", ("resnet", _zero(".conv1.bias"))),
    ("conv2 bias dropped", ("resnet", _zero(".conv2.bias"))),
    ("shortcut bias dropped", ("shortcut", _zero(".conv_shortcut.bias"))),
    ("attn1 to_out bias dropped", ("block", _zero(".attn1.to_out.0.bias"))),
    ("attn2 to_out bias dropped", ("block", _zero(".attn2.to_out.0.bias"))),
    ("ff.net.2 bias dropped", ("block", _zero(".ff.net.2.bias"))),
    ("ff.net.0.proj bias dropped", ("block", _zero(".ff.net.0.proj.bias"))),
    ("proj_in bias dropped", ("trans", _zero(".proj_in.bias"))),
    ("proj_out bias dropped", ("trans", _zero(".proj_out.bias"))),
    ("LN1 beta dropped", ("block", _zero(".norm1.bias"))),
    ("LN2 beta dropped", ("block", _zero(".norm2.bias"))),
    ("LN3 beta dropped", ("block", _zero(".norm3.bias"))),
    ("resnet norm2 beta dropped", ("resnet", _zero(".norm2.bias"))),
    ("sampler conv bias dropped", ("sampler", _zero(".conv.bias"))),
    ("gradient blocked through attn1 branch", ("block", None)),
    ("gradient blocked through attn2 branch", ("block", None)),
    ("gradient blocked through FF branch", ("block", None)),
    # graph-only kinds
    ("context of the other sample", ("block", None)),
    ("timestep of the other sample", ("resnet", None)),
    ("skip concat halves swapped", ("up", _swap_concat)),
    ("dskip dropped", ("up", None)),
    ("Transformer2D outer residual's gradient dropped", ("trans", None)),
    ("identity-shortcut gradient dropped", ("identity", None)),
    ("stride-2 downsampler's addend dropped", ("down_sampler", None)),
    ("ToMe unmerge bypassed", ("block", None)),
    ("Transformer2D GroupNorm eps 1e-5 for 1e-6", ("trans", None)),
])
TABLE_KINDS = list(MISTAKES)[:18]
TOME_KINDS = ("ToMe unmerge bypassed",)          # evaluated with tome_r = TOME_R on both sides

# (kind, site) pairs the fp16 criteria cannot see, each with its reason.  No site of the 18 TABLE_KINDS may appear here.
BLIND = {("Transformer2D GroupNorm eps 1e-5 for 1e-6", s): "group variance of order 1: eps 1e-5 against 1e-6 changes rstd by 5e-6, far below one fp16 rounding"
         for s in ("down_blocks.0.attentions.0", "down_blocks.0.attentions.1", "down_blocks.1.attentions.0", "down_blocks.1.attentions.1",
                   "mid_block.attentions.0", "up_blocks.1.attentions.0", "up_blocks.1.attentions.1", "up_blocks.1.attentions.2",
                   "up_blocks.2.attentions.0", "up_blocks.2.attentions.1", "up_blocks.2.attentions.2")}


def catalogue(cfg, sd):
    """every (kind, site) pair of the config"""
    s = sites(cfg, sd)
    return [(kind, site) for kind, (where, _) in MISTAKES.items() for site in s[where]]


# ---- verdict -------------------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def distances(got, ref):
    """rel-L2 of every observable: {"eps": .., "d_x": .., "out": {node: ..}, "grad": {node: ..}}"""
    return {"eps": rel_l2(got["eps"], ref["eps"]), "d_x": rel_l2(got["d_x"], ref["d_x"]),
            "out": {k: rel_l2(got["out"][k], v) for k, v in ref["out"].items()},
            "grad": {k: rel_l2(got["grad"][k], v) for k, v in ref["grad"].items()}}


def verdict(got, ref, floors, dtype=None):
    """Per observable rel-L2(got, ref) / (2 x floor); passes iff every ratio is <= 1.  floors: a FLOORS row (or a fresh `distances`).
    Returns (passed, ratios in the layout of `distances`, (worst ratio, group, name) per group)."""
    d = distances(got, ref)
    ratios = {"eps": d["eps"] / (2 * floors["eps"]), "d_x": d["d_x"] / (2 * floors["d_x"]),
              "out": {k: v / (2 * floors["out"][k]) for k, v in d["out"].items()},
              "grad": {k: v / (2 * floors["grad"][k]) for k, v in d["grad"].items()}}
    worst = {"eps": (ratios["eps"], "eps"), "d_x": (ratios["d_x"], "d_x")}
    for grp in ("out", "grad"):
        k = max(ratios[grp], key=lambda n: ratios[grp][n] if not math.isnan(ratios[grp][n]) else float("inf"))
        worst[grp] = (ratios[grp][k], k)
    ok = all(w[0] <= 1.0 for w in worst.values())           # NaN compares false: a NaN observable fails
    return ok, ratios, worst


def worst_ratio(worst):
    vals = [w[0] for w in worst.values()]
    return float("inf") if any(math.isnan(v) for v in vals) else max(vals)


def measure_floor(name, size, dtype, tome_r=0):
    """distances of plain `emulate` from the fp32 oracle for one FLOORS key"""
    cfg = CONFIGS[name]
    sd = state_dict(cfg)
    x, t, ctx, cot, added = inputs(cfg, *size)
    ref = oracle(sd, cfg, x, t, ctx, cot, tome_r=tome_r, added_cond=added)
    return distances(emulate(sd, cfg, x, t, ctx, cot, dtype, tome_r=tome_r, added_cond=added), ref)


def floor_key(name, size, dtype, tome_r=0):
    return (name + (f"+tome{tome_r}" if tome_r else ""), tuple(size), DT_NAME[dtype])


def compact(d, cfg):
    """a `distances` dict as the literal stored below: node values as lists in node_names order"""
    names = node_names(cfg)
    return {"eps": d["eps"], "d_x": d["d_x"], "out": [d["out"][k] for k in names], "grad": [d["grad"][k] for k in names]}


def floors_for(name, size, dtype, tome_r=0):
    """the stored FLOORS row as a `distances`-shaped dict"""
    row = FLOORS[floor_key(name, size, dtype, tome_r)]
    names = node_names(CONFIGS[name])
    return {"eps": row["eps"], "d_x": row["d_x"], "out": dict(zip(names, row["out"])), "grad": dict(zip(names, row["grad"]))}


# Emulation distances: plain emulate() against the fp32 oracle, rel-L2 per observable; node lists in node_names() order.
# Re-measured and compared (10 %) by tests/test_graph_ref_host.py::test_floor_table_is_current, whose printed `FLOORS[...] = ...` lines
# are the way to update this table.
# ---- FLOORS begin (the lines tests/test_graph_ref_host.py::test_floor_table_is_current prints) ----
FLOORS = {}
FLOORS[('graph', (16, 16), 'bf16')] = {'eps': 9.559e-03, 'd_x': 1.247e-02,
    'out': [2.829e-03, 3.491e-03, 4.389e-03, 4.835e-03, 5.479e-03, 5.870e-03, 6.687e-03, 7.467e-03, 7.708e-03, 8.228e-03, 8.595e-03, 8.795e-03, 8.928e-03, 9.158e-03, 9.406e-03, 9.570e-03, 9.576e-03, 9.713e-03, 9.601e-03, 9.909e-03, 9.641e-03, 1.020e-02, 9.554e-03, 9.949e-03, 9.588e-03, 1.014e-02, 1.047e-02, 1.005e-02, 1.035e-02, 9.128e-03, 9.495e-03, 8.772e-03, 9.172e-03],
    'grad': [1.234e-02, 1.341e-02, 1.304e-02, 1.407e-02, 1.381e-02, 1.456e-02, 1.487e-02, 1.422e-02, 1.470e-02, 1.395e-02, 1.440e-02, 1.460e-02, 1.476e-02, 1.475e-02, 1.440e-02, 1.425e-02, 1.416e-02, 1.389e-02, 1.359e-02, 1.369e-02, 1.349e-02, 1.269e-02, 1.217e-02, 1.144e-02, 1.117e-02, 1.023e-02, 1.003e-02, 9.561e-03, 8.987e-03, 8.414e-03, 7.800e-03, 7.164e-03, 6.297e-03]}
FLOORS[('graph', (16, 16), 'fp16')] = {'eps': 1.208e-03, 'd_x': 1.582e-03,
    'out': [3.533e-04, 4.412e-04, 5.581e-04, 6.108e-04, 6.853e-04, 7.446e-04, 8.519e-04, 9.382e-04, 9.694e-04, 1.035e-03, 1.086e-03, 1.115e-03, 1.137e-03, 1.161e-03, 1.204e-03, 1.223e-03, 1.200e-03, 1.218e-03, 1.224e-03, 1.263e-03, 1.207e-03, 1.263e-03, 1.218e-03, 1.276e-03, 1.245e-03, 1.305e-03, 1.351e-03, 1.285e-03, 1.320e-03, 1.175e-03, 1.216e-03, 1.121e-03, 1.177e-03],
    'grad': [1.572e-03, 1.707e-03, 1.664e-03, 1.794e-03, 1.753e-03, 1.856e-03, 1.875e-03, 1.806e-03, 1.888e-03, 1.797e-03, 1.853e-03, 1.918e-03, 1.941e-03, 1.958e-03, 1.898e-03, 1.874e-03, 1.859e-03, 1.792e-03, 1.791e-03, 1.750e-03, 1.732e-03, 1.621e-03, 1.553e-03, 1.461e-03, 1.422e-03, 1.302e-03, 1.279e-03, 1.228e-03, 1.159e-03, 1.094e-03, 1.010e-03, 9.211e-04, 8.167e-04]}
FLOORS[('graph', (9, 15), 'bf16')] = {'eps': 9.126e-03, 'd_x': 1.314e-02,
    'out': [2.830e-03, 3.466e-03, 4.426e-03, 4.827e-03, 5.533e-03, 6.089e-03, 6.763e-03, 7.665e-03, 7.945e-03, 8.674e-03, 9.013e-03, 9.208e-03, 9.406e-03, 9.588e-03, 9.815e-03, 9.934e-03, 1.023e-02, 1.010e-02, 9.906e-03, 1.019e-02, 9.620e-03, 1.021e-02, 9.738e-03, 1.031e-02, 9.737e-03, 1.036e-02, 1.047e-02, 9.829e-03, 1.020e-02, 9.148e-03, 9.611e-03, 8.756e-03, 9.140e-03],
    'grad': [1.232e-02, 1.347e-02, 1.319e-02, 1.440e-02, 1.393e-02, 1.491e-02, 1.516e-02, 1.465e-02, 1.519e-02, 1.429e-02, 1.437e-02, 1.437e-02, 1.434e-02, 1.444e-02, 1.388e-02, 1.358e-02, 1.352e-02, 1.387e-02, 1.335e-02, 1.383e-02, 1.372e-02, 1.277e-02, 1.248e-02, 1.149e-02, 1.123e-02, 1.033e-02, 1.030e-02, 1.000e-02, 9.424e-03, 8.794e-03, 8.023e-03, 7.372e-03, 6.442e-03]}
FLOORS[('graph', (9, 15), 'fp16')] = {'eps': 1.147e-03, 'd_x': 1.651e-03,
    'out': [3.510e-04, 4.311e-04, 5.577e-04, 6.101e-04, 6.896e-04, 7.641e-04, 8.478e-04, 9.458e-04, 9.728e-04, 1.061e-03, 1.097e-03, 1.110e-03, 1.142e-03, 1.166e-03, 1.210e-03, 1.232e-03, 1.270e-03, 1.237e-03, 1.225e-03, 1.200e-03, 1.191e-03, 1.259e-03, 1.192e-03, 1.266e-03, 1.213e-03, 1.285e-03, 1.301e-03, 1.243e-03, 1.294e-03, 1.146e-03, 1.203e-03, 1.101e-03, 1.154e-03],
    'grad': [1.581e-03, 1.729e-03, 1.697e-03, 1.842e-03, 1.793e-03, 1.915e-03, 1.976e-03, 1.903e-03, 1.933e-03, 1.819e-03, 1.878e-03, 1.889e-03, 1.955e-03, 1.985e-03, 1.928e-03, 1.893e-03, 1.818e-03, 1.791e-03, 1.766e-03, 1.739e-03, 1.710e-03, 1.604e-03, 1.572e-03, 1.437e-03, 1.407e-03, 1.281e-03, 1.272e-03, 1.229e-03, 1.164e-03, 1.099e-03, 1.014e-03, 9.131e-04, 7.939e-04]}
FLOORS[('graph_lin', (16, 16), 'bf16')] = {'eps': 9.846e-03, 'd_x': 1.264e-02,
    'out': [2.829e-03, 3.491e-03, 4.389e-03, 4.836e-03, 5.495e-03, 5.874e-03, 6.641e-03, 7.383e-03, 7.638e-03, 8.189e-03, 8.642e-03, 8.805e-03, 8.967e-03, 9.176e-03, 9.561e-03, 9.731e-03, 9.777e-03, 9.846e-03, 9.673e-03, 9.959e-03, 9.549e-03, 9.962e-03, 9.531e-03, 9.972e-03, 9.641e-03, 1.007e-02, 1.046e-02, 1.005e-02, 1.034e-02, 9.220e-03, 9.570e-03, 8.891e-03, 9.347e-03],
    'grad': [1.227e-02, 1.321e-02, 1.289e-02, 1.382e-02, 1.354e-02, 1.435e-02, 1.468e-02, 1.400e-02, 1.470e-02, 1.399e-02, 1.446e-02, 1.448e-02, 1.476e-02, 1.476e-02, 1.432e-02, 1.412e-02, 1.381e-02, 1.377e-02, 1.352e-02, 1.370e-02, 1.346e-02, 1.272e-02, 1.211e-02, 1.141e-02, 1.127e-02, 1.034e-02, 1.011e-02, 9.682e-03, 9.164e-03, 8.609e-03, 7.989e-03, 7.354e-03, 6.491e-03]}
FLOORS[('graph_lin', (16, 16), 'fp16')] = {'eps': 1.249e-03, 'd_x': 1.576e-03,
    'out': [3.533e-04, 4.412e-04, 5.577e-04, 6.077e-04, 6.865e-04, 7.445e-04, 8.489e-04, 9.321e-04, 9.598e-04, 1.031e-03, 1.088e-03, 1.113e-03, 1.139e-03, 1.159e-03, 1.194e-03, 1.220e-03, 1.206e-03, 1.217e-03, 1.211e-03, 1.253e-03, 1.213e-03, 1.279e-03, 1.198e-03, 1.255e-03, 1.241e-03, 1.298e-03, 1.337e-03, 1.283e-03, 1.320e-03, 1.175e-03, 1.219e-03, 1.124e-03, 1.177e-03],
    'grad': [1.568e-03, 1.698e-03, 1.662e-03, 1.789e-03, 1.756e-03, 1.860e-03, 1.880e-03, 1.787e-03, 1.839e-03, 1.764e-03, 1.759e-03, 1.849e-03, 1.874e-03, 1.880e-03, 1.836e-03, 1.812e-03, 1.788e-03, 1.733e-03, 1.675e-03, 1.749e-03, 1.729e-03, 1.615e-03, 1.545e-03, 1.440e-03, 1.421e-03, 1.305e-03, 1.272e-03, 1.226e-03, 1.162e-03, 1.099e-03, 1.020e-03, 9.318e-04, 8.246e-04]}
FLOORS[('graph_lin', (9, 15), 'bf16')] = {'eps': 9.191e-03, 'd_x': 1.329e-02,
    'out': [2.830e-03, 3.466e-03, 4.426e-03, 4.827e-03, 5.537e-03, 6.061e-03, 6.725e-03, 7.602e-03, 7.867e-03, 8.497e-03, 8.933e-03, 9.159e-03, 9.261e-03, 9.429e-03, 9.742e-03, 9.912e-03, 1.035e-02, 1.014e-02, 1.002e-02, 9.980e-03, 9.399e-03, 1.007e-02, 9.548e-03, 1.010e-02, 9.680e-03, 1.026e-02, 1.041e-02, 9.908e-03, 1.013e-02, 9.011e-03, 9.466e-03, 8.720e-03, 9.182e-03],
    'grad': [1.227e-02, 1.339e-02, 1.316e-02, 1.427e-02, 1.375e-02, 1.474e-02, 1.500e-02, 1.446e-02, 1.494e-02, 1.413e-02, 1.424e-02, 1.434e-02, 1.477e-02, 1.482e-02, 1.438e-02, 1.396e-02, 1.368e-02, 1.381e-02, 1.337e-02, 1.382e-02, 1.365e-02, 1.268e-02, 1.222e-02, 1.131e-02, 1.108e-02, 1.002e-02, 1.010e-02, 9.745e-03, 9.220e-03, 8.798e-03, 8.083e-03, 7.404e-03, 6.494e-03]}
FLOORS[('graph_lin', (9, 15), 'fp16')] = {'eps': 1.163e-03, 'd_x': 1.628e-03,
    'out': [3.510e-04, 4.311e-04, 5.575e-04, 6.126e-04, 6.956e-04, 7.637e-04, 8.444e-04, 9.310e-04, 9.554e-04, 1.044e-03, 1.086e-03, 1.098e-03, 1.122e-03, 1.148e-03, 1.189e-03, 1.199e-03, 1.230e-03, 1.239e-03, 1.215e-03, 1.215e-03, 1.171e-03, 1.236e-03, 1.193e-03, 1.260e-03, 1.208e-03, 1.277e-03, 1.284e-03, 1.234e-03, 1.285e-03, 1.146e-03, 1.199e-03, 1.098e-03, 1.157e-03],
    'grad': [1.547e-03, 1.687e-03, 1.651e-03, 1.800e-03, 1.750e-03, 1.856e-03, 1.904e-03, 1.820e-03, 1.870e-03, 1.765e-03, 1.780e-03, 1.779e-03, 1.788e-03, 1.809e-03, 1.769e-03, 1.731e-03, 1.701e-03, 1.720e-03, 1.671e-03, 1.715e-03, 1.710e-03, 1.584e-03, 1.530e-03, 1.388e-03, 1.362e-03, 1.238e-03, 1.281e-03, 1.234e-03, 1.171e-03, 1.102e-03, 1.022e-03, 9.245e-04, 8.087e-04]}
FLOORS[('graph+tome40', (16, 16), 'bf16')] = {'eps': 1.111e-02, 'd_x': 2.022e-02,
    'out': [2.829e-03, 3.491e-03, 4.541e-03, 4.952e-03, 6.186e-03, 6.453e-03, 7.174e-03, 9.643e-03, 9.848e-03, 1.101e-02, 1.098e-02, 1.117e-02, 1.123e-02, 1.139e-02, 1.155e-02, 1.165e-02, 1.175e-02, 1.150e-02, 1.144e-02, 1.159e-02, 1.174e-02, 1.340e-02, 1.243e-02, 1.436e-02, 1.355e-02, 1.420e-02, 1.454e-02, 1.344e-02, 1.377e-02, 1.181e-02, 1.207e-02, 1.088e-02, 1.137e-02],
    'grad': [1.979e-02, 2.203e-02, 2.177e-02, 2.464e-02, 2.400e-02, 2.660e-02, 2.850e-02, 2.571e-02, 2.735e-02, 2.535e-02, 2.545e-02, 2.605e-02, 2.601e-02, 2.585e-02, 2.550e-02, 2.519e-02, 2.493e-02, 2.531e-02, 2.520e-02, 2.591e-02, 2.597e-02, 2.192e-02, 2.164e-02, 1.434e-02, 1.420e-02, 1.214e-02, 1.190e-02, 1.148e-02, 1.081e-02, 1.031e-02, 9.593e-03, 8.927e-03, 7.551e-03]}
FLOORS[('graph+tome40', (16, 16), 'fp16')] = {'eps': 2.786e-03, 'd_x': 6.493e-03,
    'out': [3.533e-04, 4.412e-04, 1.259e-03, 1.277e-03, 2.340e-03, 2.289e-03, 2.346e-03, 3.182e-03, 3.184e-03, 3.251e-03, 3.280e-03, 3.287e-03, 3.284e-03, 3.308e-03, 3.335e-03, 3.349e-03, 3.188e-03, 3.264e-03, 3.325e-03, 3.287e-03, 3.304e-03, 3.369e-03, 3.316e-03, 4.475e-03, 4.150e-03, 4.235e-03, 4.338e-03, 3.904e-03, 4.207e-03, 3.404e-03, 3.513e-03, 2.961e-03, 2.996e-03],
    'grad': [6.733e-03, 7.800e-03, 7.414e-03, 8.573e-03, 7.288e-03, 8.337e-03, 9.098e-03, 7.777e-03, 7.810e-03, 7.653e-03, 7.571e-03, 7.621e-03, 7.588e-03, 7.496e-03, 7.407e-03, 7.402e-03, 7.296e-03, 7.210e-03, 7.245e-03, 7.620e-03, 7.656e-03, 7.701e-03, 7.582e-03, 3.899e-03, 3.896e-03, 3.562e-03, 3.599e-03, 3.592e-03, 2.821e-03, 2.722e-03, 2.185e-03, 2.060e-03, 1.864e-03]}
FLOORS[('tiny_sdxl', (16, 16), 'bf16')] = {'eps': 9.458e-03, 'd_x': 1.346e-02,
    'out': [2.804e-03, 3.492e-03, 4.106e-03, 4.798e-03, 5.639e-03, 6.646e-03, 7.008e-03, 7.754e-03, 7.665e-03, 8.278e-03, 9.143e-03, 9.321e-03, 1.017e-02, 1.035e-02, 1.100e-02, 1.109e-02, 1.090e-02, 1.145e-02, 1.083e-02, 1.133e-02, 1.150e-02, 1.205e-02, 1.219e-02, 1.166e-02, 1.201e-02, 1.105e-02, 1.160e-02, 1.109e-02, 1.182e-02, 1.194e-02, 1.152e-02, 1.033e-02, 8.748e-03],
    'grad': [1.339e-02, 1.552e-02, 1.736e-02, 1.913e-02, 1.966e-02, 1.893e-02, 2.097e-02, 2.028e-02, 2.171e-02, 2.256e-02, 2.127e-02, 2.201e-02, 2.056e-02, 2.139e-02, 2.007e-02, 2.001e-02, 1.960e-02, 1.809e-02, 1.807e-02, 1.676e-02, 1.644e-02, 1.468e-02, 1.425e-02, 1.405e-02, 1.306e-02, 1.291e-02, 1.182e-02, 1.142e-02, 9.484e-03, 8.793e-03, 8.094e-03, 7.358e-03, 6.293e-03]}
FLOORS[('tiny_sdxl', (16, 16), 'fp16')] = {'eps': 1.149e-03, 'd_x': 1.682e-03,
    'out': [3.488e-04, 4.387e-04, 5.133e-04, 6.026e-04, 7.159e-04, 8.365e-04, 8.748e-04, 9.521e-04, 9.796e-04, 1.039e-03, 1.168e-03, 1.187e-03, 1.267e-03, 1.283e-03, 1.376e-03, 1.409e-03, 1.374e-03, 1.431e-03, 1.367e-03, 1.419e-03, 1.397e-03, 1.476e-03, 1.506e-03, 1.481e-03, 1.548e-03, 1.403e-03, 1.474e-03, 1.409e-03, 1.475e-03, 1.501e-03, 1.439e-03, 1.288e-03, 1.087e-03],
    'grad': [1.695e-03, 1.993e-03, 2.222e-03, 2.406e-03, 2.482e-03, 2.428e-03, 2.650e-03, 2.582e-03, 2.805e-03, 2.963e-03, 2.746e-03, 2.871e-03, 2.707e-03, 2.781e-03, 2.589e-03, 2.567e-03, 2.547e-03, 2.393e-03, 2.372e-03, 2.192e-03, 2.178e-03, 1.944e-03, 1.859e-03, 1.810e-03, 1.685e-03, 1.668e-03, 1.503e-03, 1.450e-03, 1.215e-03, 1.119e-03, 1.023e-03, 9.329e-04, 8.083e-04]}
# ---- FLOORS end ----
