"""Reference side of the ControlNet tests (helper, not collected).

  ctrl_forward      the diffusers ControlNetModel forward, restated over the leaves of oracle.models_ref (_conv, resnet_block,
                    transformer_2d, timestep_embedding): conditioning embedding of the hint image, conv_in(latents) + embedding, time
                    embedding, the UNet's down path and mid block, one 1x1 zero convolution per collected tensor.  The collected
                    tensors themselves come back through ``taps`` (tests/test_ctrl_host.py pins them to oracle unet_forward).
  hint_scales       the per-residual scales of a ControlNet hint (weight, soft_injection) - reference unified_pipeline.py:1040-1050
  place             where the residuals of one hint land on a CFG side (cfg_only) - reference unified_pipeline.py:1026-1058
  emit_* / silu_*   float64 values, fp32 host emulations and element-wise error bounds of the two kernels of kernels_ctrl.hip

Error models (derived here, from the number formats and the kernels' arithmetic, not from GPU output).  u_s = 2^-8 (bf16), 2^-11
(fp16) is the unit roundoff of the storage type, f_s = 2^-134 / 2^-25 half its smallest subnormal, e = 2^-24 the unit roundoff of fp32.

ctrl_emit writes  rnd(fl(fl(scale f) + old))  (old = 0 and no addition on assign).  With E = scale f + old exact in float64:
    |fl(fl(scale f) + old) - E| <= e |scale f| + e |E| + 2^-149        (one product, one sum, a denormal step)          =: a
    |rnd(v) - v| <= u_out |v| + f_out,   |v| <= |E| + a                 (nothing for an fp32 output: it is stored as computed)
    bound = a + u_out (|E| + a) + f_out.
silu writes  rnd(x * rcp(1 + exp2(-log2(e) x)))  with 1-ulp hardware exp2 and rcp.  The argument of exp2 carries a relative error of
2^-23 (the constant and the product), i.e. an absolute one of 2^-23 |x| log2(e), which exp2 turns into a relative error of 2^-23 |x|;
with its own ulp, the sum, the reciprocal and the product that is at most 2^-23 (3 + |x|) relative on x sigmoid(x).  Where
sigmoid(x) < 2^-126 the reciprocal underflows (or the exponential overflows and rcp(inf) = 0) and the result is -0: an absolute error
of at most |x| 2^-126.  So with S = x sigmoid(x) exact:
    a = |S| 2^-23 (3 + |x|) + |x| 2^-126,      bound = a + u_s (|S| + a) + f_s.
"""
import math

import torch
import torch.nn.functional as F

from oracle import models_ref as M

UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
FLOOR = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 0.0}
E32 = 2.0 ** -24


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def cond_embedding(sd, image):
    p = "controlnet_cond_embedding"
    h = F.silu(M._conv(image, sd, p + ".conv_in"))
    k = 0
    while f"{p}.blocks.{k}.weight" in sd:
        h = F.silu(M._conv(h, sd, f"{p}.blocks.{k}", stride=2 if k % 2 else 1))
        k += 1
    return M._conv(h, sd, p + ".conv_out")


def ctrl_forward(sd, cfg, latents, t, ctx, image, taps=None):
    """[down residual 0 .. N-1, mid residual], unscaled.  cfg: gyre_amd.config.ControlNetConfig (or anything with its fields)."""
    g, eps, boc = cfg.norm_num_groups, 1e-5, cfg.block_out_channels
    B = latents.shape[0]
    if t.ndim == 0:
        t = t[None].expand(B)
    if image.shape[0] == 1 and B > 1:
        image = image.expand(B, -1, -1, -1)
    temb = M.timestep_embedding(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(latents.dtype)
    temb = M._lin(F.silu(M._lin(temb, sd, "time_embedding.linear_1")), sd, "time_embedding.linear_2")
    h = M._conv(latents, sd, "conv_in") + cond_embedding(sd, image)
    skips = [h]
    n = len(boc)
    for i in range(n):
        for j in range(cfg.layers_per_block):
            h = M.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}", g, eps)
            if cfg.attn_levels[i]:
                h = M.transformer_2d(h, ctx, sd, f"down_blocks.{i}.attentions.{j}", cfg.num_heads[i], g, cfg.transformer_depth[i],
                                     cfg.use_linear_projection)
            skips.append(h)
        if i < n - 1:
            h = M._conv(h, sd, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(h)
    h = M.resnet_block(h, temb, sd, "mid_block.resnets.0", g, eps)
    h = M.transformer_2d(h, ctx, sd, "mid_block.attentions.0", cfg.num_heads[-1], g, cfg.transformer_depth[-1], cfg.use_linear_projection)
    h = M.resnet_block(h, temb, sd, "mid_block.resnets.1", g, eps)
    if taps is not None:
        taps["skips"], taps["mid"] = list(skips), h
    out = [M._conv(s, sd, f"controlnet_down_blocks.{k}", padding=0) for k, s in enumerate(skips)]
    out.append(M._conv(h, sd, "controlnet_mid_block", padding=0))
    return out


# ---- hint weighting ------------------------------------------------------------------------------------------------------------------
def hint_scales(weight, soft_injection, n):
    """n = down residuals + 1: weight x logspace(-1, 0, n)[k] for down residual k and the last point for the mid one; weight alone
    without soft injection."""
    if not soft_injection:
        return [float(weight)] * n
    return [float(weight) * float(s) for s in torch.logspace(-1, 0, n)]


def place(residuals, side, cfg_only):
    """What one hint contributes on a CFG side, from its residuals over the guided batch: "g" all of it; "u" nothing for a cfg_only
    hint (None); "f" (unconditional | guided along the batch) zeros below the residuals for a cfg_only hint.  A hint that is not
    cfg_only runs on whatever batch the side has, so its residuals are returned as they are."""
    if not cfg_only or side == "g":
        return list(residuals)
    if side == "u":
        return None
    return [torch.cat([torch.zeros_like(r), r], dim=0) for r in residuals]


# ---- ctrl_emit ---------------------------------------------------------------------------------------------------------------------
def _nchw(f, C):
    """f NHWC [B][HW][Cpad] -> [B][C][HW]"""
    return f[:, :, :C].transpose(1, 2)


def emit_exact(f, C, scale, accumulate, out, b0):
    """float64 value of every element of out after the call, and the magnitude |scale f| (zero outside the window)"""
    B = f.shape[0]
    s = float(torch.tensor(scale, dtype=torch.float32))
    prod = s * _nchw(f.double(), C)
    res = out.double().clone() if accumulate else torch.zeros(out.shape, dtype=torch.float64)
    mag = torch.zeros(out.shape, dtype=torch.float64)
    res[b0:b0 + B] = res[b0:b0 + B] + prod if accumulate else prod
    mag[b0:b0 + B] = prod.abs()
    return res, mag


def emit_bound(exact, mag, out_dtype, accumulate):
    a = E32 * mag + (E32 * exact.abs() if accumulate else 0.0) + 2.0 ** -149
    a = torch.where(mag > 0, a, torch.zeros_like(a))                   # an untouched or zeroed sample carries no error at all
    tail = UNIT[out_dtype] * (exact.abs() + a) + FLOOR[out_dtype]
    return a + torch.where(mag > 0, tail, torch.zeros_like(tail))


def emit_host(f, C, scale, accumulate, out, b0, mistake=None):
    """fp32 host emulation of the kernel: the tensor `out` would hold after the call.  mistake: one of the seeded errors of the
    error-model self-test."""
    B = f.shape[0]
    s = torch.tensor(1.0 if mistake == "scale_dropped" else scale, dtype=torch.float32)
    prod = s * _nchw(f.float(), C)
    if mistake == "rounded_before_accumulate":
        prod = prod.to(f.dtype).float()
    if mistake == "wrong_offset":
        b0 = b0 - 1 if b0 > 0 else b0 + 1
    res = out.clone()
    if accumulate:
        res[b0:b0 + B] = (res[b0:b0 + B].float() + prod).to(out.dtype)
        if mistake == "lower_clobbered":
            res[:b0] = 0
    else:
        if mistake != "lower_not_zeroed":
            res.zero_()
        res[b0:b0 + B] = prod.to(out.dtype)
    return res


# ---- silu --------------------------------------------------------------------------------------------------------------------------
def silu_exact(x):
    xd = x.double()
    return xd * torch.sigmoid(xd)


def silu_bound(x, sdt):
    xd = x.double().abs()
    S = silu_exact(x).abs()
    a = S * 2.0 ** -23 * (3.0 + xd) + xd * 2.0 ** -126
    return a + UNIT[sdt] * (S + a) + FLOOR[sdt]


def silu_host(x):
    xf = x.float()
    return (xf * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * xf)))).to(x.dtype)


def silu_inputs(n, sdt, seed=0):
    """N(0, 3) with the edge values in front: +-0, the largest and the smallest normal and subnormal storage values, +-88, -100,
    -65504 and a NaN."""
    fi = torch.finfo(sdt)
    edge = [0.0, -0.0, fi.max, -fi.max, fi.smallest_normal, -fi.smallest_normal, fi.smallest_normal * fi.eps, -fi.smallest_normal * fi.eps,
            fi.smallest_normal * (1 - fi.eps), 88.0, -88.0, -100.0, -65504.0, float("nan")]
    x = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3.0).to(sdt)
    if n >= 16:
        x[:len(edge)] = torch.tensor(edge, dtype=torch.float64).to(sdt)
    else:                                                             # n = 8: the values that matter most
        x[:] = torch.tensor([0.0, -0.0, 88.0, -88.0, -100.0, -65504.0, float("nan"), fi.smallest_normal * fi.eps], dtype=torch.float64).to(sdt)
    return x


def silu_check(x, y):
    """(worst |y - exact| / bound over the non-NaN inputs, NaN kept, no new NaN / inf)"""
    nan = torch.isnan(x)
    ok = ~nan
    err = (y.double()[ok] - silu_exact(x)[ok]).abs()
    ratio = float((err / silu_bound(x, x.dtype)[ok]).max()) if bool(ok.any()) else 0.0
    return ratio, bool(torch.isnan(y[nan]).all()), bool(torch.isfinite(y[ok]).all())
