"""float64 reference and error model of the time-embedding chain (csrc/kernels_elem.hip: k_timestep_embedding, k_rowvec_linear,
k_rowvec_small<1|2|4, 0|1|2>, k_silu_inplace_f32), with a numpy fp32 emulation of the same expressions and summation order.
TEST INFRASTRUCTURE, shared by tests/test_temb_ref_host.py (CPU) and tests/test_gpu_temb.py (-m gpu).  u = 2^-24 throughout.

Embedding (diffusers get_timestep_embedding):  freq_i = exp(-ln(10000) i / (half - shift)), a = t freq_i,
out = [sin | cos], or [cos | sin] with flip.      |err| <= (C1 |a| + C2) u,   C1 = 32, C2 = 4:

    the kernel evaluates  E = (fl(ln 10000) * (float)i) / ((float)half - shift):  the constant, the product and the division are
    one rounding each (the denominator is exact) -> 3 u |E|, |E| <= ln 10000 = 9.21 -> 27.7 u relative in exp(E);  expf itself is
    1 ulp = 2 u;  t * freq one more u  ->  relative error of a <= 30.7 u, rounded up to C1 = 32;  |d sin / da| <= 1 turns it into
    32 u |a| absolute.  sinf / cosf are 2 ulp of a result of magnitude <= 1  ->  C2 = 4.

SiLU as the kernels compute it, silu_f(x) = x * rcp(1 + exp2(-log2(e) x)):  relative error s(x) u with

    s(x) = 4 + (2 |x| + 2) sigmoid(-x)

    the argument z = fl(-log2 e) * x carries 2 u |z| (constant, product), i.e. 2 u |x| relative in 2^z;  v_exp_f32 is 1 ulp = 2 u;
    both reach the denominator 1 + e scaled by e / (1 + e) = sigmoid(-x);  then the addition (u), v_rcp_f32 (1 ulp = 2 u) and the
    final multiply (u): 4.  For x >= 0 this is below 6; on the negative tail (x = -80: 166) the argument rounding dominates - a
    relative error of a value of magnitude 80 e^-80, which is why s stays a function of x instead of a constant.

Row-vector linear, out = sum_k f(x_k) w_k + bias, stored as fp32 (check_bound(..., hdt=torch.float32) adds u |ref|):

    |err| <= u sum_k (8 ceil(K / 512) + 7 + s_k) |f(x_k)| |w_k| + (8 ceil(K / 512) + 7) u |bias|

    a lane adds its products in ceil(K / 512) chunks of 8 fused multiply-adds, the xor butterfly 32 .. 1 adds 6 more partial sums
    and the bias is one further addition: no product passes more than 8 ceil(K / 512) + 7 roundings, each relative to a partial
    sum that sum |f(x)| |w| + |bias| bounds.  s_k = s(x_k) with SiLU on the input, 0 without.  Weights are 16-bit storage values
    and enter exactly.

The constants come from the derivation above, not from a device.  tests/test_temb_ref_host.py confirms them with the fp32
emulation below (same expressions, lane-strided chunks of 8, then the butterfly), which must stay under one half of the
tolerance.  Its worst ratios |err| / tolerance:

    embedding 0.30        linear 0.11 (bf16 weights), 0.17 (fp16 weights)
    SiLU 0.57 of s(x) at x = -45.4, where the argument product - an IEEE multiply, the same on every machine, whose bound
         2 |x| sigmoid(-x) is sharp - is nearly all of s; of the part an implementation may do differently from the emulation
         (exp2 and the reciprocal, budgeted at 1 ulp each, correctly rounded in numpy) it uses 0.25, and 0.5 is what the host
         test demands of that part."""
from __future__ import annotations

import math

import numpy as np
import torch

Tensor = torch.Tensor
U32 = 2.0 ** -24
C1, C2 = 32.0, 4.0
T_VALUES = (0, 1, 12, 637, 999)
LN10000 = math.log(10000.0)


# ---- float64 reference --------------------------------------------------------------------------------------------------------------
def embedding64(t: Tensor, dim: int, flip: int, shift: float):
    """t [B] int64 -> (emb [B, dim] float64, a [B, dim] = the sine / cosine argument of every column)."""
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64)
    freq = torch.exp(-LN10000 * i / (half - float(shift)))
    a = t.double()[:, None] * freq[None, :]
    s, c = torch.sin(a), torch.cos(a)
    emb = torch.cat([c, s], 1) if flip else torch.cat([s, c], 1)
    return emb, torch.cat([a, a], 1)


def embedding_tolerance(a: Tensor) -> Tensor:
    return (C1 * a.abs() + C2) * U32


def silu64(x: Tensor) -> Tensor:
    x = x.double()
    return x * torch.sigmoid(x)


def silu_s(x: Tensor) -> Tensor:
    x = x.double()
    return 4.0 + (2.0 * x.abs() + 2.0) * torch.sigmoid(-x)


def lin_k(K: int) -> float:
    return 8.0 * ((K + 511) // 512) + 7.0


def linear64(x: Tensor, W: Tensor, bias, silu: bool):
    """x [B, K], W [N, K], bias [N] or None -> (out [B, N] float64, bound [B, N]): |err| <= u bound + u |out| (module docstring;
    pass bound to gpu_util.check_bound with k = 1, hdt = torch.float32)."""
    K = x.shape[1]
    xd, Wd = x.double(), W.double()
    fx = silu64(xd) if silu else xd
    weight = lin_k(K) + (silu_s(xd) if silu else 0.0)
    out = fx @ Wd.t()
    bound = (fx.abs() * weight) @ Wd.abs().t()
    if bias is not None:
        out = out + bias.double()[None, :]
        bound = bound + lin_k(K) * bias.double().abs()[None, :]
    return out, bound


def linear_inputs(K: int, N: int, rows: int, seed: int):
    """x [rows, K] fp32: Gaussian rows; row 1 holds the SiLU tails only (entries in +-[20, 80]) and row 0 is Gaussian with a tail
    entry in every fifth column (the one-row kernels see the tails too).  W [N, K] Gaussian of magnitude 1 / sqrt(K), bias [N]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    tails = (20.0 + 60.0 * torch.rand(K, generator=g)) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
    if rows > 1:
        x[1] = tails
    x[0, ::5] = tails.flip(0)[::5]
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    return x, W, bias


def timesteps(B: int, offset: int = 0) -> Tensor:
    return torch.tensor([T_VALUES[(b + offset) % len(T_VALUES)] for b in range(B)], dtype=torch.int64)


# ---- fp32 emulation of the kernels (numpy) ------------------------------------------------------------------------------------------
F = np.float32


def embedding_emulate_f32(t: Tensor, dim: int, flip: int, shift: float) -> np.ndarray:
    half = dim // 2
    j = np.arange(dim)
    i = np.where(j < half, j, j - half).astype(F)
    e = (F(-9.210340371976184) * i) / (F(half) - F(shift))
    freq = np.exp(e.astype(F)).astype(F)
    a = (t.numpy().astype(F)[:, None] * freq[None, :]).astype(F)
    is_cos = (j < half) if flip else (j >= half)
    return np.where(is_cos[None, :], np.cos(a).astype(F), np.sin(a).astype(F)).astype(F)


def silu_emulate_f32(x: np.ndarray) -> np.ndarray:
    x = x.astype(F)
    e = np.exp2((F(-1.4426950408889634) * x).astype(F)).astype(F)
    return (x * (F(1.0) / (F(1.0) + e)).astype(F)).astype(F)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def linear_emulate_f32(fx: np.ndarray, W: np.ndarray, bias) -> np.ndarray:
    """k_rowvec_linear / k_rowvec_small on already-transformed fp32 inputs fx [B, K]: lane l owns columns l * 8 + 512 c .. + 7,
    fused multiply-adds in ascending k, the xor butterfly 32 .. 1, then the bias."""
    B, K = fx.shape
    N = W.shape[0]
    T = (K + 511) // 512
    xp = np.zeros((B, T * 512), F)
    wp = np.zeros((N, T * 512), F)
    xp[:, :K], wp[:, :K] = fx, W                       # a zero product leaves the accumulator as it is, like the skipped chunk
    xp, wp = xp.reshape(B, 1, T, 64, 8), wp.reshape(1, N, T, 64, 8)
    acc = np.zeros((B, N, 64), F)
    for c in range(T):
        for j in range(8):
            acc = _fma(xp[:, :, c, :, j], wp[:, :, c, :, j], acc)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, :, lanes ^ off]).astype(F)
    out = acc[:, :, 0]
    return (out + bias.astype(F)[None, :]).astype(F) if bias is not None else out
