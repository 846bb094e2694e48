"""float64 reference, error model and input families of the forward normalisation checks (tests/test_gpu_norm_fwd.py on the GPU,
tests/test_norm_fwd_ref_host.py on the host).  Nothing here touches a GPU.

Reference.  Everything is float64 on the exact 16-bit values the kernel is handed.  GroupNorm over the [B, G, HW * cpg] view
(LayerNorm: one set per row): xh = (x - mean) rstd, u = xh gamma + beta, ref = u or silu(u); mean / var (biased) / rstd in float64.
bound = |xh gamma| + |beta| is the absolute-value form of u (times 1.1 with SiLU: sup |silu'| = 1.0998), so an element whose true
output is about zero is still measured against the size of its own terms.

Error model.  Every element is held to  |got - ref| <= k u bound + u |ref| + fp32 term + floor  (gpu_util.check_bound, `tiny` = the
fp32 term as a tensor), u the unit roundoff of the storage type (2^-8 bf16, 2^-11 fp16).

  16-bit roundings (csrc/kernels_elem.hip).  x is read exactly, gamma / beta are fp32, all arithmetic is fp32 and the result is rounded
  to 16 bits ONCE, on store: that is the u |ref| term.  No other 16-bit rounding exists on any GroupNorm / LayerNorm path, so k counts
  fp32 roundings only and is tiny in units of u:  k = n32 2^-24 / u.
    affine part, n32 = K32 = 8.  One-pass form y = fma(a, x, b): a = rstd gamma (1), mean a (1), beta - . (1), the fma (1); two-pass
    form ((x - mean) rstd) gamma + beta: 4 roundings as well.  rstd itself where its error is NOT amplified (kappa = 1): rsqrt
    (hardware approximation, <= 1 ulp = 2 roundings), the division by the count and the + eps (2, halved by the square root): 4 more
    relative to |xh gamma| <= bound.  The summation error of the statistics is the separate fp32 term below.
    SiLU, n32 += K32_SILU = 6.  silu_f(v) = v rcp(1 + exp2(-log2e v)): the product with log2e (its absolute error |v| 2^-24 in the
    exponent moves silu by |v|^2 s (1 - s) 2^-24 <= 0.44 |v| 2^-24: under 1), v_exp_f32 and v_rcp_f32 (1 ulp each = 2 roundings
    each), the 1 + . (1) and the final product (1).  Each is relative to |silu(v)| <= |v| <= bound.  The error u carries into the
    SiLU is scaled by |silu'| <= 1.0998: the factor 1.1 on bound and on the fp32 term.
  So k = 8 2^-24 / u plain and 14 2^-24 / u with SiLU: 1.2e-4 / 2.1e-4 (bf16), 9.8e-4 / 1.7e-3 (fp16) - the 16-bit tolerance is
  the output's own rounding and nothing else.

  fp32 term (conditioning).  kappa = (mean^2 + var) / (var + eps) per normalised set: E[x^2] over the variance the kernel divides by.
    one-pass paths (k_gn_partial -> k_gn_finalize / the k_gn_apply_fin and k_gn_fold prologues; the ln_parts finish of the GEMM
    epilogue): var = E[x^2] - mean^2 from fp32 sums.  A relative error d of the sums is a relative error kappa d of var, kappa d / 2
    of rstd: c32 2^-24 kappa |xh gamma|.  And y = a x + (beta - mean a) cancels two numbers of size |mean| rstd |gamma| =
    sqrt(kappa - 1) |gamma| (the rounding of mean a, of the fma, and the error of mean itself): c32 2^-24 sqrt(kappa) |gamma|.
    two-pass paths (k_gn_small, k_layernorm, ln_linear with the statistics pass): the centred sum has no cancellation (that part is
    in K32); x - mean still carries the error of mean, |mean| 2^-24 rstd |gamma|: c32 2^-24 sqrt(kappa) |gamma| only.
  c32 stands for the summation error of the kernel's own order in units of 2^-24.  A lane adds up to 256 pixel rows sequentially,
  then PY <= 32 lanes, the cpg channels of the group, the chunks (<= 17 per part) and the parts (<= 8) are added in turn: chains of a
  few hundred additions of same-sign terms (x^2, or x at a large mean), whose error grows like the square root of the chain length
  times the mean partial sum - several 2^-24, not hundreds.  The fp32 emulation of tests/test_norm_fwd_ref_host.py (same chunk rule,
  same order) fixes the number: C32 is chosen so that the emulation's fp32 error BEFORE the output rounding is at most 0.5 of the
  tolerance without its u |ref| term at group means of 0 ... 512 sigma, a factor 2 of room for the device's different but equally
  long order (the measured ratios are in that file's docstring).  The rounded output itself reaches u |ref| by construction.

GroupNorm fold (k_gn_fold; gyre_op_gn_fold).  Checked are the folded weights and bias, not a GEMM output.  Wf[b][n][k] against
W[n][k] a[b][k], a = rstd gamma: one 16-bit rounding (u |ref|), K32 fp32 roundings, and c32 2^-24 kappa |ref| (rstd of a one-pass
variance).  bf[b][n] (fp32, never rounded to 16 bits: fold_bias_tol, no u term) against bias[n] + sum_k W[n][k] (beta[k] - mean a[b][k]):
c32 2^-24 sum_k |W| (|beta| + |mean a|) (1 + kappa).

Folded LayerNorm -> GEMM (gyre_op_ln_linear).  ref = sum_k n_k W_k + bias, n = xh gamma + beta in float64;
bound = sum_k (|xh_k gamma_k| + |beta_k|) |W_k| + |bias|.  16-bit roundings: the weights are rounded AFTER the gamma scaling
(k_ln_fold packs W gamma): gamma_k W_k (1 + d_k), |d_k| <= u, moves the sum by at most u sum_k |xh_k gamma_k W_k| <= u bound - one
rounding, where normalise-then-project rounds n instead (also one, on a different product).  beta W is summed in fp32 (no
rounding), the column sum is taken over the ROUNDED folded weights (consistent with the product, no further term), the output is
rounded once (u |ref|).  K_LN_LINEAR = 1 (+ K32 fp32 roundings).  fp32 term: the epilogue forms rstd acc - rstd mean colsum, two
numbers of size sqrt(kappa) sum |gamma W| accumulated over K in fp32, plus the rstd error kappa / 2 of the parts route:
c32 2^-24 (kappa + sqrt(kappa)) sum_k |gamma_k W_k| (statistics pass: the sqrt(kappa) part only).
"""
import math

import torch

import gpu_util

U32 = 2.0 ** -24
K32 = 8.0
K32_SILU = 6.0
SILU_SUP = 1.1                        # sup |silu'| = 1.0998
K_LN_LINEAR = 1.0
# summation constants, set by the emulation of tests/test_norm_fwd_ref_host.py (worst emulated ratio <= 0.5)
C32_ONE = 10.0                        # one-pass GroupNorm: k_gn_partial sums finished by k_gn_finalize / k_gn_apply_fin / k_gn_fold
C32_TWO = 4.0                         # two-pass: k_gn_small, k_layernorm
C32_GEMM = 8.0                        # the folded LayerNorm -> GEMM: fp32 accumulation over K of uncentred rows, ln_parts finish
GN_DIMS = ("sample", "pixel", "channel")


def unit_roundoff(dt):
    return 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11


def q16(t, dt):
    """Round to the storage dtype; float32 holding exactly the 16-bit values."""
    return t.to(dt).float()


def k_of(dt, silu=False):
    """k of check_bound: the fp32 roundings of the affine part (and the fast SiLU) in units of the storage type's u."""
    return (K32 + (K32_SILU if silu else 0.0)) * U32 / unit_roundoff(dt)


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def silu64(t):
    return t * torch.sigmoid(t)


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------
def gn_stats(x, G, eps):
    """x [B, HW, C] -> (mean, var, rstd, kappa), float64 [B, G]."""
    B, HW, C = x.shape
    v = x.double().reshape(B, HW, G, C // G)
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    kappa = (mean * mean + var) / (var + eps)
    return mean, var, rstd, kappa


def gn_ref(x, G, gamma, beta, eps, silu, one_pass, c32=None):
    """x [B, HW, C] (exact 16-bit values).  Returns (ref, bound, tiny) float64 [B, HW, C]: tiny is the fp32 term of the module
    docstring for a one-pass or a two-pass path."""
    B, HW, C = x.shape
    cpg = C // G
    mean, var, rstd, kappa = gn_stats(x, G, eps)
    per_c = lambda t: t.repeat_interleave(cpg, dim=1)[:, None, :]           # [B, G] -> [B, 1, C]
    g, b = gamma.double()[None, None, :], beta.double()[None, None, :]
    xh = (x.double() - per_c(mean)) * per_c(rstd)
    u = xh * g + b
    bound = (xh * g).abs() + b.abs()
    tiny = per_c(kappa.sqrt()) * g.abs()
    if one_pass:
        tiny = tiny + per_c(kappa) * (xh * g).abs()
    tiny = tiny * ((C32_ONE if one_pass else C32_TWO) if c32 is None else c32) * U32
    if silu:
        return silu64(u), bound * SILU_SUP, tiny * SILU_SUP
    return u, bound, tiny


def half_ulp(t, dt):
    """Half the spacing of the storage type at |t| (subnormal spacing below the smallest normal)."""
    bits, emin = (8, -126) if dt == torch.bfloat16 else (11, -14)
    e = torch.frexp(t.double().abs().clamp_min(2.0 ** emin))[1] - 1          # floor(log2 |t|)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - bits)


def fp32_floor(name, got, ref, bound, tiny, k, dt):
    """What a stored result still tells about the fp32 error behind it.  The value before the store lies within half an ulp of
    `got`, so max(|got - ref| - half_ulp(got), 0) is a LOWER bound of the device's fp32 error; printed (`[fp32]`) as a ratio to the
    tolerance without its u |ref| term, the quantity the host emulation keeps <= 0.5.  A value above 1 means the device's fp32 part
    is more than twice the emulation's allowance: a finding.  (The full error cannot be read from a rounded output; the host
    emulation, which sees the value before the store, is where the factor-2 room is set.)"""
    g, r = got.double().cpu(), ref.double().cpu()
    low = ((g - r).abs() - half_ulp(g, dt)).clamp_min(0.0)
    tol = k * unit_roundoff(dt) * bound.double().cpu() + (tiny.double().cpu() if torch.is_tensor(tiny) else tiny)
    worst = float((low / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    print(f"[fp32] {name}: device fp32 part >= {worst:.3g} of its allowance")
    return worst


def gn_check(name, got, x, G, gamma, beta, eps, silu, one_pass, dt, enforce=True, c32=None):
    """One sample at a time (the float64 tensors of a whole large batch need not exist at once); the worst ratio."""
    worst = 0.0
    for b in range(x.shape[0]):
        ref, bound, tiny = gn_ref(x[b:b + 1], G, gamma, beta, eps, silu, one_pass, c32)
        worst = max(worst, gpu_util.check_bound(f"{name} sample {b}", got[b:b + 1], ref, bound, k=k_of(dt, silu), tiny=tiny,
                                                dims=GN_DIMS, hdt=dt, enforce=enforce))
        if enforce:
            fp32_floor(f"{name} sample {b}", got[b:b + 1], ref, bound, tiny, k_of(dt, silu), dt)
    return worst


def fp32_ratio(got32, ref, bound, tiny, k, dt):
    """Worst |got32 - ref| / (k u bound + tiny) of a result BEFORE its rounding to 16 bits: the tolerance without the u |ref| term,
    i.e. the part of the error model that K32 and C32_* govern (host emulations only)."""
    tol = k * unit_roundoff(dt) * bound.double() + tiny
    return float(((got32.double() - ref).abs() / tol.clamp_min(1e-300)).max())


def rel_l2(a, b):
    return gpu_util.rel_l2(a, b)


def gn_inputs(B, HW, C, G, dt, mean_sigma=0.3, seed=0, first=None):
    """x [B, HW, C] in 16-bit values: every sample has its own scale (0.3 ... 2) and its own mean (-1 ... 1 in units of its scale),
    every group a further offset of about half a sigma, and the LAST sample sits at mean_sigma standard deviations (sample 0 at
    `first` sigma when given: the 64 sigma family).  gamma = 0.5 + rand, beta = 0.2 randn."""
    cpg = C // G
    x = randn(B, HW, C, seed=seed + 1)
    scale = torch.linspace(2.0, 0.3, B) if B > 1 else torch.tensor([1.5])
    m = torch.linspace(-1.0, 1.0, B) if B > 1 else torch.tensor([0.0])
    m[B - 1] = mean_sigma
    if first is not None:
        m[0] = first
    goff = (0.5 * randn(B, G, seed=seed + 2)).repeat_interleave(cpg, dim=1)
    x = (x + goff[:, None, :] + m[:, None, None]) * scale[:, None, None]
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 3))
    beta = 0.2 * randn(C, seed=seed + 4)
    return q16(x, dt), gamma, beta


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm folded into the consuming Linear: weights and bias
# ---------------------------------------------------------------------------------------------------------------------------
def fold_ref(x, G, gamma, beta, eps, W, bias):
    """Returns (Wf_ref [B, N, C], Wf_tiny, bf_ref [B, N], bf_tol): Wf is checked with check_bound (bound = |Wf_ref|, tiny = Wf_tiny),
    bf (fp32) against bf_tol alone."""
    B, HW, C = x.shape
    cpg = C // G
    mean, var, rstd, kappa = gn_stats(x, G, eps)
    per_c = lambda t: t.repeat_interleave(cpg, dim=1)                        # [B, C]
    a = per_c(rstd) * gamma.double()[None, :]
    s = beta.double()[None, :] - per_c(mean) * a
    Wd = W.double()
    wf = Wd[None, :, :] * a[:, None, :]
    wf_tiny = C32_ONE * U32 * per_c(kappa)[:, None, :] * wf.abs()
    bf = s @ Wd.T + (bias.double()[None, :] if bias is not None else 0.0)
    bf_tol = C32_ONE * U32 * (((beta.double().abs()[None, :] + (per_c(mean) * a).abs()) * (1.0 + per_c(kappa))) @ Wd.abs().T)
    return wf, wf_tiny, bf, bf_tol


def check_abs(name, got, ref, tol, enforce=True):
    """|got - ref| <= tol element-wise for a quantity that is never rounded to 16 bits; prints and returns the worst ratio."""
    g, r, t = got.double().cpu(), ref.double().cpu(), tol.double().cpu()
    ratio = ((g - r).abs() / t.clamp_min(1e-300)).nan_to_num(nan=float("inf"))
    flat = int(ratio.flatten().argmax())
    worst = float(ratio.flatten()[flat])
    print(f"[bound] {name}: worst ratio {worst:.3g} at flat index {flat}: got {float(g.flatten()[flat]):.8g} "
          f"ref {float(r.flatten()[flat]):.8g} tol {float(t.flatten()[flat]):.3g}")
    assert worst <= 1.0 or not enforce, f"{name}: |got - ref| exceeds its fp32 tolerance by {worst:.3g}x"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm and the folded LayerNorm -> GEMM
# ---------------------------------------------------------------------------------------------------------------------------
def ln_stats(x, eps):
    """x [M, C] -> (mean, var, rstd, kappa) float64 [M, 1]."""
    v = x.double()
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    return mean, var, 1.0 / torch.sqrt(var + eps), (mean * mean + var) / (var + eps)


def ln_ref(x, gamma, beta, eps, c32=None):
    """(ref, bound, tiny) [M, C] of k_layernorm (two-pass)."""
    mean, var, rstd, kappa = ln_stats(x, eps)
    g, b = gamma.double()[None, :], beta.double()[None, :]
    xh = (x.double() - mean) * rstd
    return xh * g + b, (xh * g).abs() + b.abs(), (C32_TWO if c32 is None else c32) * U32 * kappa.sqrt() * g.abs()


def ln_inputs(M, C, dt, seed=0, sigmas=(0.0, 8.0, 64.0)):
    """Rows with means from -1 to 1 (units of the row's scale) plus, cycling over the rows, one of `sigmas`; scales 0.3 ... 2."""
    x = randn(M, C, seed=seed + 1)
    scale = torch.linspace(0.3, 2.0, M) if M > 1 else torch.tensor([1.0])
    m = (torch.linspace(-1.0, 1.0, M) if M > 1 else torch.tensor([0.0])) + torch.tensor([sigmas[i % len(sigmas)] for i in range(M)])
    x = (x + m[:, None]) * scale[:, None]
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 3))
    beta = 0.2 * randn(C, seed=seed + 4)
    return q16(x, dt), gamma, beta


def ln_linear_ref(x, gamma, beta, eps, W, bias, from_parts, c32=None):
    """(ref, bound, tiny) [M, N] of the folded LayerNorm -> Linear; from_parts: statistics finished from one-pass row partials."""
    mean, var, rstd, kappa = ln_stats(x, eps)
    g, b, Wd = gamma.double()[None, :], beta.double()[None, :], W.double()
    xh = (x.double() - mean) * rstd
    ref = (xh * g + b) @ Wd.T
    bound = ((xh * g).abs() + b.abs()) @ Wd.abs().T
    if bias is not None:
        ref, bound = ref + bias.double()[None, :], bound + bias.double().abs()[None, :]
    gw = (g * Wd).abs().sum(1)[None, :]                                     # sum_k |gamma_k W_k| per output column
    cond = kappa + kappa.sqrt() if from_parts else kappa.sqrt()
    return ref, bound, (C32_GEMM if c32 is None else c32) * U32 * cond * gw


def k_ln_linear(dt):
    return K_LN_LINEAR + k_of(dt)


def gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
