"""Float64 references and exact-lattice data for the GEMM / implicit-GEMM convolution kernels (csrc/kernels_gemm*.hip,
kernels_conv_out.hip).  CPU only: no GPU import.

The reference is a GATHER: a convolution is turned into the [M][9 Cin] operand the kernels walk (tap-major: K index = tap * Cin + c,
tap = 3 ky + kx) by the index arithmetic of the kernels' own documentation - zero or circular padding, stride, the nearest 2x
upsample with its optional crop - and then multiplied in float64.  tests/test_gemm_ref_host.py checks it against independent ATen
formulations (F.conv2d, F.pad(mode="circular"), F.interpolate + crop, torch.cat, a separate 1x1 convolution).

Three kinds of data ("What the exact lattice proves"):
  lattice   small integers, sparse, such that every fp32 partial sum is an integer far below 2^24 (exact in ANY order) and the final
            value - bias, row bias and residual included - is an integer of magnitude <= 256: representable in bf16 and in fp16.  The
            kernel output must equal it bit for bit whatever the tile, split factor, ring depth or weight layout.
  wide      activations with a full 8-bit significand (odd integers 129 .. 255, signed, times 2^-7), weights 0 / +-2^-j (j <= 4):
            accumulation is still exact, the result is NOT representable: the output must equal ONE round-to-nearest-even of the
            exact value.  Sees lost low operand bits and double rounding, which the plain lattice cannot.
  gauss     Gaussian data judged element-wise by gpu_util.check_bound against the float64 value and its absolute-value form, with
            the DERIVED constant gauss_k(): first-order worst case of an fp32 sum of K products in any order, (K - 1) 2^-24 sum|a||w|,
            allowed twice (the MFMA's internal adder tree is undocumented; the factor also covers the <= 3 epilogue adds).
"""
import math

import numpy as np
import torch

F64 = torch.float64
GELU_DERIV_MAX = 1.13          # max |d gelu / dx| (1.1289 at x = sqrt(2))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_f_np(x):
    """Transcription of gelu_erf_f (csrc/common.h) into numpy float32, operation by operation (fmaf = one rounding: done in float64
    and rounded once, exact because a product of two float32 has 48 bits).  The hardware reciprocal (1 ulp) is an exact division here."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    z = (np.abs(x) * f32(0.70710678118654752)).astype(f32)
    p = fma(z, np.full_like(z, f32(0.0000430638)), np.full_like(z, f32(0.0002765672)))
    for c in (0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784, 1.0):
        p = fma(z, p, np.full_like(z, f32(c)))
    with np.errstate(over="ignore"):
        for _ in range(4):
            p = (p * p).astype(f32)
    with np.errstate(divide="ignore"):
        q = (f32(1.0) / p).astype(f32)
    return fma((f32(-0.70710678118654752) * z).astype(f32), q, np.maximum(x, f32(0.0)))


# Measured by tests/test_gemm_ref_host.py::test_gelu_transcription over [-12, 12] (step 2^-10): max |gelu_erf_f - gelu| of the float32
# transcription against float64 erf-GELU.  The GEGLU tolerance term is twice this, times |value|.
GELU_ABS_ERR = 6.95e-7


def gauss_k(K, hdt):
    """k of check_bound for an fp32 sum of K products: k u bound = 2 (K 2^-24) bound."""
    u = 2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -11
    return K * 2.0 ** -23 / u


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def conv_out_size(Hi, Wi, stride=1, pad=1, ups=0, Hup=0, Wup=0):
    Hin = (Hup or 2 * Hi) if ups else Hi
    Win = (Wup or 2 * Wi) if ups else Wi
    extra = 2 if pad else 1            # pad = 0 is the asymmetric (0, 1, 0, 1) pad: one zero row below, one zero column right
    return (Hin + extra - 3) // stride + 1, (Win + extra - 3) // stride + 1


def _axis(n_out, n_src, stride, pad, ups, lim_up, wrap, k, bug=None):
    """Source index and validity of tap offset k along one axis for every output position."""
    lim = (lim_up or 2 * n_src) if ups else n_src
    if bug == "crop_ignored" and ups:
        lim = 2 * n_src
    o = torch.arange(n_out)
    i = o * stride - pad + k
    if bug == "asym_wrong_side":
        i = i - 1
    if wrap:
        if bug == "wrap_one_side":
            i = torch.where(i < 0, i + lim, i)
        else:
            i = torch.where(i < 0, i + lim, torch.where((i >= lim) & (i < 2 * lim), i - lim, i))
    ok = (i >= 0) & (i < (lim + 1 if bug == "right_edge" else lim))
    if ups:
        i = (i + 1) // 2 if bug == "ups_round_up" else i // 2
    return i.clamp(0, n_src - 1), ok


def conv_gather(x, stride=1, pad=1, ups=0, Hup=0, Wup=0, wrap=0, bug=None):
    """x [B][Hi][Wi][C] -> the implicit-GEMM A operand [B * Ho * Wo][9][C] (same dtype)."""
    B, Hi, Wi, C = x.shape
    Ho, Wo = conv_out_size(Hi, Wi, stride, pad, ups, Hup, Wup)
    taps = []
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        if bug == "kykx":
            ky, kx = kx, ky
        iy, oky = _axis(Ho, Hi, stride, pad, ups, Hup, wrap & 2, ky, bug if bug in ("crop_ignored", "ups_round_up", "asym_wrong_side") else None)
        ix, okx = _axis(Wo, Wi, stride, pad, ups, Wup, wrap & 1, kx, bug)
        g = x[:, iy][:, :, ix]                                          # [B][Ho][Wo][C]
        m = (oky[:, None] & okx[None, :]).to(x.dtype)[None, :, :, None]
        taps.append(g * m)
    return torch.stack(taps, dim=3).reshape(B * Ho * Wo, 9, C)


def two_sources(a, a2):
    """The kernels split K (linear) or the channel axis (conv) at C1 = width of the first source."""
    return a if a2 is None else torch.cat([a, a2], dim=-1)


def reference(A, W, bias=None, rowbias=None, rows_per_sample=1, residual=None, geglu=False):
    """A [M][K], W [N][K] (GEGLU: [2 N] rows, value rows first, gate rows second - the diffusers order), everything float64.
    Returns (value, bound): out = A W^T + bias + rowbias[row / rows_per_sample] + residual, bound = the absolute-value form;
    GEGLU: value * gelu(gate) with bound |gelu(g)| bound_v + 1.13 |v| bound_g."""
    A, W = A.to(F64), W.to(F64)
    v = A @ W.T
    b = A.abs() @ W.abs().T
    if bias is not None:
        v, b = v + bias.to(F64), b + bias.to(F64).abs()
    if rowbias is not None:
        rb = rowbias.to(F64).repeat_interleave(rows_per_sample, dim=0)
        v, b = v + rb, b + rb.abs()
    if geglu:
        n = v.shape[1] // 2
        val, gate, bv, bg = v[:, :n], v[:, n:], b[:, :n], b[:, n:]
        return val * gelu64(gate), gelu64(gate).abs() * bv + GELU_DERIV_MAX * val.abs() * bg
    if residual is not None:
        v, b = v + residual.to(F64), b + residual.to(F64).abs()
    return v, b


def geglu_value_abs(A, W, bias):
    """|value| of a GEGLU problem: the factor of gelu_erf_f's own approximation error in the tolerance."""
    n = W.shape[0] // 2
    v = A.to(F64) @ W[:n].to(F64).T
    return (v + bias[:n].to(F64)).abs() if bias is not None else v.abs()


def geglu_interleave(w):
    """[2 N][...] value rows | gate rows -> the kernels' order: 16 value rows, their 16 gate rows, ... (gyre_op_repack_linear_weight)."""
    n = w.shape[0] // 2
    assert n % 16 == 0
    v, g = w[:n].reshape(n // 16, 16, *w.shape[1:]), w[n:].reshape(n // 16, 16, *w.shape[1:])
    return torch.cat([v, g], dim=1).reshape(w.shape)


def transposed(y, tokens, ldt, fill):
    """[B * tokens][N] -> [B][N][ldt] with the pad columns holding `fill`."""
    M, N = y.shape
    B = M // tokens
    out = torch.full((B, N, ldt), fill, dtype=y.dtype)
    out[:, :, :tokens] = y.reshape(B, tokens, N).permute(0, 2, 1)
    return out


def nchw(y, B, Ho, Wo):
    return y.reshape(B, Ho, Wo, -1).permute(0, 3, 1, 2).contiguous()


def colstats(y, rows, unit):
    """[M / rows][N / unit][2]: sum and sum of squares of the stored outputs per row block and channel unit."""
    M, N = y.shape
    t = y.to(F64).reshape(M // rows, rows, N // unit, unit)
    return torch.stack([t.sum(dim=(1, 3)), (t * t).sum(dim=(1, 3))], dim=-1)


def rowstats(y, bn):
    """[tiles_n][M][2]: per row the sum and sum of squares of the stored outputs of every bn-wide N tile."""
    M, N = y.shape
    parts = []
    for n0 in range(0, N, bn):
        t = y[:, n0:n0 + bn].to(F64)
        parts.append(torch.stack([t.sum(1), (t * t).sum(1)], dim=-1))
    return torch.stack(parts, dim=0)


# ---- data ----------------------------------------------------------------------------------------------------------------------
LATTICE_MAX = 256            # integers up to here are bf16 values (8-bit significand) and fp16 values (11 bits)
STAT_MAX = 32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sparse_int(shape, mags, density, g):
    mag = torch.tensor(mags, dtype=F64)[torch.randint(0, len(mags), shape, generator=g)]
    sign = torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1
    keep = (torch.rand(shape, generator=g, dtype=F64) < density).to(F64)
    return mag * sign * keep


def lattice_density(K, target):
    """Density of each operand such that an output sees about `target` non-zero products of K (1: dense)."""
    return min(1.0, math.sqrt(target / K))


def lattice_operands(kind, a_shape, w_shape, K, seed):
    """Operands of one source / one weight matrix.  kind: 'lattice' (a in +-{1,2,3}, w in +-{1,2}, ~64 products per output: sigma
    of the sum 27), 'stat' (a, w in +-1, ~9 products: sigma 3), 'wide' (a = +-odd(129..255) 2^-7, w = +-2^-j, j <= 4, ~48 products)."""
    g = _gen(seed)
    if kind == "wide":
        d = lattice_density(K, 48)
        odd = (torch.randint(64, 128, a_shape, generator=g).to(F64) * 2 + 1) / 128.0
        sign = torch.randint(0, 2, a_shape, generator=g).to(F64) * 2 - 1
        a = odd * sign * (torch.rand(a_shape, generator=g, dtype=F64) < d).to(F64)
        w = _sparse_int(w_shape, [1.0, 0.5, 0.25, 0.125, 0.0625], d, g)
        return a, w
    if kind == "stat":
        d = lattice_density(K, 9)
        return _sparse_int(a_shape, [1.0], d, g), _sparse_int(w_shape, [1.0], d, g)
    d = lattice_density(K, 64)
    return _sparse_int(a_shape, [1.0, 2.0, 3.0], d, g), _sparse_int(w_shape, [1.0, 2.0], d, g)


def lattice_addend(kind, shape, seed, scale=1.0):
    """Bias / row bias / residual on the lattice: integers within +-32 (lattice; row bias +-16), +-4 (stat); wide: 8-bit
    significands like the activations (a residual is a stored 16-bit value)."""
    g = _gen(seed)
    if kind == "wide":
        odd = (torch.randint(64, 128, shape, generator=g).to(F64) * 2 + 1) / 128.0
        return odd * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1) * 4.0
    r = int((4 if kind == "stat" else 32) * scale)
    return torch.randint(-r, r + 1, shape, generator=g).to(F64)


def gauss_operands(a_shape, w_shape, K, seed, hdt):
    g = _gen(seed)
    a = torch.randn(a_shape, generator=g).to(hdt).to(F64)
    w = (torch.randn(w_shape, generator=g) / math.sqrt(K)).to(hdt).to(F64)
    return a, w


def gauss_addend(shape, seed, hdt=None):
    t = torch.randn(shape, generator=_gen(seed))
    return (t.to(hdt) if hdt is not None else t).to(F64)


def assert_lattice(kind, exact, partial_abs=None, sumsq=None):
    """The conditions under which the kernel output must be bit-exact: asserted, never clamped."""
    m = float(exact.abs().max())
    if kind == "wide":
        # exact accumulation: every partial sum is a multiple of 2^-11 (2^-7 x 2^-4) below 2^13, i.e. fits 24 bits
        assert partial_abs is not None and float(partial_abs.max()) < 2.0 ** 13, float(partial_abs.max())
        assert bool((exact * 2048 == (exact * 2048).round()).all())
        return
    lim = STAT_MAX if kind == "stat" else LATTICE_MAX
    assert m <= lim, f"lattice overflow: max |exact| = {m} > {lim}"
    assert bool((exact == exact.round()).all())
    if partial_abs is not None:
        assert float(partial_abs.max()) < 2.0 ** 24
    if sumsq is not None:
        assert float(sumsq) < 2.0 ** 24, float(sumsq)


def rne(exact, hdt):
    """ONE round-to-nearest-even of an exact float64 value that fits float32 (<= 24 significant bits) to the storage type."""
    f = exact.to(torch.float32)
    assert bool((f.to(F64) == exact).all()), "value does not fit float32: the rounding below would be a double rounding"
    return f.to(hdt)


# ---- fp32 emulation of a correct kernel (host self-test) ------------------------------------------------------------------------
def emulate_fp32(A, W, bias=None, rowbias=None, rows_per_sample=1, residual=None, geglu=False, chunk=64, conv_cin=0, splits=1,
                 bug=None, tile_n=64):
    """fp32 accumulation in the kernels' order: K in 64-wide chunks (a convolution with whole 64-channel chunks: chunk outer, tap
    inner - the uniform-tap order; else K linear), each chunk two 32-wide MFMA steps whose dot product is formed exactly and added to
    the fp32 accumulator with one rounding; split K: slabs summed in order; then bias, row bias, (GEGLU,) residual in fp32.  Returns
    the fp32 value BEFORE the store.  A [M][K] (conv: tap-major K), W [N][K] float64 holding storage values (GEGLU: value | gate rows).
    bug: a seeded mistake (tests/test_gemm_ref_host.py)."""
    f32 = torch.float32
    M, K = A.shape
    N = W.shape[0]
    if conv_cin and conv_cin % chunk == 0:
        order = [(t * conv_cin + c0, t * conv_cin + c0 + chunk) for c0 in range(0, conv_cin, chunk) for t in range(K // conv_cin)]
    else:
        order = [(k0, min(K, k0 + chunk)) for k0 in range(0, K, chunk)]
    if bug == "k_tail":
        order = [(a, b) for a, b in order if b - a == chunk]
    per = (len(order) + splits - 1) // splits
    slabs = []
    for s in range(splits):
        acc = torch.zeros(M, N, dtype=f32)
        for ci, (k0, k1) in enumerate(order[s * per:(s + 1) * per]):
            for h0 in range(k0, k1, 32):
                h1 = min(k1, h0 + 32)
                part = A[:, h0:h1] @ W[:, h0:h1].T                                    # exact enough: float64 dot of <= 32 products
                if bug == "last_chunk_col" and s == splits - 1 and (k0, k1) == order[-1]:
                    part = part.clone(); part[:, N - tile_n:] = 0
                acc = (acc.to(F64) + part).to(f32)
        slabs.append(acc)
    if bug == "slab":
        slabs = slabs[:-1]
    acc = slabs[0]
    for s in slabs[1:]:
        acc = acc + s
    if bug == "one_product":
        acc = acc.clone()
        m, n = M // 2, N // 2
        ks = torch.nonzero(A[m] * W[n])
        k = int(ks[0]) if len(ks) else 0
        acc[m, n] = (acc[m, n].to(F64) - A[m, k] * W[n, k]).to(f32)
    if bias is not None:
        bb = bias.to(f32)
        if bug == "bias_shift":
            bb = bb.clone(); bb[N - tile_n:] = torch.roll(bb[N - tile_n:], 4)
        acc = acc + bb
    if rowbias is not None:
        rps = rows_per_sample
        rb = rowbias.to(f32).repeat_interleave(rps, dim=0)
        if bug == "sample_boundary":                # every row of a 64-row tile takes the sample of the tile's first row
            idx = (torch.arange(M) // 64 * 64) // rps
            rb = rowbias.to(f32)[idx]
        acc = acc + rb
    if geglu:
        n = N // 2
        val, gate = acc[:, :n], acc[:, n:]
        if bug == "pairing":
            gate = torch.roll(gate, 16, dims=1)
        if bug == "tanh_gelu":
            gl = torch.nn.functional.gelu(gate, approximate="tanh")
        else:
            gl = torch.from_numpy(gelu_erf_f_np(gate.numpy()))
        acc = val * gl
    if residual is not None:
        r = residual.to(f32)
        acc = acc + r
    return acc


# ---- one row of tests/gemm_cases.py -> operands in the kernels' layouts and the expected result -----------------------------------
PLAN_FIELDS = ("cfg", "splits", "ws_lo", "ws_hi", "w_block", "colstat_rows", "rowstat_parts", "ln_fold", "per_sample_w", "shortcut_fold",
               "nst", "uni")
PAD_POISON = 5.0             # pad columns of the operands hold this (a stray read changes an integer); output pads hold CANARY
CANARY = -3.0
CANARY_ROWS = 4


class Case:
    pass


def _padded(t, pad, fill=PAD_POISON):
    """[rows][w] -> [rows][w + pad] with the pad columns holding `fill`."""
    if not pad:
        return t.contiguous()
    out = torch.full(t.shape[:-1] + (t.shape[-1] + pad,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def make_operands(kind, hdt, a_shape, w_shape, M, N, K, rps, seed, geglu=False, bias=True, rowbias=False, res=False, Ktot=None):
    """The data of one problem, float64 holding storage values: (a, w, bias, rowbias, residual) with w / bias in the reference's row
    order (GEGLU: value rows | gate rows).  The one generator behind the case table and the host self-test.
    GEGLU lattice: zero gate weights, gate bias 0 or 16 per column (gelu_erf_f gives exactly 0 and 16), values within +-16."""
    Ktot = Ktot or K
    Nw = w_shape[0]
    if kind == "gauss":
        a, w = gauss_operands(a_shape, w_shape, Ktot, seed, hdt)
        add = lambda shape, sd, rnd=False, scale=1.0: gauss_addend(shape, sd, hdt if rnd else None)
    else:
        a, w = lattice_operands(kind, a_shape, w_shape, Ktot, seed)
        add = lambda shape, sd, rnd=False, scale=1.0: lattice_addend(kind, shape, sd, scale)
    b = add((Nw,), seed + 1) if bias else None
    if geglu and kind != "gauss":
        g = _gen(seed + 5)
        d = lattice_density(K, 6)                    # sigma of the value 2.5: +-14 is 5.7 sigma
        w = torch.cat([_sparse_int((N,) + tuple(w_shape[1:]), [1.0], d, g), torch.zeros((N,) + tuple(w_shape[1:]), dtype=F64)])
        a = _sparse_int(a_shape, [1.0], d, g)
        b = torch.cat([torch.randint(-2, 3, (N,), generator=g).to(F64), torch.randint(0, 2, (N,), generator=g).to(F64) * 16.0])
    if geglu and kind == "gauss":
        # Generic gates whose size comes mostly from the bias: the gate's share of the tolerance is 1.13 |v| K 2^-23 (sum|a||w| + |bias|),
        # and with unit-variance operands sum|a||w| ~ 0.64 sqrt(K) |gate|: from K = 320 on that allowance alone reaches the 4e-4 |v| by
        # which a tanh-GELU differs from the erf form around gate = -3 (host self-test, seeded mistake).  Gate weights a quarter the
        # size (exact in both storage types) keep every mantissa bit in play and leave the rows able to tell the two apart.
        w = w.clone(); w[N:] *= 0.25
        b = b.clone(); b[N:] *= 1.5
    rb = add((M // rps, N), seed + 2, scale=0.5) if rowbias else None
    rs = add((M, N), seed + 3, rnd=True) if res else None
    return a, w, b, rb, rs


def case_shapes(r):
    """Sizes, strides and which operands a row has - everything gyre_gemm_test_args needs, no data."""
    s, f = r["shape"], r["feats"]
    op = r["op"]
    conv = op in ("conv", "conv_nchw", "colstats_conv", "shortcut")
    c = Case()
    c.row, c.conv, c.geglu = r, conv, bool(f.get("geglu"))
    if conv:
        B, H, W, Cin, N = s["B"], s["H"], s["W"], s["Cin"], s["Cout"]
        c.geom = dict(stride=f.get("stride", 1), pad=f.get("pad", 1), ups=f.get("ups", 0), wrap=f.get("wrap", 0),
                      Hup=2 * H - 1 if f.get("crop") else 0, Wup=2 * W - 1 if f.get("crop") else 0)
        c.Ho, c.Wo = conv_out_size(H, W, c.geom["stride"], c.geom["pad"], c.geom["ups"], c.geom["Hup"], c.geom["Wup"])
        M, K, width, c.a_shape = B * c.Ho * c.Wo, 9 * Cin, Cin, (B, H, W, Cin)
        c.rps = c.Ho * c.Wo
    else:
        M, K, N = s["M"], s["K"], s["N"]
        width, c.a_shape = K, (M, K)
        c.rps = f.get("rps", 1)
    c.sc_C1, c.sc_K = f.get("C1s", 0), f.get("C1s", 0) + f.get("C2s", 0)
    c.M, c.K, c.N, c.Nw, c.Ktot, c.width = M, K, N, 2 * N if c.geglu else N, K + c.sc_K, width
    c.w_shape = (c.Nw, 9, Cin) if conv else (c.Nw, K)
    c.C1 = f.get("C1", 0)
    c.lda = (c.C1 or width) + f.get("lda_pad", 0)
    c.lda2 = width - c.C1 + f.get("lda2_pad", 0) if c.C1 else 0
    c.has_bias, c.has_rowbias, c.has_res = bool(f.get("bias")), bool(f.get("rowbias")), bool(f.get("res"))
    c.ld_rowbias, c.ldr, c.ldc = N + 4, N + f.get("ldr_pad", 0), N + f.get("ldc_pad", 0)
    return c


def build_case(r, hdt):
    """Operands (float64 holding storage values, in the kernels' layouts and strides), the float64 value and - for Gaussian rows -
    its absolute-value bound; lattice rows assert their conditions here (assert_lattice)."""
    f, kind = r["feats"], r["kind"]
    seed = (sum(ord(ch) * (i + 1) for i, ch in enumerate(r["id"])) % 100000) * 10
    c = case_shapes(r)
    conv, M, K, N, Nw, Ktot, sc_K = c.conv, c.M, c.K, c.N, c.Nw, c.Ktot, c.sc_K
    a, wv, bias, rowbias, residual = make_operands(kind, hdt, c.a_shape, c.w_shape, M, N, K, c.rps, seed, c.geglu, c.has_bias, c.has_rowbias,
                                                   c.has_res, Ktot)
    # the A operand as the kernels gather it
    A = conv_gather(a, **c.geom).reshape(M, K) if conv else a
    Wm = wv.reshape(Nw, K)
    if sc_K:
        sA, sW, c.bias_sc, _, _ = make_operands(kind, hdt, (M, sc_K), (Nw, sc_K), M, N, sc_K, c.rps, seed + 7, Ktot=Ktot)
        c.sc, c.w_sc = sA, sW
        A, Wm = torch.cat([A, sA], dim=1), torch.cat([Wm, sW], dim=1)
        bias_all = c.bias_sc if bias is None else bias + c.bias_sc
    else:
        bias_all = bias
    big = kind != "gauss" and M * Ktot * Nw > 2e9       # lattice data: float32 is exact too and the large rows are cheaper in it
    if big:
        v = (A.float() @ Wm.float().T).to(F64)
        if bias_all is not None:
            v = v + bias_all
        if rowbias is not None:
            v = v + rowbias.repeat_interleave(c.rps, dim=0)
        if residual is not None:
            v = v + residual
        bound = None
    else:
        v, bound = reference(A, Wm, bias_all, rowbias, c.rps, residual, c.geglu)
    c.value, c.bound = v, bound
    if kind != "gauss":
        partial = A.abs().sum(1).max() * Wm.abs().max() + 64 if bound is None else bound
        if c.geglu:
            assert bool(((v == 0) | (v.abs() <= 256)).all()) and float(geglu_value_abs(A, Wm, bias_all).max()) <= 16
            assert_lattice("lattice", v, partial)
        else:
            assert_lattice(kind, v, partial)
    else:
        c.k = gauss_k(Ktot, hdt)
        c.tiny = 2 * GELU_ABS_ERR * geglu_value_abs(A, Wm, bias_all) if c.geglu else 0.0
    # operands in the kernels' layouts
    C1 = c.C1
    src = a.reshape(-1, c.width)
    c.a1 = _padded(src[:, :C1] if C1 else src, f.get("lda_pad", 0))
    c.a2 = _padded(src[:, C1:], f.get("lda2_pad", 0)) if C1 else None
    c.w = geglu_interleave(wv.reshape(Nw, -1)) if c.geglu else wv.reshape(Nw, -1)
    c.bias = None if bias is None else (geglu_interleave(bias) if c.geglu else bias)
    c.rowbias = None if rowbias is None else _padded(rowbias, 4)
    c.residual = None if residual is None else _padded(residual, f.get("ldr_pad", 0))
    assert c.a1.shape[-1] == c.lda and (c.a2 is None or c.a2.shape[-1] == c.lda2)
    assert (c.rowbias is None or c.rowbias.shape[-1] == c.ld_rowbias) and (c.residual is None or c.residual.shape[-1] == c.ldr)
    return c


def expected_store(c, hdt):
    """The stored value of a lattice / wide row: the exact value is representable (lattice) or rounded ONCE (wide)."""
    return rne(c.value, hdt)


def gemm_test_args(c, ptr=None, out_ptr=0, ws=(0, 0)):
    """gyre_gemm_test_args of a row from its shapes (case_shapes / build_case).  ptr: name -> device address (a1, a2, w, bias, rowbias,
    residual, sc1, sc2); None: the plan query's stand-ins (aligned non-null values where the row has the operand - the query looks
    at NULL-ness and alignment only)."""
    from gyre_amd import _lib
    r = c.row
    f, s = r["feats"], r["shape"]
    fake = ptr is None
    ptr = ptr or {k: 4096 for k in ("a1", "a2", "w", "bias", "rowbias", "residual", "sc1", "sc2")}
    a = _lib.GemmTestArgs()
    a.conv = 1 if c.conv else 0
    a.N, a.geglu = c.N, int(c.geglu)
    if c.conv:
        a.B, a.Hi, a.Wi, a.Cin = s["B"], s["H"], s["W"], s["Cin"]
        g = c.geom
        a.stride, a.pad, a.ups, a.Hup, a.Wup, a.wrap = g["stride"], g["pad"], g["ups"], g["Hup"], g["Wup"], g["wrap"]
    else:
        a.M, a.K = c.M, c.K
        a.rows_per_sample = c.rps
    a.lda = c.lda
    a.A, a.W = ptr["a1"], ptr["w"]
    if c.C1:
        a.A2, a.C1, a.lda2 = ptr["a2"], c.C1, c.lda2
    if c.has_bias or c.sc_K:
        a.bias = ptr["bias"]
    if c.has_rowbias:
        a.rowbias, a.ld_rowbias = ptr["rowbias"], c.ld_rowbias
    if c.has_res:
        a.residual, a.ldr = ptr["residual"], c.ldr
    a.ldc = c.ldc
    a.out = out_ptr or (4096 + f.get("out_off", 0) if fake else 0)
    if r["op"] == "linear_t":
        a.out_mode, a.tokens, a.ldt = 2, f["tokens"], f["ldt"]
    if r["op"] == "conv_nchw":
        a.out_mode, a.out_dtype = 1, f["dtype"]
    if c.sc_K:
        a.sc_A, a.sc_K = ptr["sc1"], c.sc_K
        if c.sc_C1 < c.sc_K:
            a.sc_A2, a.sc_C1 = ptr["sc2"], c.sc_C1
    a.colstat_unit = f.get("unit", 0)
    a.ws, a.ws_bytes = ws
    return a


def plan_query(L, a):
    import ctypes
    out = (ctypes.c_int32 * 12)()
    rc = L.gyre_debug_gemm_plan(ctypes.byref(a), out)
    return rc, dict(zip(PLAN_FIELDS, list(out)))
