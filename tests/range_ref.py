"""Builders, exponent derivation, judgement and a torch emulation for the range-edge family (tests/range_cases.py).  CPU only.
TEST INFRASTRUCTURE shared by tests/test_range_ref_host.py (CPU) and tests/test_gpu_range.py (-m gpu).

The operations themselves are not restated here: gemm_ref.reference / conv_gather, norm_fwd_ref, attn_fwd_ref, tome_exact_ref and
temb_ref are the float64 references, and their error models are the ones every row is judged with.

Two checks per row.
  1  exact power-of-two scaling.  A power of two commutes with every rounding as long as no value leaves the format, so the SCALED
     run must equal 2^k times the BASE run (the O(1) data the rest of the suite trusts) bit for bit.  Elements whose base or scaled
     float64 reference is below the smallest normal of the storage type are excluded (rounding is absolute there); at most 1 % of
     a row may be (EXCLUDE_CAP, asserted from the reference alone by the host test).  The offset rows (cancel, bias_back,
     rowbias_back, res_order) and the subnormal rows live on the exact lattice of gemm_ref: there the expected value is
     2^k base + offset, nothing is excluded, and check 2 is exactness (one RNE of the float64 value) - the lattice family's own bound.
  2  the float64 reference of the scaled problem under the family's existing element-wise bound; NaN / inf fails.

Exponents (derive_exps).  fp16: the largest k with  max |scaled output| <= 65504, which puts it in (top / 2, top].  bf16 stores in
fp32's exponent range, so its binding limit is the fp32 intermediates: k is the largest with the float64 ABSOLUTE-VALUE form of
the computation (which bounds every partial sum in any order) <= 2^126.  The subnormal rows use fixed exponents: lattice integers
1 .. 3 (x 2^8 for convolutions) times 2^-24 are fp16 subnormals, the other operand is scaled up as far as its format allows so
that the outputs are normal.  On the bf16 flavour those rows run the same numbers, which are ordinary small normals there."""
import copy
import math

import torch

import gemm_ref as G

F64 = torch.float64
NAME = {torch.float16: "f16", torch.bfloat16: "bf16"}
TOP = {torch.float16: 65504.0, torch.bfloat16: 2.0 ** 126, torch.float32: 2.0 ** 126}
NORMAL_MIN = {torch.float16: 2.0 ** -14, torch.bfloat16: 2.0 ** -126, torch.float32: 2.0 ** -126}
EXCLUDE_CAP = 0.01
OFFSET_PROPS = ("cancel", "bias_back", "rowbias_back", "res_order")
SUB_PROPS = ("sub_act", "sub_w", "sub_out")
NCHW_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def storage_name(hdt):
    return NAME[hdt]


def rows_for(rows, hdt):
    return [r for r in rows if NAME[hdt] in r["only"]]


def floor_log2(x):
    m, e = math.frexp(x)                    # x = m 2^e, 0.5 <= m < 1
    return e - 1


def k_top(maximum, top):
    """The largest k with maximum * 2^k <= top."""
    k = floor_log2(top / maximum)
    while maximum * 2.0 ** (k + 1) <= top:
        k += 1
    while maximum * 2.0 ** k > top:
        k -= 1
    return k


def representable(t, dt):
    """Every value of t (float64) is a value of dt."""
    return bool((t.to(dt).to(F64) == t).all())


def all_subnormal(t, dt):
    """Every non-zero value is below the smallest normal of dt (and there is a non-zero value)."""
    nz = t[t != 0].abs()
    return nz.numel() > 0 and float(nz.max()) < NORMAL_MIN[dt]


# ---- GEMM / convolution rows ---------------------------------------------------------------------------------------------------------
def _geglu_perm(c):
    """laid-out row i holds reference row perm[i]"""
    return G.geglu_interleave(torch.arange(c.Nw))


def operands(c):
    """(A [M][Ktot] as the kernel gathers it, W [Nw][K], bias, rowbias [samples][N], residual [M][N]) in the REFERENCE's row order,
    from the laid-out operands of a Case (rows of this family carry no padded strides and one source)."""
    f = c.row["feats"]
    assert not any(f.get(k) for k in ("lda_pad", "ldr_pad", "C1", "C1s")), "range rows use dense single-source operands"
    A = G.conv_gather(c.a1.reshape(c.a_shape), **c.geom).reshape(c.M, c.K) if c.conv else c.a1
    W, bias = c.w, c.bias
    if c.geglu:
        perm = _geglu_perm(c)
        W = torch.empty_like(c.w); W[perm] = c.w
        if bias is not None:
            bias = torch.empty_like(c.bias); bias[perm] = c.bias
    rb = None if c.rowbias is None else c.rowbias[:, :c.N]
    return A, W, bias, rb, c.residual


def evaluate(c):
    """value, bound, tiny of a Case from its laid-out operands (gemm_ref.reference)."""
    A, W, bias, rb, res = operands(c)
    c.value, c.bound = G.reference(A, W, bias, rb, c.rps, res, c.geglu)
    c.tiny = 2 * G.GELU_ABS_ERR * G.geglu_value_abs(A, W, bias) if c.geglu else 0.0
    # the largest fp32 intermediate in absolute-value form: the bound itself; GEGLU: the value half before the product
    if c.geglu:
        n = W.shape[0] // 2
        c.inter = A.abs() @ W[:n].abs().T + (bias[:n].abs() if bias is not None else 0.0)
    else:
        c.inter = c.bound
    return c


def injection(row, c):
    """The offset rows: (a_cols {column of a1: value}, w_cols {column of w: value}, addends {operand: value added}, offset of the
    final value).  Convolutions: an a1 column is a channel PLANE (constant over the image), and all nine taps of that channel's
    weights are set (zero where not named), so the injected products depend on nothing but which taps are valid at a pixel."""
    prop, K = row["prop"], c.K
    if prop not in OFFSET_PROPS:
        return {}, {}, {}, 0.0
    if c.conv:
        Cin = c.a_shape[-1]
        taps = lambda ch, vals: {t * Cin + ch: float(vals.get(t, 0.0)) for t in range(9)}
        if prop == "cancel":
            # chunk-major kernels walk channel 0's nine taps first: + 2^15 per valid tap (4 at a corner: 2^17), the last channel
            # takes every one of them back - the same taps are valid for both, at every pixel
            a_cols = {0: 512.0, Cin - 1: 512.0}
            w_cols = {**taps(0, {t: 64.0 for t in range(9)}), **taps(Cin - 1, {t: -64.0 for t in range(9)})}
            return a_cols, w_cols, {}, 0.0
        centre = lambda w: taps(0, {4: w})              # the centre tap is valid at every pixel (stride 1, pad 1)
        if prop == "bias_back":
            return {0: 512.0}, centre(256.0), {"bias": -2.0 ** 17}, 0.0
        if prop == "res_order":
            return {0: 256.0}, centre(128.0), {"bias": 49152.0, "residual": -49152.0}, 2.0 ** 15
        raise KeyError(prop)
    if prop == "cancel":                                # first K step + 2^18, last K step (the K tail; the last split-K slice) - 2^18
        return {0: 512.0, K - 1: 512.0}, {0: 512.0, K - 1: -512.0}, {}, 0.0
    if prop == "bias_back":
        return {0: 512.0}, {0: 256.0}, {"bias": -2.0 ** 17}, 0.0
    if prop == "rowbias_back":
        return {0: 512.0}, {0: 256.0}, {"rowbias": -2.0 ** 17}, 0.0
    # accumulator 2^15 + bias 49152 = 81920 (less the lattice part: beyond the top for all but the odd element), residual -49152
    return {0: 256.0}, {0: 128.0}, {"bias": 49152.0, "residual": -49152.0}, 2.0 ** 15


def gemm_base(row, hdt):
    """The base Case of a gemm / conv row: gemm_ref.build_case of its O(1) problem, with the columns an offset row injects into
    zeroed in A and (GEGLU top rows) gates moved to where gelu is small, then re-evaluated."""
    c = G.build_case(row["base"], hdt)
    if row["op"] == "shortcut":
        # lattice row at the planner's size: the value is build_case's (float32 matmul, exact on the lattice); the absolute-value
        # form is bounded from above by the operand maxima instead of a second 27 GFLOP product
        c.tiny, c.bound = 0.0, c.value.abs()
        amax = lambda t: float(t.abs().max())
        c.inter = torch.tensor(c.K * amax(c.a1) * amax(c.w) + c.sc_K * amax(c.sc) * amax(c.w_sc) + amax(c.bias) + amax(c.bias_sc))
        return c
    a_cols, _, _, _ = injection(row, c)
    if a_cols:
        c.a1 = c.a1.clone()
        c.a1[:, list(a_cols)] = 0.0
    if row["prop"] == "sub_act_gauss":
        c.a1 = quantised(c.a1, hdt, 2.0 ** -6).double()
    if row["prop"] == "sub_w_gauss":
        c.w = quantised(c.w, hdt, 2.0 ** -10).double()
    if row["prop"] == "geglu":
        # gates around -2.5: |gelu(gate)| <= 0.17, so a value half far beyond the top of fp16 still gives a product inside it
        n = c.N
        g = torch.Generator().manual_seed(7)
        gate_bias = (-2.5 + 0.3 * torch.randn(n, generator=g)).to(F64)
        ref_bias = torch.cat([operands(c)[2][:n], gate_bias])
        c.bias = G.geglu_interleave(ref_bias)
        c.w = c.w.to(hdt).to(F64)                       # (make_operands quarters the gate weights after their rounding)
    return evaluate(c)


def derive_exps(row, c0, hdt):
    """(ka, kw) of a gemm / conv row from the float64 reference of its base Case (module docstring)."""
    prop = row["prop"]
    if row["op"] == "shortcut":
        k = k_top(float(c0.value.abs().max()), TOP[hdt]) if hdt == torch.float16 else k_top(float(c0.inter), TOP[hdt])
        return k // 2, k - k // 2
    A, W, _, _, _ = operands(c0)
    if prop == "sub_act":
        s = 8 if c0.conv else 0
        assert float(A.abs().max()) * 2.0 ** (s - 24) < 2.0 ** -14
        return s - 24, k_top(float(W.abs().max()), TOP[torch.float16])
    if prop == "sub_w":
        s = 8 if c0.conv else 0
        return k_top(float(A.abs().max()), TOP[torch.float16]), s - 24
    if prop == "sub_out":
        return -12, -12
    if prop == "sub_act_gauss":                         # A = n 2^-6, |n| <= 1023: x 2^-18 onto the subnormal lattice; weights to their top
        return -18, k_top(float(W.abs().max()), TOP[torch.float16])
    if prop == "sub_w_gauss":                           # W = n 2^-10: x 2^-14; activations to their top
        return k_top(float(A.abs().max()), TOP[torch.float16]), -14
    vmax = float(c0.value.abs().max())
    if row["op"] == "conv_nchw":
        odt = NCHW_DT[row["base"]["feats"]["dtype"]]
        if hdt == torch.bfloat16 and odt == torch.float16:
            k = k_top(vmax, TOP[torch.float16]) + 1     # just past the top: the largest outputs are inf, as torch's cast makes them
        elif hdt == torch.float16:
            k = k_top(vmax, TOP[torch.float16])
        else:
            k = k_top(float(c0.inter.max()), TOP[hdt])
        return k // 2, k - k // 2
    if hdt == torch.bfloat16 and row["op"] in STAT_OPS:
        return (lambda k: (k // 2, k - k // 2))(k_top(stats_of(row, c0)[..., 1].max().item(), TOP[hdt]) // 2)
    if hdt == torch.bfloat16:
        k = k_top(float(c0.inter.max()), TOP[hdt])
    else:
        off = injection(row, c0)[3]
        k = k_top(vmax, TOP[hdt] - off)
    if prop == "geglu":
        return 0, k
    return k // 2, k - k // 2


STAT_OPS = ("colstats_linear", "colstats_conv", "rowstats")


def stats_of(row, c):
    """The float64 (sum, sum of squares) blocks the fused-statistics epilogue of the row writes (gemm_ref.colstats / rowstats; the
    block height is the planner's answer the row records, a row-statistics tile spans the whole row here: one part)."""
    b = row["base"]
    if row["op"] == "rowstats":
        assert b["plan"]["rowstat_parts"] == 1
        return G.rowstats(c.value, c.N)
    return G.colstats(c.value, b["plan"]["colstat_rows"], b["feats"]["unit"])


def gemm_scaled(row, c0, exps):
    """The scaled Case: A x 2^ka, weights x 2^kw, addends x 2^(ka + kw) (GEGLU: the value half only; the gate half is untouched, so
    the product scales exactly), then the row's injection."""
    ka, kw = exps
    k = ka + kw
    c = copy.copy(c0)
    c.exps, c.k = (ka, kw), k
    c.a1 = c0.a1 * 2.0 ** ka
    if row["op"] == "shortcut":                         # both GEMMs of the fold scale alike; the value by 2^k exactly (a power of two)
        c.w, c.sc, c.w_sc = c0.w * 2.0 ** kw, c0.sc * 2.0 ** ka, c0.w_sc * 2.0 ** kw
        c.bias, c.bias_sc = c0.bias * 2.0 ** k, c0.bias_sc * 2.0 ** k
        c.value, c.bound, c.inter, c.offset = c0.value * 2.0 ** k, c0.bound * 2.0 ** k, c0.inter * 2.0 ** k, 0.0
        return c
    if c.geglu:
        value_rows = _geglu_perm(c) < c.N
        gate_w = c0.w[~value_rows]
        assert ka == 0 or not bool(gate_w.any()), "the gate must not see the scaling"
        c.w = torch.where(value_rows[:, None], c0.w * 2.0 ** kw, c0.w)
        c.bias = None if c0.bias is None else torch.where(value_rows, c0.bias * 2.0 ** k, c0.bias)
    else:
        c.w = c0.w * 2.0 ** kw
        c.bias = None if c0.bias is None else c0.bias * 2.0 ** k
    c.rowbias = None if c0.rowbias is None else c0.rowbias * 2.0 ** k
    c.residual = None if c0.residual is None else c0.residual * 2.0 ** k
    a_cols, w_cols, addends, off = injection(row, c0)
    c.offset = off
    if a_cols:
        c.a1, c.w = c.a1.clone(), c.w.clone()
        for col, v in a_cols.items():
            c.a1[:, col] = v
        for col, v in w_cols.items():
            c.w[:, col] = v
        for name, v in addends.items():
            setattr(c, name, getattr(c, name) + v)
    return evaluate(c)


def out_dtype(row, hdt):
    return NCHW_DT[row["base"]["feats"]["dtype"]] if row["op"] == "conv_nchw" else hdt


def mfma_subnormal_row(row, hdt):
    """Rows whose fp16 MFMA operand is subnormal with a full significand and whose sums are not exact in fp32 (additions beyond
    the rows the family was asked for, and the folded LayerNorm with x in the subnormals).  Measured on gfx950:
    the instruction keeps such operands - every lattice row is exact, every row is inside its float64 bound - but does not
    accumulate them to the bits of the same problem with normal operands, on every tile family alike.  For these rows check 1 is
    the bounded form of last_bit_check instead of bit equality."""
    if hdt != torch.float16:
        return False
    return row["prop"] in ("sub_act_gauss", "sub_w_gauss") or (row["op"] == "ln_linear" and row["end"] == "down")


def ulp_of(t, dt):
    """Spacing of dt at |t| (float64), the subnormal spacing below the smallest normal."""
    bits, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}[dt]
    e = torch.frexp(t.abs().clamp_min(2.0 ** emin))[1] - 1
    return torch.ldexp(torch.ones_like(t), e - bits)


def check1(g1, want, ex, odt, last_bit=False, allow=0.0):
    """(differing, beyond) of check 1 outside the excluded elements: elements that are not `want`, and of those the ones further
    from it than one unit in the last place of the output type plus `allow`.  Plain rows demand differing == 0.  last_bit rows
    (mfma_subnormal_row) demand beyond == 0 and differing + excluded <= EXCLUDE_CAP of the row.
    allow is the fp32 part of the family's own tolerance for the element (GEMM: K 2^-23 sum|a||w|, gemm_ref.gauss_k; folded
    LayerNorm: K32 roundings of the bound plus the conditioning term): base and scaled run are two fp32 summations of the same
    exact products, each within half of that of the exact sum, so they are within allow of each other before the one 16-bit
    rounding and within allow + 1 ulp after it.  Where an output is a cancelling sum, allow is many units of its last place - a
    bare 1-ulp rule is not a property of a correct kernel there (seen on the device: 2 - 8 such elements of 95 000).  The cap is
    the share of a row check 1 may leave out anyway, set by the family's rule and not by the measured counts."""
    same = (g1 == want) | ((g1 == 0) & (want == 0))
    diff = ~same & ~ex
    beyond = diff & ~((g1 - want).abs() <= ulp_of(want, odt) + allow)
    return int(diff.sum()), int(beyond.sum())


def excluded_mask(ref0, ref1, hdt):
    lim = NORMAL_MIN[hdt]
    return (ref0.abs() < lim) | (ref1.abs() < lim)


def judge_gemm(row, c0, c1, got0, got1, hdt, enforce=True):
    """Both checks of a gemm / conv row.  got0 / got1: the stored outputs of the base and the scaled run in the layout of c.value
    (any float dtype).  Prints the `[range]` line; returns dict(excluded, bitdiff, ratio, failed)."""
    import gpu_util
    odt = out_dtype(row, hdt)
    g0, g1 = got0.double().cpu(), got1.double().cpu()
    lattice = row["base"]["kind"] != "gauss"
    want1 = (g0 * 2.0 ** c1.k + c1.offset).to(odt).double()
    ex = torch.zeros_like(g0, dtype=torch.bool) if lattice else excluded_mask(c0.value, c1.value, hdt)
    last_bit = mfma_subnormal_row(row, hdt)
    allow = 0.0 if lattice else G.gauss_k(c1.Ktot, hdt) * (2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -11) * c1.bound + c1.tiny
    bitdiff, beyond = check1(g1, want1, ex, odt, last_bit, allow)
    excluded = int(ex.sum())
    name = f"{row['id']} {NAME[hdt]}"
    if lattice:
        exact = G.rne(c1.value, odt).double()
        inf_ok = exact.isinf()                          # an f16 NCHW output of the bf16 flavour: inf where torch's cast gives inf
        bitdiff += int((~((g1 == exact) | ((g1 == 0) & (exact == 0)))).sum())
        ratio = gpu_util.check_bound(name, torch.where(inf_ok, 0.0, g1), torch.where(inf_ok, 0.0, c1.value), c1.value.abs().clamp_max(1e300),
                                     k=0.0, hdt=odt, enforce=False)
    else:
        kk = G.gauss_k(c1.Ktot, odt) if odt != torch.float32 else c1.Ktot * 2.0
        ratio = gpu_util.check_bound(name, g1, c1.value, c1.bound, k=kk, tiny=c1.tiny, hdt=odt, enforce=False)
    report(row["id"], hdt, c1.exps, excluded, bitdiff, ratio)
    cap = EXCLUDE_CAP * g0.numel()
    bad1 = (beyond > 0 or bitdiff + excluded > cap) if last_bit else bitdiff > 0
    failed = bad1 or not ratio <= 1.0 or excluded > cap
    if enforce:
        assert excluded <= cap, f"{name}: {excluded} of {g0.numel()} elements excluded"
        assert ratio <= 1.0, f"{name}: the scaled run leaves the float64 bound by {ratio:.3g}x"
        assert not bad1, (f"{name}: {bitdiff} elements are not 2^k times the base run (or not the exact value)"
                          + (f", {beyond} of them by more than one unit in the last place (cap {cap:.0f} elements)" if last_bit else ""))
    return dict(excluded=excluded, bitdiff=bitdiff, ratio=ratio, failed=failed)


def report(rid, hdt, exps, excluded, bitdiff, ratio):
    print(f"[range] {rid}: storage {NAME[hdt]} exponents {tuple(exps)} excluded {excluded} bit differences {bitdiff} worst ratio {ratio:.3g}")


# ---- a torch emulation of a GEMM kernel, with the range mistakes the family is there to catch --------------------------------------------
MISTAKES = ("narrow_before_bias", "narrow_before_residual", "splitk_16bit_partials", "geglu_value_narrowed", "flush_subnormal_operands",
            "flush_subnormal_results")


def _narrow(t, dt):
    return t.to(torch.float32).to(dt).to(F64)


def _f32(t):
    return t.to(torch.float32).to(F64)


def flush(t, dt):
    return torch.where(t.abs() < NORMAL_MIN[dt], torch.zeros_like(t), t)


def emulate_gemm(c, hdt, mistake=None, odt=None):
    """The stored output of a correct kernel in the layout of c.value - fp32 accumulation per K slice (one slice unless the row
    forces split K), slices added in fp32, bias and row bias in fp32, (GEGLU,) residual in fp32, ONE narrowing - or of one with a
    seeded range mistake."""
    odt = odt or hdt
    A, W, bias, rb, res = operands(c)
    if mistake == "flush_subnormal_operands":
        A, W = flush(A, hdt), flush(W, hdt)
        res = None if res is None else flush(res, hdt)
    splits = max(1, c.row["splits"])
    steps = (c.K + 63) // 64
    per = (steps + splits - 1) // splits
    slabs = []
    for s in range(splits):
        k0, k1 = min(c.K, s * per * 64), min(c.K, (s + 1) * per * 64)
        if k1 > k0:
            slabs.append(_f32(A[:, k0:k1] @ W[:, k0:k1].T))
    if mistake == "splitk_16bit_partials":
        slabs = [_narrow(s, hdt) for s in slabs]
    acc = slabs[0]
    for s in slabs[1:]:
        acc = _f32(acc + s)
    if mistake == "narrow_before_bias":
        acc = _narrow(acc, hdt)
    if bias is not None:
        acc = _f32(acc + bias)
    if rb is not None:
        acc = _f32(acc + rb.repeat_interleave(c.rps, dim=0))
    if c.geglu:
        n = acc.shape[1] // 2
        val, gate = acc[:, :n], acc[:, n:]
        if mistake == "geglu_value_narrowed":
            val = _narrow(val, hdt)
        acc = _f32(val * _f32(G.gelu64(gate)))
    if mistake == "narrow_before_residual":
        acc = _narrow(acc, hdt)
    if res is not None:
        acc = _f32(acc + res)
    out = acc.to(torch.float32).to(odt).to(F64)
    if mistake == "flush_subnormal_results":
        out = flush(out, odt)
    return out


# ---- the other families: small helpers -------------------------------------------------------------------------------------------------------
def quantised(x, hdt, unit=2.0 ** -6, limit=1023):
    """x rounded to integers n * unit, |n| <= limit, then to the storage type: every value times 2^k stays a storage value as long
    as n 2^k unit is one - limit 1023 and unit 2^-6 put x 2^-18 on the fp16 subnormal lattice."""
    n = (x.double() / unit).round().clamp(-limit, limit)
    return (n * unit).to(hdt).to(torch.float32)


def judge_scaling(rid, hdt, exps, got0, got1, k, ref0, ref1, ratio, odt=None, exclude=True, exact=None, enforce=True, last_bit=False,
                  allow=0.0):
    """Check 1 for the families whose base and scaled outputs differ by 2^k alone (k = 0: an invariant output), with check 2's worst
    ratio (computed by the family's own bound) passed in.  exact: the expected stored value where the row lives on a lattice."""
    odt = odt or hdt
    g0, g1 = got0.double().cpu(), got1.double().cpu()
    want = (g0 * 2.0 ** k).to(odt).double()
    ex = excluded_mask(ref0.double(), ref1.double(), odt) if exclude else torch.zeros_like(g0, dtype=torch.bool)
    bitdiff, beyond = check1(g1, want, ex, odt, last_bit, allow)
    if exact is not None:
        e = exact.double()
        bitdiff += int((~((g1 == e) | ((g1 == 0) & (e == 0)))).sum())
    excluded = int(ex.sum())
    report(rid, hdt, exps, excluded, bitdiff, ratio)
    finite = bool(torch.isfinite(g1).all())
    cap = EXCLUDE_CAP * g0.numel()
    bad1 = (beyond > 0 or bitdiff + excluded > cap) if last_bit else bitdiff > 0
    failed = bad1 or not ratio <= 1.0 or excluded > cap or not finite
    if enforce:
        assert finite, f"{rid}: NaN / inf in the scaled output"
        assert excluded <= EXCLUDE_CAP * g0.numel(), f"{rid}: {excluded} of {g0.numel()} elements excluded"
        assert ratio <= 1.0, f"{rid}: the scaled run leaves the float64 bound by {ratio:.3g}x"
        assert not bad1, (f"{rid}: {bitdiff} elements of the scaled run are not 2^{k} times the base run"
                          + (f", {beyond} of them by more than one unit in the last place (cap {cap:.0f} elements)" if last_bit else ""))
    return dict(excluded=excluded, bitdiff=bitdiff, ratio=ratio, failed=failed)


# ---- GroupNorm / LayerNorm -----------------------------------------------------------------------------------------------------------------
NORM_UNIT = 2.0 ** -5                    # quantum of the normalisation inputs: |x| <= 1023 / 32, x 2^-19 is the fp16 subnormal lattice
EPS = 1e-5


def norm_inputs(row, hdt):
    """(x, gamma, beta) of a normalisation row: the inputs of tests/norm_fwd_ref.py on the quantum NORM_UNIT.  x [B, HW, C] or [M, C]."""
    import norm_fwd_ref as N
    s = row["shape"]
    if row["op"] in ("layernorm", "ln_linear"):
        x, gamma, beta = N.ln_inputs(s["M"], s["C"], hdt, seed=row["seed"], sigmas=(0.0, 2.0, 4.0))
    else:
        x, gamma, beta = N.gn_inputs(s["B"], s["H"] * s["W"], s["C"], s["G"], hdt, mean_sigma=0.3, seed=row["seed"])
    return quantised(x, hdt, NORM_UNIT), gamma, beta


def norm_sumsq_max(row, x):
    """The largest sum of squares a kernel of the row forms, float64: per (sample, group) / per row."""
    xd = x.double()
    if row["op"] in ("layernorm", "ln_linear"):
        return float((xd * xd).sum(1).max())
    B, HW, C = x.shape
    G_ = row["shape"]["G"]
    return float((xd * xd).reshape(B, HW, G_, C // G_).sum(dim=(1, 3)).max())


def fold_weights(row, hdt):
    """(W [N, C] of 16-bit values, bias [N]) of a gn_fold row, as tests/test_gpu_norm_fwd.py::test_gn_fold_weights_and_bias makes them."""
    import norm_fwd_ref as N
    C, n = row["shape"]["C"], row["N"]
    return N.q16(N.randn(n, C, seed=C + n + 5) / math.sqrt(C), hdt), 0.3 * N.randn(n, seed=C + n + 6)


def ln_linear_weights(row, hdt):
    """(W [N or 2 N][K] of 16-bit values, bias) of an ln_linear row, as tests/test_gpu_norm_fwd.py makes them."""
    import norm_fwd_ref as N
    K, rows = row["shape"]["C"], row["N"] * (2 if row["geglu"] else 1)
    return N.q16(N.randn(rows, K, seed=K + 21) / math.sqrt(K), hdt), 0.5 * N.randn(rows, seed=K + 22)


def row_parts(x):
    """[1][M][2] float32: the (sum, sum of squares) of every row of x, as the producing GEMM's row-statistics epilogue leaves them
    (one part); from float64 sums, so that the parts of 2^k x are exactly (2^k, 4^k) times the parts of x."""
    xd = x.double()
    return torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1)[None].float().contiguous()


def ln_linear_ref(row, x, gamma, beta, eps, W, bias, hdt):
    """(ref, bound, tiny) of an ln_linear row from norm_fwd_ref.ln_linear_ref (statistics pass); GEGLU: the product form of
    tests/test_gpu_norm_fwd.py::test_ln_linear_geglu_elementwise."""
    import norm_fwd_ref as N
    ref, bound, tiny = N.ln_linear_ref(x, gamma, beta, eps, W, bias, bool(row.get("parts")))
    if not row["geglu"]:
        return ref, bound, tiny
    (v, g), (bv, bg), (tv, tg) = ref.chunk(2, -1), bound.chunk(2, -1), tiny.chunk(2, -1)
    ge = N.gelu64(g)
    return v * ge, ge.abs() * bv + 1.13 * v.abs() * bg, ge.abs() * tv + 1.13 * v.abs() * tg + 1e-6 * v.abs()


def norm_exps(row, x, hdt, gamma=None, beta=None):
    """(k,): x -> 2^k x, eps -> 4^k eps.  up: fp16 - the largest |x| into (top / 2, top]; bf16 - the largest sum of squares a kernel
    forms stays <= 2^126.  down: fp16 - every non-zero x a subnormal (-24 - log2 NORM_UNIT); bf16 - the smallest k that keeps
    eps 4^k and the smallest non-zero x^2 4^k normal in fp32 (>= 2^-125).  gn_fold (fp16): x is scaled DOWN until the largest
    float64 folded weight W rstd gamma, which grows by 2^-k, lies in (top / 2, top]; bf16: as `down` - x^2 leaves fp32 long before a
    folded weight reaches the top."""
    if row["op"] == "gn_fold" and hdt == torch.float16:
        import norm_fwd_ref as N
        W, bias = fold_weights(row, hdt)
        wf = N.fold_ref(x, row["shape"]["G"], gamma, beta, float(eps_scaled(0)), W, bias)[0]
        return (-k_top(float(wf.abs().max()), TOP[hdt]),)
    if row["end"] == "up":
        if hdt == torch.float16:
            return (k_top(float(x.abs().max()), TOP[hdt]),)
        return (k_top(norm_sumsq_max(row, x), TOP[hdt]) // 2,)
    if hdt == torch.float16:
        return (-24 - floor_log2(NORM_UNIT),)
    m = min(EPS, float(x[x != 0].abs().min()) ** 2)
    return (math.ceil((-125 - math.log2(m)) / 2),)


def eps_scaled(k):
    """float32(eps) 4^k as the float the C ABI takes: exact."""
    import numpy as np
    return float(np.float32(EPS)) * 4.0 ** k


# ---- attention forward ----------------------------------------------------------------------------------------------------------------------
def attn_inputs(row, hdt):
    """(q, k, v, heads, presc, variant, vpad) of the BASE problem.  up: q, k of attn_fwd_ref.family_randn, V bounded away from zero.  down: uniform softmax
    (q = 0) over Nk = 64 or 256 keys with V = Nk n 2^-6, n in {-1, 0, 1}: the output sum(n) 2^-6 is exact, and times 2^-18 both V
    (Nk 2^-24) and the output (an integer <= Nk times 2^-24) are fp16 subnormals on the lattice."""
    import attn_cases as AC
    import attn_fwd_ref as A
    variant, presc, _, _, vpad = AC.BRANCHES[row["branch"]][:5]
    D = row["D"]
    B, heads = AC.batch_heads(D)
    Nq, Nk = row["shape"]["Nq"], row["shape"]["Nk"]
    if row["end"] == "up":
        # V = +-(1.5 + randn / 4), one sign per channel: every output, a convex combination, has magnitude >= 0.3.  The error of an
        # attention output is relative to sum p |v|, not to the output, so an output near zero could be a subnormal on the device
        # while its float64 reference is not; with no output near zero the reference alone says that check 1 excludes nothing.
        q, k, v = A.family_randn(B, heads, Nq, Nk, D, presc, hdt, seed=D)
        sign = torch.where(torch.arange(heads * D) % 3 == 0, -1.0, 1.0)
        return q, k, A.q16((1.5 + 0.25 * v) * sign, hdt), heads, presc, variant, vpad
    Nk = 256 if Nk >= 256 else 64
    q, k, _ = A.family_randn(B, heads, Nq, Nk, D, presc, hdt, seed=D)
    n = torch.randint(-1, 2, (B, Nk, heads * D), generator=torch.Generator().manual_seed(D + 1)).float()
    return torch.zeros_like(q), k, n * Nk * 2.0 ** -6, heads, presc, variant, vpad


def attn_exps(row, v, hdt):
    """(k,) for V.  up: fp16 - max |V| into (top / 2, top] (the output, a convex combination, is below it); bf16 - the kernels keep
    UNNORMALISED fp32 sums of p V with p up to 2^TAU (attn_fwd_ref.TAU: 60) over Nk keys, so 2^60 Nk max |V| 2^k <= 2^126.
    down: -18, see attn_inputs (the same numbers on the bf16 flavour: its fp32 products p V have no lower bound to approach)."""
    import attn_fwd_ref as A
    if row["end"] == "down":
        return (-18,)
    vmax = float(v.abs().max())
    if hdt == torch.float16:
        return (k_top(vmax, TOP[hdt]),)
    return (k_top(2.0 ** A.TAU[hdt] * v.shape[1] * vmax, TOP[hdt]),)


# ---- token merging --------------------------------------------------------------------------------------------------------------------------
def tome_inputs(row, hdt):
    """(keys, values, r): lattice keys fix the selection (tome_exact_ref.lattice_keys), the VALUES carry the range data."""
    import tome_exact_ref as X
    s = row["shape"]
    B, N, C, r = s["B"], s["N"], s["C"], s["r"]
    k = X.lattice_keys(B, N, C, seed=1000 + N, star=False, r=r)
    v = torch.randn(B, N, C, generator=torch.Generator().manual_seed(N)).to(hdt).float()
    # every token of a row that merges three or more: its first 8 channels a little above half the tensor's largest magnitude, same sign
    order, node_idx, _, reff = X.select64(k, r)
    rows, cnt = X.merge_rows(order, X.dstlist_of(order, node_idx, reff), reff, N)
    m = float(v.abs().max())
    many = torch.gather(cnt, 1, rows) >= 3                                   # [B, N]
    near_half = (m * (0.5 + 0.01 * (torch.arange(N) % 8).float()))[None, :, None].expand(B, N, 8)
    v[:, :, :8] = torch.where(many[:, :, None], near_half, v[:, :, :8]).to(hdt).float()
    return k, v, r


def tome_exps(row, k, v, r, hdt):
    """(k,).  merge: fp16 - max |v| into (top / 2, top]; bf16 - the largest sum of |v_i| over a merged row <= 2^126.  unmerge
    (dy = the first N - r rows of v): max |dy| to the top of either type (w dy has no sum)."""
    import tome_exact_ref as X
    if row["op"] == "tome_unmerge":
        return (k_top(float(v[:, :v.shape[1] - r].abs().max()), TOP[hdt]),)
    if hdt == torch.float16:
        return (k_top(float(v.abs().max()), TOP[hdt]),)
    order, node_idx, _, reff = X.select64(k, r)
    _, cnt, absmean = X.merge_wavg64(v, order, node_idx, reff)
    return (k_top(float((absmean * cnt[..., None]).max()), TOP[hdt]),)


def avgpool_exps(row, x, hdt):
    """(k,): top - fp16: max |x| into (top / 2, top]; bf16: the fp32 sum of four, 4 max |x| <= 2^126.  sub_out: -18 (avgpool_inputs)."""
    if row["prop"] == "sub_out":
        return (-18,)
    m = float(x.abs().max())
    return (k_top(m, TOP[hdt]),) if hdt == torch.float16 else (k_top(4 * m, TOP[hdt]),)


def derive(row, hdt):
    """The exponents of any row, from its base problem and float64 reference alone (range_cases.EXPS records them)."""
    fam = row["family"]
    if fam in ("gemm", "conv"):
        return tuple(derive_exps(row, gemm_base(row, hdt), hdt))
    if fam == "norm":
        x, gamma, beta = norm_inputs(row, hdt)
        return norm_exps(row, x, hdt, gamma, beta)
    if row["op"] == "cross_attention_block":
        return xattn_exps(row, xattn_inputs(row, hdt), hdt)
    if fam == "attn":
        return attn_exps(row, attn_inputs(row, hdt)[2], hdt)
    if fam == "tome":
        return tome_exps(row, *tome_inputs(row, hdt), hdt)
    if fam == "temb":
        return temb_exps(row, hdt)
    if fam == "lora":
        return lora_exps(row, hdt)
    if row["op"] == "avgpool2":
        return avgpool_exps(row, avgpool_inputs(row, hdt), hdt)
    return ()


# ---- boundary and element-wise kernels ---------------------------------------------------------------------------------------------------------
SRC_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def cast_specials(src):
    """float32 values a cast to a 16-bit type can get wrong, as a tensor of dtype `src` (values the source type cannot hold are
    rounded by torch's own cast first): ties at the last bit of fp16 and of bf16, 65504, 65519.99, 65520, the top of bf16, +-inf,
    NaN, the largest and smallest subnormals of both types and the ties around them, +-0."""
    inf, nan = float("inf"), float("nan")
    v = [0.0, -0.0, 1.0, -1.0,
         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -24,        # fp16 ties and their neighbours
         1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -24,            # bf16
         65504.0, 65519.99, 65520.0, 65536.0, -65504.0, -65519.99, -65520.0, 1e5, -1e5,
         2.0 ** 127 * (2 - 2.0 ** -7), 2.0 ** 127 * (2 - 2.0 ** -8), 3.4028234663852886e38, -3.4028234663852886e38,
         inf, -inf, nan,
         2.0 ** -14, 1023 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26,
         -1023 * 2.0 ** -24, -2.0 ** -24, -2.0 ** -25, -1.5 * 2.0 ** -24,
         2.0 ** -126, 127 * 2.0 ** -133, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -133, 2.0 ** -149, -2.0 ** -133, -2.0 ** -134]
    return torch.tensor(v, dtype=torch.float64).to(torch.float32).to(SRC_DT[src])


def cast_image(src, shape, seed=0):
    """A tensor of `shape` and dtype `src`: randn with the cast_specials written over its first elements, cycling to fill a quarter."""
    sp = cast_specials(src)
    n = 1
    for d in shape:
        n *= d
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(SRC_DT[src])
    reps = max(1, n // 4 // len(sp))
    x[:reps * len(sp)] = sp.repeat(reps)
    return x.reshape(shape)


def same_bits(got, want):
    """Count of elements that differ: bit patterns must agree, except that any NaN matches any NaN (payloads are not specified)."""
    g, w = got.cpu().contiguous(), want.cpu().contiguous()
    it = torch.int16 if g.element_size() == 2 else torch.int32
    nan = torch.isnan(g) & torch.isnan(w)
    return int(((g.view(it) != w.view(it)) & ~nan).sum())


def avgpool_inputs(row, hdt):
    """[B, H, W, C] base values.  top: randn with some 2 x 2 windows holding the tensor's largest magnitude four times (scaled: four
    values at the top, fp32 sum 2.6e5, mean in range).  sub_out: 4 m 2^-6, |m| <= 63: times 2^-18 the inputs are fp16 subnormals and
    every mean, sum(m) 2^-24 with |sum(m)| <= 252, is one too - exact in both storage types."""
    B, H, W, Cn = 2, 5, 6, 40
    g = torch.Generator().manual_seed(7)
    if row["prop"] == "top":
        x = torch.randn(B, H, W, Cn, generator=g).to(hdt).float()
        m = float(x.abs().max())
        x[0, 0:2, 0:2, :8] = m
        x[1, 2:4, 4:6, 8:16] = -m
        return x
    return torch.randint(-63, 64, (B, H, W, Cn), generator=g).float() * 4 * 2.0 ** -6


def avgpool_ref(x):
    B, H, W, Cn = x.shape
    xd = x.double()[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, Cn)
    return xd.mean(dim=(2, 4)), xd.abs().mean(dim=(2, 4))


def avgpool_tolerance(ref, mabs, hdt):
    """tests/test_gpu_t2i.py::test_avgpool2_against_float64: u |ref| + 2^-22 mean|x_i|, with the storage type's own rounding floor in
    place of that test's absolute 2^-24 (which is there for O(1) data and would hide everything at 2^-24)."""
    u = 2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -11
    return u * ref.abs() + 2.0 ** -22 * mabs + (2.0 ** -134 if hdt == torch.bfloat16 else 2.0 ** -25)


def avgpool_emulate(x, hdt, mistake=None):
    xd = x.double()
    if mistake == "flush_subnormal_operands":
        xd = flush(xd, hdt)
    B, H, W, Cn = x.shape
    t = xd[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, Cn)
    if mistake == "pool_sum_16bit":
        s = _narrow(t.sum(dim=(2, 4)), hdt)
    else:
        s = _f32(t.sum(dim=(2, 4)))
    out = _narrow(s * 0.25, hdt)
    return flush(out, hdt) if mistake == "flush_subnormal_results" else out


# ---- time-embedding path -----------------------------------------------------------------------------------------------------------------------
TEMB_UNIT = 2.0 ** -10


def temb_inputs(row, hdt):
    """(x [B, K] fp32, W [N, K] of 16-bit values, bias [N]) of the BASE problem: temb_ref.linear_inputs with W on the quantum 2^-10
    (|n| <= 1023), so that W 2^-14 is the fp16 subnormal lattice."""
    import temb_ref as T
    s = row["shape"]
    x, W, bias = T.linear_inputs(s["K"], s["N"], s["B"], seed=s["K"] + s["N"])
    return x, quantised(W, hdt, TEMB_UNIT), bias


def temb_exps(row, hdt):
    return (-24 - floor_log2(TEMB_UNIT),)


def tome_emulate(v, order, node_idx, reff, hdt, mistake=None):
    """merge_wavg of the values with an fp32 token sum (correct) or a 16-bit one."""
    import tome_exact_ref as X
    row, cnt = X.merge_rows(order, X.dstlist_of(order, node_idx, reff), reff, v.shape[1])
    B, N, C = v.shape
    acc = torch.zeros(B, N - reff, C, dtype=F64)
    for b in range(B):
        for t in range(N):                                # token by token, narrowing the running sum where the mistake says so
            a = acc[b, row[b, t]] + v[b, t].double()
            acc[b, row[b, t]] = _narrow(a, hdt) if mistake == "token_sum_16bit" else _f32(a)
    return _narrow(acc / cnt[..., None].double(), hdt)


# ---- the fused cross-attention block ------------------------------------------------------------------------------------------------------------
def xattn_inputs(row, hdt):
    """(x [M, C], gamma, beta, wq, k, v, wo, bo) as tests/test_gpu_attn_fwd.py::test_fused_cross_attention_block_against_its_operator_chain
    makes them (randn family), x moved away from zero and on the quantum 2^-5 so that it stays a storage value when scaled."""
    import attn_fwd_ref as A
    s = row["shape"]
    B, tokens, C_, heads, Nk = s["B"], s["tokens"], s["C"], s["heads"], s["Nk"]
    D = C_ // heads
    # x = 12 + 1.5 randn: the output x + bo + a Wo^T stays above 1 everywhere.  Its error is relative to the terms, not to the
    # output, so an output near zero could be a subnormal on the device while its float64 reference is not (as in attn_inputs)
    x = quantised(A.randn(B, tokens, C_, seed=401) * 1.5 + 12.0, hdt, NORM_UNIT).reshape(B * tokens, C_)
    g, be = A.randn(C_, seed=403) * 0.2 + 1, A.randn(C_, seed=404) * 0.2
    wq = A.q16(A.randn(C_, C_, seed=405) / math.sqrt(C_), hdt)
    wo = A.q16(A.randn(C_, C_, seed=406) / math.sqrt(C_), hdt)
    bo = A.randn(C_, seed=407) * 0.1
    k = A.q16(A.randn(B, Nk, C_, seed=408) * (A.LOG2E / math.sqrt(D)), hdt)
    v = A.q16(A.randn(B, Nk, C_, seed=409), hdt)
    return x, g, be, wq, k, v, wo, bo


def xattn_ref(row, ins, eps=EPS):
    """float64 (out, attention output a) of the block from the float64 references of its stages (norm_fwd_ref, attn_fwd_ref), with no
    intermediate rounding: what the exponent is derived from."""
    import attn_fwd_ref as A
    import norm_fwd_ref as N
    s = row["shape"]
    x, g, be, wq, k, v, wo, bo = ins
    n = N.ln_ref(x, g, be, eps)[0]
    q = (n @ wq.double().T).reshape(s["B"], s["tokens"], s["C"])
    a = A.fwd_ref(q, k, v, s["heads"], 1)[0].reshape(-1, s["C"])
    return x.double() + bo.double() + a @ wo.double().T, a


def xattn_exps(row, ins, hdt):
    """(k,): fp16 - the largest float64 output into (top / 2, top]; bf16 - as a normalisation row: the LayerNorm's sum of squares
    of a row of x, the first fp32 intermediate to leave its format, <= 2^126."""
    if hdt == torch.float16:
        return (k_top(float(xattn_ref(row, ins)[0].abs().max()), TOP[hdt]),)
    x = ins[0].double()
    return (k_top(float((x * x).sum(1).max()), TOP[hdt]) // 2,)


# ---- LoRA / LyCORIS merge --------------------------------------------------------------------------------------------------------------------------
def lora_inputs(row, hdt):
    """repack_lora: (case, base, pairs); repack_delta: (case, base, terms) - the families of tests/lora_ref.py / tests/lyco_ref.py."""
    if row["op"] == "repack_lora":
        import lora_ref as LRF
        from test_lora_ref_host import CASES
        case = next(c for c in CASES if c[0] == row["case"])
        name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
        conv = name.startswith("conv") or KH * KW > 1
        if row["data"] == "lattice":
            base, pairs, _ = LRF.lattice(O, I, ranks, KH, KW, conv=conv, seed=len(name))
        else:
            base, pairs = LRF.gaussian(O, I, ranks, KH, KW, conv=conv, seed=len(name))
        return case, base, pairs
    import lyco_ref as LY
    case = next(c for c in LY.CASES if c[0] == row["case"])
    return (case,) + tuple(LY.case_terms(case))


def lora_scaled(row, base, terms, k):
    """base x 2^k and every pair's up factor x 2^k (repack_lora); base x 2^k and every term's user scale x 2^k (repack_delta: its
    forms have no single up factor)."""
    import numpy as np
    f = np.float32(2.0 ** k)
    if row["op"] == "repack_lora":
        return base * f, [(up * f, down, s) for up, down, s in terms]
    return base * f, [(fields, user * 2.0 ** k) for fields, user in terms]


def lora_ref(row, case, base, terms, hdt):
    """(float64 value, tolerance, absolute-value form) [O][KH][KW][I_pad] from lora_ref / lyco_ref."""
    import numpy as np
    name, O, I, KH, KW, I_pad, geglu, scale_p = case[:8]
    if row["op"] == "repack_lora":
        import lora_ref as LRF
        absform = LRF.ref64(np.abs(base), [(np.abs(up), np.abs(down), abs(s)) for up, down, s in terms], I_pad, geglu, abs(scale_p))
        return LRF.ref64(base, terms, I_pad, geglu, scale_p), LRF.bound(base, terms, I_pad, geglu, scale_p, hdt), absform
    import lyco_ref as LY
    ref = LY.ref64(base, terms, I_pad, geglu, scale_p)
    return ref, LY.bound(base, terms, I_pad, geglu, scale_p, hdt), None


def lora_exps(row, hdt):
    """(k,).  up: fp16 - the largest merged weight into (top / 2, top]; bf16 - the absolute-value form of the merge (LyCORIS: the
    tolerance's own absolute sum is not exposed, so the largest merged weight times 2^8, a margin its lattice terms stay inside)
    <= 2^126.  down: the lattice (multiples of 1/4 up to 8, of 1/8 with scale_p = 1/2) onto the fp16 subnormals, n 2^-24 with n <= 64."""
    if row["op"] == "lyco_core":
        return (-18,)
    import numpy as np
    case, base, terms = lora_inputs(row, hdt)
    ref, _, absform = lora_ref(row, case, base, terms, hdt)
    if row["end"] == "down":
        k = -24                                             # the smallest k that leaves every merged weight an integer times 2^-24
        while not np.array_equal(ref * 2.0 ** (k + 24), np.round(ref * 2.0 ** (k + 24))):
            k += 1
        return (k,)
    m = float(np.abs(ref).max())
    if hdt == torch.float16:
        return (k_top(m, TOP[hdt]),)
    return (k_top(float(absform.max()) if absform is not None else m * 256.0, TOP[hdt]),)


def lyco_core_inputs(row):
    """(core [A, B, *tail] of fp16 values on the quantum 2^-6, right [B, C] fp32): core x 2^-18 is all fp16 subnormals."""
    import numpy as np
    s = row["shape"]
    g = np.random.default_rng(s["A"] + s["B"])
    core = quantised(torch.from_numpy(g.standard_normal((s["A"], s["B"], *s["tail"])).astype(np.float32)), torch.float16).numpy()
    right = g.standard_normal((s["B"], s["C"])).astype(np.float32)
    return core, right


# ---- the hint-residual add inside the UNet ------------------------------------------------------------------------------------------------------
def residual_targets(skip, src):
    """A residual r (dtype of `src`) that takes the skip tensor to the edges: skip + r lands on 65504, 65519.99, 65520, -65520, the
    largest and smallest fp16 subnormals and ties between them, cycling over the elements; what the source type cannot hold is
    rounded by torch's cast, and the expectation is formed from the rounded r."""
    t = torch.tensor([65504.0, 65519.99, 65520.0, -65520.0, 1023 * 2.0 ** -24, 2.0 ** -24, 1.5 * 2.0 ** -24, -2.0 ** -25, 1e5, 3e38],
                     dtype=torch.float64)
    n = skip.numel()
    target = t.repeat((n + len(t) - 1) // len(t))[:n].reshape(skip.shape)
    return (target - skip.double()).float().to(SRC_DT[src])


def residual_expected(skip, r, hdt):
    """One fp32 sum, one rounding to the storage type."""
    return (skip.float() + r.float()).to(hdt)
