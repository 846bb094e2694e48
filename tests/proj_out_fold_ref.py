"""Float64 reference of a Transformer2D's proj_out folded into the FF2 of its last block (csrc/model_impl.h Exec::proj_out_folded,
launch_compose_proj in csrc/kernels_elem.hip).  CPU only: no GPU import.

Nothing non-linear sits between the last block's FF2 and proj_out:

    h2  = ff W2^T + b2 + h                       (FF2: K = 4C, residual h)
    out = h2 Wp^T + bp + x                       (proj_out: K = C, residual x = the transformer's input)
  => out = [ff | h] Wc^T + bc + x,   Wc [C][5C] = [Wp W2 | Wp],   bc = Wp b2 + bp

The device makes Wc from the STORED 16-bit Wp and W2: every element one fmaf chain over k ascending in fp32, rounded once to the
storage type; the Wp columns are copied; bc is one fp32 fmaf chain per row plus bp.  The bounds below follow from that statement
alone (first-order worst case of a recursive fp32 sum of K terms: K 2^-24 sum |terms|), never from what the kernel returns.

MISTAKES: seeded errors of a composition; tests/test_proj_out_fold_ref_host.py shows that the comparison against the two-launch
form catches each of them.
"""
import torch

F64 = torch.float64
MISTAKES = ("wp_missing_on_h", "b2_not_through_wp", "residual_from_h", "w2_transposed")


def compose(Wp, W2, b2, bp, mistake=None):
    """Wp [C][C], W2 [C][4C], b2 [C], bp [C] (float64 holding the stored values) -> (Wc [C][5C], bc [C]) in float64."""
    Wp, W2, b2, bp = Wp.to(F64), W2.to(F64), b2.to(F64), bp.to(F64)
    C = Wp.shape[0]
    assert Wp.shape == (C, C) and W2.shape == (C, 4 * C) and b2.shape == (C,) and bp.shape == (C,)
    w2 = W2.T.contiguous().reshape(C, 4 * C) if mistake == "w2_transposed" else W2      # the transposed buffer read as [C][4C] rows
    right = torch.eye(C, dtype=F64) if mistake == "wp_missing_on_h" else Wp
    bc = (b2 if mistake == "b2_not_through_wp" else Wp @ b2) + bp
    return torch.cat([Wp @ w2, right], dim=1), bc


def folded(ff, h, x, Wc, bc, mistake=None):
    """out = [ff | h] Wc^T + bc + x (float64)."""
    res = h if mistake == "residual_from_h" else x
    return torch.cat([ff, h], dim=1).to(F64) @ Wc.to(F64).T + bc.to(F64) + res.to(F64)


def two_launch(ff, h, x, Wp, W2, b2, bp):
    """proj_out(FF2(ff) + h) + x (float64, no intermediate rounding)."""
    h2 = ff.to(F64) @ W2.to(F64).T + b2.to(F64) + h.to(F64)
    return h2 @ Wp.to(F64).T + bp.to(F64) + x.to(F64)


def folded_with(ff, h, x, Wp, W2, b2, bp, mistake=None):
    Wc, bc = compose(Wp, W2, b2, bp, mistake)
    return folded(ff, h, x, Wc, bc, mistake)


def storage_bits(hdt):
    """(significand bits incl. the hidden one, smallest normal exponent) of the 16-bit storage type."""
    return (8, -126) if hdt == torch.bfloat16 else (11, -14)


def half_ulp(v, hdt):
    """Half a unit in the last place of the storage type at the magnitude of v (float64 tensor), subnormal range included."""
    p, emin = storage_bits(hdt)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=F64), e - p)


def wc_bound(Wp, W2, hdt):
    """Element-wise tolerance of the stored Wc [C][5C] against compose()'s float64 value: the fp32 chain of C products is within
    acc = C 2^-24 sum_k |Wp[n][k] W2[k][j]| of the exact sum, and the one rounding adds half an ulp of the storage type at the
    magnitude of the value being rounded (at most |exact| + acc).  The copied Wp columns must be exact (tolerance 0)."""
    Wp, W2 = Wp.to(F64), W2.to(F64)
    C = Wp.shape[0]
    acc = C * 2.0 ** -24 * (Wp.abs() @ W2.abs())
    exact = Wp @ W2
    return torch.cat([half_ulp(exact.abs() + acc, hdt) + acc, torch.zeros(C, C, dtype=F64)], dim=1)


def bc_bound(Wp, b2, bp):
    """Tolerance of the fp32 bc [C]: C products in one chain, one more add for bp -> (C + 1) 2^-24 (sum_k |Wp[n][k] b2[k]| + |bp[n]|)."""
    Wp, b2, bp = Wp.to(F64), b2.to(F64), bp.to(F64)
    C = Wp.shape[0]
    return (C + 1) * 2.0 ** -24 * (Wp.abs() @ b2.abs() + bp.abs())


def emulate_fp32(Wp, W2, b2, bp, hdt):
    """A correct device computation in numpy-free torch: fp32 fmaf chains over k ascending (product exact in float64, one rounding
    per step), then ONE rounding to the storage type.  Returns (Wc in hdt, bc in float32)."""
    f32 = torch.float32
    Wp64, W264 = Wp.to(F64), W2.to(F64)
    C = Wp.shape[0]
    acc = torch.zeros(C, 4 * C, dtype=f32)
    accb = torch.zeros(C, dtype=f32)
    for k in range(C):
        acc = (acc.to(F64) + Wp64[:, k:k + 1] * W264[k:k + 1, :]).to(f32)
        accb = (accb.to(F64) + Wp64[:, k] * b2.to(F64)[k]).to(f32)
    return torch.cat([acc.to(hdt), Wp.to(hdt)], dim=1), (accb + bp.to(f32)).to(f32)


def operands(C, seed, hdt):
    """Stored weights of one site: Wp, W2 ~ N(0, 1 / fan_in) rounded to the storage type, biases fp32 (all returned as float64)."""
    g = torch.Generator().manual_seed(seed)
    Wp = (torch.randn(C, C, generator=g) / C ** 0.5).to(hdt).to(F64)
    W2 = (torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5).to(hdt).to(F64)
    b2 = (torch.randn(C, generator=g) * 0.1).float().to(F64)
    bp = (torch.randn(C, generator=g) * 0.1).float().to(F64)
    return Wp, W2, b2, bp


def activations(M, C, seed, hdt):
    g = torch.Generator().manual_seed(seed)
    ff = torch.randn(M, 4 * C, generator=g).to(hdt).to(F64)
    h = torch.randn(M, C, generator=g).to(hdt).to(F64)
    x = torch.randn(M, C, generator=g).to(hdt).to(F64)
    return ff, h, x
