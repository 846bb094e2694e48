"""Element-wise parity of the input-gradient kernels (csrc/kernels_bwd.hip) against float64 CPU references (-m gpu).

Every reference is the exact formula evaluated on the exact 16-bit inputs the kernel receives (for attention, delta = rowsum(dO o)
with the o handed to the kernel, as the operation's contract says), and every element is held to

    |got - ref| <= k u bound + u |ref| + tiny                                   (gpu_util.check_bound)

where u is the unit roundoff of the 16-bit storage and bound the float64 absolute-value form of the same computation - the size of
what the kernel adds up, so a dropped or mis-scaled term that is small next to the result is still caught where it matters.
k = 4: a correct kernel rounds each 16-bit operand of its second products once (u |term|) and its output once (u |ref|), all
else is fp32.  The cotangents are chosen so that the terms kernels get wrong dominate: structured GroupNorm / LayerNorm cotangents
whose true gradient nearly cancels, and score ramps whose row maximum keeps moving under the one-pass dQ kernels.

The attention cases walk every dispatch branch of launch_attention_bwd; the head dims and the kernel set each reaches are in
tests/attn_cases.py (BWD_REACHES), which tests/test_attn_plan_host.py holds against the library's own rule.
"""
import math

import pytest
import torch

from attn_cases import BWD_D_ALL as D_ALL, BWD_EQUAL_V_DIMS, BWD_SCALING_DIMS, BWD_SUM_DIMS, bwd_elementwise_shapes
from gyre_amd import _lib
from gpu_util import DEV, HDT, check_bound, randn, release_kept, st, vp

pytestmark = pytest.mark.gpu

U = 2.0 ** -8 if HDT == torch.bfloat16 else 2.0 ** -11
TOK = ("sample", "token", "channel")


def q16(t):
    """Round to the storage dtype; returns float32 holding exactly the 16-bit values."""
    return t.to(HDT).float()


def dev16(t):
    return t.to(HDT).contiguous().to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------------------------------------------------------
def attn_inputs(B, heads, Nq, Nk, D, presc, seed=0, qscale=1.0, ramp=False, equal_v=False, do_scale=1.0):
    C = heads * D
    c = math.log2(math.e) / math.sqrt(D)
    q = q16(randn(B, Nq, C, seed=seed + 1) * qscale)
    kk = randn(B, Nk, C, seed=seed + 2)
    if ramp:               # later keys score higher: the running reference of the one-pass dQ kernels keeps moving
        kk = kk * torch.linspace(0.2, 2.0, Nk).view(1, Nk, 1)
    k = q16(kk * (c if presc else 1.0))
    v = randn(B, Nk, C, seed=seed + 3)
    if equal_v:
        v = v[:, :1].expand(B, Nk, C)
    v = q16(v)
    d_o = q16(randn(B, Nq, C, seed=seed + 4) * do_scale)
    sc = math.log(2.0) if presc else 1.0 / math.sqrt(D)
    P = (_heads(q, heads) @ _heads(k, heads).transpose(-1, -2) * sc).softmax(-1)
    o = q16(_merge(P @ _heads(v, heads)))
    return q, k, v, o, d_o


def _heads(t, heads):
    B, N, C = t.shape
    return t.double().reshape(B, N, heads, C // heads).transpose(1, 2)


def _merge(t):
    B, H, N, D = t.shape
    return t.transpose(1, 2).reshape(B, N, H * D)


def attn_ref(q, k, v, o, d_o, heads, presc):
    """float64 dQ, dK, dV of softmax(logits) V and their bounds:  dQ: beta sum_j |P|(|dP| + |delta|)|K_j|,
    dK: beta sum_q |P|(|dP| + |delta|)|Q_q|,  dV: sum_q |P||dO_q|."""
    D = q.shape[-1] // heads
    Q, K, V, O, dO = (_heads(t, heads) for t in (q, k, v, o, d_o))
    beta = math.log(2.0) if presc else 1.0 / math.sqrt(D)
    P = (Q @ K.transpose(-1, -2) * beta).softmax(-1)
    dP = dO @ V.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    A = P * (dP.abs() + delta.abs())
    ref = (_merge(beta * dS @ K), _merge(beta * dS.transpose(-1, -2) @ Q), _merge(P.transpose(-1, -2) @ dO))
    bnd = (_merge(beta * A @ K.abs()), _merge(beta * A.transpose(-1, -2) @ Q.abs()), _merge(P.transpose(-1, -2) @ dO.abs()))
    return ref, bnd


def run_attn(q, k, v, o, d_o, heads, presc, cross=False, ld_mult=1, off=0, sentinel=None):
    """gyre_op_attention_bwd on [B, N, ld_mult * C] buffers whose operand sits at column `off`; the other input columns hold NaN,
    the other output columns `sentinel` (int16 bits).  Returns (dq, dk, dv) as [B, N, C] float32 and the full output buffers."""
    L = _lib.lib()
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // heads
    ld = ld_mult * C

    def place(t):
        if ld_mult == 1:
            return dev16(t)
        buf = torch.full((t.shape[0], t.shape[1], ld), float("nan"), dtype=HDT, device=DEV)
        buf[..., off:off + C] = t.to(HDT).to(DEV)
        return buf[..., off:off + C]

    def out(n):
        if sentinel is None:
            return torch.zeros(B, n, ld, dtype=HDT, device=DEV)
        return torch.full((B, n, ld), sentinel, dtype=torch.int16, device=DEV).view(HDT)
    dqb = out(Nq)
    dkb, dvb = (None, None) if cross else (out(Nk), out(Nk))
    need = L.gyre_op_attention_bwd_workspace(B, heads, Nq, Nk, D)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    sl = slice(off, off + C)
    _lib.check(L.gyre_op_attention_bwd(st(), vp(place(q)), ld, vp(place(k)), ld, vp(place(v)), ld, vp(place(o)), ld,
                                       vp(place(d_o)), ld, B, heads, Nq, Nk, D, presc, vp(ws), need,
                                       vp(dqb[..., sl]), ld, vp(None if cross else dkb[..., sl]), ld,
                                       vp(None if cross else dvb[..., sl]), ld))
    release_kept()
    bufs = (dqb, dkb, dvb)
    res = tuple(None if b is None else b[..., sl].float().cpu() for b in bufs)
    return res, bufs


def attn_tiny(k, q, d_o, heads, presc):
    """Absolute floor of the attention checks: the fp16 dS / P operands of the second products are rounded to fp16's subnormal
    spacing 2^-24 where they are small (|dS| < 2^-14), an error no relative bound describes; summed over the contraction it is at
    most 2^-25 sum_j |K_j| (dQ), 2^-25 sum_q |Q_q| (dK) and 2^-25 sum_q |dO_q| (dV), times beta.  bf16 shares fp32's exponent
    range: no such floor."""
    if HDT == torch.bfloat16:
        return 0.0, 0.0, 0.0
    D = q.shape[-1] // heads
    beta = math.log(2.0) if presc else 1.0 / math.sqrt(D)
    e = 2.0 ** -25
    return (e * beta * k.double().abs().sum(1, keepdim=True), e * beta * q.double().abs().sum(1, keepdim=True),
            e * d_o.double().abs().sum(1, keepdim=True))


def check_attn(tag, got, ref, bnd, tiny=(0.0, 0.0, 0.0)):
    worst = []
    for name, g, r, b, t in zip(("dq", "dk", "dv"), got, ref, bnd, tiny):
        if g is not None:
            worst.append(check_bound(f"{tag} {name}", g, r, b, tiny=t, dims=TOK))
    return max(worst)


def attn_case(B, heads, Nq, Nk, D, presc, cross=False, **kw):
    q, k, v, o, d_o = attn_inputs(B, heads, Nq, Nk, D, presc, **kw)
    got, _ = run_attn(q, k, v, o, d_o, heads, presc, cross=cross)
    ref, bnd = attn_ref(q, k, v, o, d_o, heads, presc)
    tag = f"attn_bwd B{B} h{heads} {Nq}x{Nk} D{D} presc{presc}" + (" cross" if cross else "") + (" ramp" if kw.get("ramp") else "")
    check_attn(tag, got, ref, bnd, attn_tiny(k, q, d_o, heads, presc))
    return (q, k, v, o, d_o), got, ref, bnd


@pytest.mark.parametrize("B,Nq,Nk,D,presc", bwd_elementwise_shapes())
def test_attention_bwd_elementwise(B, Nq, Nk, D, presc):
    """(1, 1): one key per row, P = 1, dQ = dK = 0 exactly in the reference; (33, 31): ragged single tiles; (300, 257): enough
    32-row tiles to wrap the prefetch rings, ragged last tile; 1030 tokens: a UNet-sized self-attention."""
    attn_case(B, 2 if D < 512 else 1, Nq, Nk, D, presc)


@pytest.mark.parametrize("qscale", [6.0, 20.0])
@pytest.mark.parametrize("D", D_ALL)
def test_attention_bwd_large_logit_ramp(D, qscale):
    """Scores growing along the keys: the one-pass dQ kernels (D <= 160) re-centre their running reference several times per
    row.  qscale 6: the row maximum climbs about 45 log2 units past the first tile's; 20: about 160, so a reference that stopped
    following it would overflow 2^(s - m) in fp32."""
    attn_case(1, 2 if D < 512 else 1, 192, 640, D, 1, qscale=qscale, ramp=True)


@pytest.mark.parametrize("Nk", [1, 77])
@pytest.mark.parametrize("D", D_ALL)
def test_attention_bwd_cross(D, Nk):
    """dk = dv = NULL: the dQ kernel alone (text cross-attention: 77 keys)."""
    attn_case(2, 2 if D < 512 else 1, 300, Nk, D, 1, cross=True)


@pytest.mark.parametrize("D", D_ALL)
def test_attention_bwd_strided_operands_leave_other_columns_alone(D):
    """ld = 3C as in the reverse sweep's fused q|k|v rows, the head block at column C: NaN in every other input column must not
    leak in, and every other output column must come back bit-identical."""
    heads = 2 if D < 512 else 1
    q, k, v, o, d_o = attn_inputs(1, heads, 300, 257, D, 1, seed=10)
    sentinel = 0x7E5A
    got, bufs = run_attn(q, k, v, o, d_o, heads, 1, ld_mult=3, off=heads * D, sentinel=sentinel)
    ref, bnd = attn_ref(q, k, v, o, d_o, heads, 1)
    check_attn(f"attn_bwd strided ld=3C D{D}", got, ref, bnd, attn_tiny(k, q, d_o, heads, 1))
    C = heads * D
    for name, b in zip(("dq", "dk", "dv"), bufs):
        bits = b.view(torch.int16).cpu()
        gap = torch.cat([bits[..., :C], bits[..., 2 * C:]], -1)
        assert bool((gap == sentinel).all()), f"{name}: {int((gap != sentinel).sum())} gap elements overwritten"


@pytest.mark.parametrize("D", D_ALL)
def test_attention_bwd_cross_dq_bitwise_equals_self_dq(D):
    heads = 2 if D < 512 else 1
    ins = attn_inputs(2, heads, 130, 97, D, 0, seed=20)
    (dq_self, _, _), _ = run_attn(*ins, heads, 0)
    (dq_cross, _, _), _ = run_attn(*ins, heads, 0, cross=True)
    assert torch.equal(dq_self, dq_cross)


@pytest.mark.parametrize("D", D_ALL)
def test_attention_bwd_batch_sample_bitwise_equals_single_sample(D):
    heads = 2 if D < 512 else 1
    ins = attn_inputs(3, heads, 70, 65, D, 1, seed=30)
    full, _ = run_attn(*ins, heads, 1)
    for b in range(3):
        one, _ = run_attn(*(t[b:b + 1] for t in ins), heads, 1)
        for name, x, y in zip(("dq", "dk", "dv"), full, one):
            assert torch.equal(x[b:b + 1], y), f"sample {b} {name} differs from the B = 1 call"


_SCALES = [-4, 6] if HDT == torch.bfloat16 else [6]


@pytest.mark.parametrize("kexp", _SCALES)
@pytest.mark.parametrize("D", BWD_SCALING_DIMS)
def test_attention_bwd_power_of_two_cotangent_scaling_is_exact(D, kexp):
    """f(2^k dO) = 2^k f(dO) bit for bit: every step is linear in dO (delta, dP, dS, the fp32 sums) and a power of two commutes
    with every rounding - unless a value leaves the format's range.  The ramp puts p = 2^(s - m) of the one-pass dQ kernels at
    its largest; with k = 6 |dP - delta| reaches several hundred (the guided loss is scaled by 500 x guidance_scale before it is
    differentiated)."""
    heads = 2
    ins = attn_inputs(1, heads, 192, 640, D, 1, qscale=6.0, ramp=True, seed=40)
    q, k, v, o, d_o = ins
    s = 2.0 ** kexp
    base, _ = run_attn(q, k, v, o, d_o, heads, 1)
    scaled, _ = run_attn(q, k, v, o, d_o * s, heads, 1)
    ref, bnd = attn_ref(q, k, v, o, d_o * s, heads, 1)
    check_attn(f"attn_bwd D{D} ramp dO*2^{kexp}", scaled, ref, bnd, attn_tiny(k, q, d_o * s, heads, 1))
    for name, x, y in zip(("dq", "dk", "dv"), base, scaled):
        diff = int((x * s != y).sum())
        print(f"[scale] D{D} {name}: {diff} of {x.numel()} elements of f(2^{kexp} dO) differ from 2^{kexp} f(dO)")
        # fp16: a dS / P operand or an output below 2^-14 is rounded to the fixed subnormal spacing 2^-24, which does not scale -
        # scaling moves values in or out of that range, so only the bound above (no overflow, same accuracy) holds there
        if HDT == torch.bfloat16:
            assert diff == 0, f"{name}: {diff} elements of f(2^{kexp} dO) differ from 2^{kexp} f(dO)"


@pytest.mark.parametrize("D", BWD_SUM_DIMS)
def test_attention_bwd_sum_identities(D):
    """Per (sample, head):  sum_j dV_j = sum_q dO_q  and  sum_j dK_j = beta sum_q Q_q dO_q.(O_q - o_q)  (zero but for the rounding
    of the o handed in), each within the summed element bounds."""
    heads = 2 if D < 512 else 1
    (q, k, v, o, d_o), got, ref, bnd = attn_case(2, heads, 200, 150, D, 1, seed=50)
    Q, K, V, Ob, dO = (_heads(t, heads) for t in (q, k, v, o, d_o))
    beta = math.log(2.0)
    O = (Q @ K.transpose(-1, -2) * beta).softmax(-1) @ V
    want_k = beta * (Q * (dO * (O - Ob)).sum(-1, keepdim=True)).sum(2)          # [B, H, D]
    want_v = dO.sum(2)
    for name, g, want, b in (("sum dK", got[1], want_k, bnd[1]), ("sum dV", got[2], want_v, bnd[2])):
        gs = _heads(g, heads).sum(2)
        tol = (4 * U * _heads(b, heads) + U * _heads(g, heads).abs()).sum(2)
        check_bound(f"attn_bwd D{D} {name}", gs, want, tol / (4 * U), k=4.0, dims=("sample", "head", "d"))


@pytest.mark.parametrize("D", BWD_EQUAL_V_DIMS)
def test_attention_bwd_equal_value_rows_give_zero_dq_dk(D):
    """All V rows equal: O = v for every query, dP_qj = dO_q.v = delta_q, so dS = 0 and dQ = dK = 0 up to the rounding of dP and
    delta - within the bound."""
    heads = 2
    attn_case(1, heads, 200, 150, D, 1, seed=60, equal_v=True)


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm / LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------------
def norm_ref(xg, dyg, gam, bet, silu, eps=1e-5):
    """xg, dyg [..., n] (the normalised set on the last axis... reshaped by the caller), gam / bet broadcastable: float64 dx and
    its bound rstd (|g| + mean|g| + |xh| mean|g xh|)."""
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (xg - mean) * rstd
    g = dyg * gam
    if silu:
        u = xh * gam + bet
        s = torch.sigmoid(u)
        g = g * s * (1 + u * (1 - s))
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    bound = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    return dx, bound, xh


def _gn_group_view(t, G):     # [B, HW, C] -> [B, G, HW * cpg]
    B, HW, C = t.shape
    return t.double().reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)


def _gn_ungroup(t, B, HW, C, G):
    return t.reshape(B, G, HW, C // G).permute(0, 2, 1, 3).reshape(B, HW, C)


def _structured_dy(xh, gam, seed):
    """dy = (alpha + beta xh) / gamma + small noise per normalised set: the true dx is the noise's, the mean corrections carry
    the rest."""
    sh = xh.shape[:-1] + (1,)
    a, b = randn(*sh, seed=seed).double() + 0.5, randn(*sh, seed=seed + 1).double()
    return (a + b * xh) / gam + 0.01 * randn(*xh.shape, seed=seed + 2).double()


@pytest.mark.parametrize("B,H,W,C,C1,G,silu,add,mean_sigma", [
    (2, 65, 65, 320, 320, 32, 0, 1, 0), (2, 65, 65, 320, 320, 32, 1, 0, 0),
    (1, 65, 65, 960, 640, 32, 0, 0, 0), (1, 65, 65, 960, 640, 32, 1, 1, 0),        # a group straddles the two sources
    (1, 65, 65, 2560, 1280, 32, 0, 1, 0), (1, 65, 65, 2560, 1280, 32, 1, 0, 0),    # NV = 2
    (1, 65, 65, 5120, 5120, 32, 0, 0, 0), (1, 33, 33, 5120, 2560, 32, 1, 0, 0),    # NV = 3 -> the NV = 4 kernels
    (2, 65, 65, 320, 320, 8, 0, 0, 8), (1, 65, 65, 2560, 1280, 8, 0, 1, 0),
    (2, 9, 7, 64, 64, 32, 0, 0, 8)])
def test_groupnorm_bwd_elementwise(B, H, W, C, C1, G, silu, add, mean_sigma):
    L = _lib.lib()
    HW = H * W
    # a different mean and scale per sample (sample 0 at mean_sigma standard deviations when asked)
    means = torch.tensor([float(mean_sigma) if mean_sigma else 0.3, -2.0, 1.0])[:B].view(B, 1, 1)
    scales = torch.tensor([1.5, 0.25, 3.0])[:B].view(B, 1, 1)
    x = q16(randn(B, HW, C, seed=1) * scales + means * scales)
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3))
    beta = randn(C, seed=4) * 0.2
    gam_g = _gn_group_view(gamma.view(1, 1, C).expand(1, HW, C), G)          # [1, G, HW cpg]
    bet_g = _gn_group_view(beta.view(1, 1, C).expand(1, HW, C), G)
    xg = _gn_group_view(x, G)
    if silu:
        dy = q16(randn(B, HW, C, seed=2))
    else:
        _, _, xh = norm_ref(xg, xg, gam_g, bet_g, 0)
        dy = q16(_gn_ungroup(_structured_dy(xh, gam_g, seed=5), B, HW, C, G).float())
    dx, bound, _ = norm_ref(xg, _gn_group_view(dy, G), gam_g, bet_g, silu)
    ref, bnd = _gn_ungroup(dx, B, HW, C, G), _gn_ungroup(bound, B, HW, C, G)
    addend = q16(randn(B, HW, C1, seed=6)) if add else None
    if add:
        ref = torch.cat([ref[..., :C1] + addend.double(), ref[..., C1:]], -1)
    x1, x2 = dev16(x[..., :C1]), (dev16(x[..., C1:]) if C1 < C else None)
    dx1 = torch.empty(B, HW, C1, dtype=HDT, device=DEV)
    dx2 = torch.empty(B, HW, C - C1, dtype=HDT, device=DEV) if C1 < C else None
    need = L.gyre_op_groupnorm_bwd_workspace(B, HW, C, G)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.check(L.gyre_op_groupnorm_bwd(st(), vp(x1), vp(x2), C1, B, HW, C, G, vp(gamma.to(DEV)), vp(beta.to(DEV)), 1e-5, silu,
                                       vp(dev16(dy)), vp(dev16(addend)) if add else None, vp(ws), need, vp(dx1), vp(dx2)))
    release_kept()
    got = dx1.float().cpu() if C1 == C else torch.cat([dx1.float().cpu(), dx2.float().cpu()], -1)
    tag = f"gn_bwd {B}x{H}x{W}x{C} C1={C1} G={G} silu={silu} add={add} mean={mean_sigma}sigma"
    check_bound(tag, got, ref, bnd, dims=("sample", "pixel", "channel"))
    # identities per (sample, group), addend subtracted:  sum dx = 0  and  sum dx xh = 0
    pure = got.double()
    if add:
        pure = torch.cat([pure[..., :C1] - addend.double(), pure[..., C1:]], -1)
    _, _, xh = norm_ref(xg, xg, gam_g, bet_g, 0)
    pg, bg, rg = _gn_group_view(pure, G), _gn_group_view(bnd, G), _gn_group_view(ref.abs(), G)
    for name, w in (("sum dx", 1.0), ("sum dx xh", xh.abs())):
        s = (pg * (1.0 if name == "sum dx" else xh)).sum(-1)
        tol = ((4 * U * bg + U * rg + U * pg.abs()) * w).sum(-1)
        check_bound(f"{tag} {name}", s, torch.zeros_like(s), tol / (4 * U), dims=("sample", "group"))


def test_groupnorm_bwd_rejects_more_than_four_vectors_per_thread():
    L = _lib.lib()
    B, HW, C, G = 1, 16, 8448, 32                                 # C / 8 = 1056 vectors over 256 lanes: five per thread
    x = dev16(randn(B, HW, C, seed=1))
    dx = torch.empty(B, HW, C, dtype=HDT, device=DEV)
    need = L.gyre_op_groupnorm_bwd_workspace(B, HW, C, G)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    g = torch.ones(C, device=DEV)
    rc = L.gyre_op_groupnorm_bwd(st(), vp(x), None, C, B, HW, C, G, vp(g), vp(g * 0), 1e-5, 0, vp(x), None, vp(ws), need, vp(dx), None)
    release_kept()
    assert rc == -6


@pytest.mark.parametrize("M_,C,add,mean_sigma", [(1, 8, 0, 0), (6, 8, 1, 8), (7, 64, 0, 0), (33, 64, 1, 8), (5, 320, 1, 0),
                                                 (66, 320, 0, 8), (7, 2048, 1, 0), (33, 2048, 0, 8), (2, 2048, 0, 0)])
def test_layernorm_bwd_elementwise(M_, C, add, mean_sigma):
    """Four rows per workgroup: M = 1, 2, 3 mod 4 leave ragged last blocks."""
    L = _lib.lib()
    rows_mean = torch.linspace(-1, 1, M_).view(M_, 1) + float(mean_sigma)
    rows_scale = torch.linspace(0.3, 2.0, M_).view(M_, 1)
    x = q16((randn(M_, C, seed=1) + rows_mean) * rows_scale)
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(3))
    gam = gamma.double().view(1, C)
    _, _, xh = norm_ref(x.double(), x.double(), gam, 0.0, 0)
    dy = q16(_structured_dy(xh, gam, seed=5).float())
    ref, bnd, xh = norm_ref(x.double(), dy.double(), gam, 0.0, 0)
    addend = q16(randn(M_, C, seed=6)) if add else None
    if add:
        ref = ref + addend.double()
    dx = torch.empty(M_, C, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_layernorm_bwd(st(), vp(dev16(x)), vp(dev16(dy)), M_, C, vp(gamma.to(DEV)), 1e-5,
                                       vp(dev16(addend)) if add else None, vp(dx)))
    release_kept()
    got = dx.float().cpu()
    check_bound(f"ln_bwd {M_}x{C} add={add} mean={mean_sigma}sigma", got, ref, bnd, dims=("row", "channel"))


def test_layernorm_bwd_rejects_wide_rows():
    L = _lib.lib()
    M_, C = 4, 2056
    x = dev16(randn(M_, C, seed=1))
    dx = torch.empty(M_, C, dtype=HDT, device=DEV)
    rc = L.gyre_op_layernorm_bwd(st(), vp(x), vp(x), M_, C, vp(torch.ones(C, device=DEV)), 1e-5, None, vp(dx))
    release_kept()
    assert rc == -6


# ---------------------------------------------------------------------------------------------------------------------------
# GEGLU backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M_,F_", [(41, 16), (1, 16)])
def test_geglu_bwd_gate_grid(M_, F_):
    """Gates on a grid over [-10, 10] that contains 0, against the float64 erf-GELU derivative:
    d val = dy gate Phi(gate),  d gate = dy val (Phi(gate) + gate phi(gate))."""
    L = _lib.lib()
    n = M_ * F_
    if n >= 641:
        grid = torch.linspace(-10.0, 10.0, 641)                      # step 1/32: 0 and +-10 exactly
        gate = torch.cat([grid, grid[: n - 641]])
    else:
        gate = torch.tensor([-10.0, -8, -6, -5, -4, -3, -2, -1, -0.5, 0, 0.5, 1, 2, 4, 6, 10])
    gate = q16(gate.view(M_, F_))
    val = q16(randn(M_, F_, seed=1) * 2)
    dy = q16(randn(M_, F_, seed=2))
    x, vv, d = gate.double(), val.double(), dy.double()
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    ref_v, ref_g = d * x * cdf, d * vv * (cdf + x * pdf)
    bnd_v, bnd_g = d.abs() * x.abs() * cdf, d.abs() * vv.abs() * (cdf + x.abs() * pdf)
    # The kernel evaluates Phi = 0.5 (1 + erf(x / sqrt 2)) in fp32: near Phi = 0 (x < -3) the sum 1 + erf keeps an absolute error
    # of about one fp32 ulp of 1 (2^-23, erff's own error included), 2^-24 after the halving - a floor no relative bound covers.
    eps = 2.0 ** -23
    tiny_v, tiny_g = eps * d.abs() * x.abs(), eps * d.abs() * vv.abs()

    def pack(a, b):     # packed column order of the GEGLU weight rows: 16 values then their 16 gates
        return torch.stack([a.reshape(M_, F_ // 16, 16), b.reshape(M_, F_ // 16, 16)], 2).reshape(M_, 2 * F_)
    dpre = torch.empty(M_, 2 * F_, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_geglu_bwd(st(), vp(dev16(pack(val, gate))), vp(dev16(dy)), M_, F_, vp(dpre)))
    release_kept()
    got = dpre.float().cpu().reshape(M_, F_ // 16, 2, 16)
    got_v, got_g = got[:, :, 0].reshape(M_, F_), got[:, :, 1].reshape(M_, F_)
    check_bound(f"geglu_bwd {M_}x{F_} d val", got_v, ref_v, bnd_v, tiny=tiny_v, dims=("row", "column"))
    check_bound(f"geglu_bwd {M_}x{F_} d gate", got_g, ref_g, bnd_g, tiny=tiny_g, dims=("row", "column"))
