"""The native Swin-B backbone (-m gpu; kernels_swinb.hip, model_swinb.hip behind gyre_amd.hinters.GyreHipSwinB) against the float64
restatement tests/swinb_ref.py (itself held to the reference's code by tests/test_swinb_ref_host.py), on both storage flavours.

k_win12_attn, element by element.  The bound is that of tests/swinir_ref.py (derived there the way tests/attn_fwd_ref.py derives the
forward-attention bound), recounted for 144 keys at D = 32; no factor is fitted.  u = 2^-8 (bf16) / 2^-11 (fp16), fl = half the smallest
storage subnormal, e = 2^-24; q, k, v are storage values, so every product is exact in fp32.  With A = sum_d |q_a,d| |k_b,d| and
L = |c (q . k)| + |bias| + |mask|, c = fl32(32^-1/2):
    logit        dl <= c 2 32 e A + 3 e L        (32 products in one MFMA, doubled for its undocumented adder tree; fma, mask add, one spare)
    exponent     r = 2 D + 2 e |x| + 4 e          (D = max_b dl: own logit and the maximum's; the subtraction, the exp2 product, v_exp_f32)
    row sum      R = sum_b p r + 144 e            (the p-weighted mean of the terms' errors, plus the 144 additions)
    probability  dp = p (r + R + 4 e) (1 + u) + u p + fl + 2^-126     (reciprocal and product; the one rounding to storage; flushed masked pairs)
    output       t = sum_b dp |v_b| + 2 160 e sum_b p |v_b|           (five MFMA steps of 32 products, 16 of them zeros, doubled as above)
    bound = t + u (|E| + t) + fl
Measured on an MI355X: worst |got - E| / bound 0.73 (bf16) and 0.59 (fp16) over the cases below.

Whole module.  The bar is the one of the SwinIR / HAT whole-network tests (tests/test_gpu_swinir_model.py): twice the rel-L2 of the
restatement with every stored tensor rounded to the storage type against the float64 restatement, both on storage-rounded weights;
EMULATION holds that distance per size and map (B = 1; B = 2 differs in the third digit).  The eight-block residual stream did not need
more: measured on an MI355X the native maps sit at 0.76 - 1.03 of the emulation's distance (the deepest map at 104 x 88: 8.14e-3
against 8.38e-3 in bf16, 1.053e-3 against 1.054e-3 in fp16), so the gate of twice the emulation holds without a wider bar.
"""
import ctypes as C

import pytest
import torch

import swinb_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hinters import GyreHipSwinB
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
E = 2.0 ** -24
# no padding / more than one window / row and column padding (36 x 24) / one padded window
MAPS = [(12, 12), (24, 24), (26, 22), (7, 6)]
EMULATION = {((96, 96), torch.bfloat16): [2.221e-03, 4.229e-03, 4.196e-03, 5.290e-03, 6.585e-03],
             ((104, 88), torch.bfloat16): [2.235e-03, 4.394e-03, 5.079e-03, 6.702e-03, 8.376e-03],
             ((96, 96), torch.float16): [2.752e-04, 5.326e-04, 5.295e-04, 7.241e-04, 8.961e-04],
             ((104, 88), torch.float16): [2.743e-04, 5.405e-04, 6.288e-04, 8.152e-04, 1.054e-03]}
_REF = {}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("shift", [0, 6])
@pytest.mark.parametrize("hw", MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_win12_attn_element_by_element(hw, shift, heads, storage, sdt):
    (H, W), B, lib = hw, 2, _lib.lib(storage)
    g = torch.Generator().manual_seed(H * 100 + W + shift + heads)
    qkv = torch.randn((B * H * W, 96 * heads), generator=g).to(sdt)
    qb = 0.5 * torch.randn(96 * heads, generator=g)                  # nonzero: the padded keys matter
    table = 0.5 * torch.randn((529, heads), generator=g)
    o0 = torch.full((B * H * W, 32 * heads + 8), 7.0, dtype=sdt)
    o, bias = o0.to(DEV), torch.empty(heads * 144 * 144, dtype=torch.float32, device=DEV)
    td, qd, bd = table.to(DEV), qkv.to(DEV), qb.to(DEV)               # (held: a temporary's memory is reused by the next one)
    _lib.check(lib.gyre_op_win12_bias(_st(), _p(td), heads, _p(bias)), lib)
    _lib.check(lib.gyre_op_win12_attn(_st(), _p(qd), 96 * heads, _p(bd), _p(o), o.shape[1], _p(bias), B, H, W, heads, shift), lib)
    torch.cuda.synchronize()
    got = o.cpu()

    val, d = R.win_attn(qkv.double().view(B, H, W, -1), qb.to(sdt).double(), table, heads, shift, detail=True)
    u, fl = U[sdt], FL[sdt]
    dot = d["scale"] * (d["q"] @ d["k"].transpose(-2, -1))
    Lm = dot.abs() + d["bias"].abs() + (d["mask"].abs() if shift else 0.0)
    dl = d["scale"] * 2 * 32 * E * (d["q"].abs() @ d["k"].abs().transpose(-2, -1)) + 3 * E * Lm
    p = torch.softmax(d["l"], -1)
    r = 2 * dl.amax(-1, keepdim=True) + 2 * E * (d["l"] - d["l"].amax(-1, keepdim=True)).abs() + 4 * E
    Rs = (p * r).sum(-1, keepdim=True) + 144 * E
    dp = p * (r + Rs + 4 * E) * (1 + u) + u * p + fl + 2.0 ** -126
    t = d["back"](dp @ d["v"].abs() + 2 * 160 * E * (p @ d["v"].abs()))
    bound = (t + u * (val.abs() + t) + fl).reshape(B * H * W, -1)
    n = 32 * heads
    worst = float(((got[:, :n].double() - val.reshape(B * H * W, -1)).abs() / bound).nan_to_num(nan=float("inf")).max())
    print(f"[swinb] win12_attn {sdt} {H}x{W} shift {shift} heads {heads}: worst |got - value64| / bound = {worst:.3f}")
    assert torch.equal(got[:, n:], o0[:, n:]), "a column outside the heads was written"
    assert worst <= 1.0


def _tiny(sdt):
    """(state dict rounded to storage as fp32, the same as float64) - shared"""
    if sdt not in _REF:
        sd = R.seeded_state_dict(weights.swinb_param_shapes(gcfg.swinb_config(**R.TINY)))
        sd = {k: v.to(sdt).float() for k, v in sd.items()}
        _REF[sdt] = (sd, {k: v.double() for k, v in sd.items()})
    return _REF[sdt]


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(96, 96), (104, 88)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_swinb_maps_against_the_float64_restatement(hw, B, storage, sdt):
    sd, sd64 = _tiny(sdt)
    m = GyreHipSwinB(**R.TINY)
    m.load_state_dict(sd, strict=False)                              # (the synthetic dict carries no index buffers)
    m = m.to(sdt).to(DEV)
    x = torch.rand((B, 3) + hw, generator=torch.Generator().manual_seed(1)).to(sdt)
    key = (hw, B, sdt)
    if key not in _REF:
        _REF[key] = R.net(sd64, R.TINY, x.double())
    got = m(x.to(DEV))
    assert len(got) == 5
    for i, (a, ref) in enumerate(zip(got, _REF[key])):
        assert a.dtype == sdt and a.is_contiguous() and tuple(a.shape) == tuple(ref.shape)
        dist, gate = R.rel_l2(a.float().cpu(), ref), 2 * EMULATION[(hw, sdt)][i]
        print(f"[swinb] {hw} B {B} {sdt} map {i}: rel-L2 against the float64 restatement {dist:.3e} (gate {gate:.3e})")
        assert dist <= gate


def test_swinb_real_configuration_and_refusals():
    m = GyreHipSwinB().to(torch.float16)
    g = torch.Generator().manual_seed(0)
    sd = {k: (v if k.endswith("index") else (1.0 + 0.02 * torch.randn(v.shape, generator=g) if "norm" in k and k.endswith("weight")
                                             else 0.02 * torch.randn(v.shape, generator=g)).to(torch.float16)) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)                                            # strict, buffers included
    m = m.to(DEV)
    x = torch.rand((1, 3, 96, 96), generator=g).to(DEV)
    a, b = m(x), m(x)
    assert [tuple(t.shape) for t in a] == [(1, 128, 24, 24), (1, 128, 24, 24), (1, 256, 12, 12), (1, 512, 6, 6), (1, 1024, 3, 3)]
    assert all(bool(torch.isfinite(t.float()).all()) and torch.equal(t, s) for t, s in zip(a, b))
    with pytest.raises(NotImplementedError):
        GyreHipSwinB(window_size=7)
    with pytest.raises(NotImplementedError):
        GyreHipSwinB(ape=True)
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 3, 96), device=DEV))
    bad, L = m._c_cfg(), m._L()
    bad.window_size = 7
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_swinb_create(C.byref(bad), 0, C.byref(C.c_void_p())), L)
