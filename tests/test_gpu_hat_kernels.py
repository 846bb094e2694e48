"""The kernels of the HAT upscaler (-m gpu; kernels_hat.hip) through their raw-operator entry points, on both storage flavours in this
process: the 16 x 16 window attention gyre_op_hat_attn in its two modes (shifted self-attention, overlapping cross-attention), the
channel-attention passes gyre_op_chan_pool / gyre_op_chan_gate / gyre_op_scale_add and gyre_op_pixel_shuffle2.  Values, host emulation
and the element-wise bounds: tests/hat_ref.py (derived there, held against seeded mistakes in tests/test_hat_ref_host.py)."""
import ctypes as C

import pytest
import torch

import hat_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
IDS = ["-".join(map(str, c)) for c in R.CASES]
MODE = {"sa": 0, "oca": 1}


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_attn(L, lib, expect=None, **over):
    """one gyre_op_hat_attn call on the data of L (hat_ref.case); returns the output buffer.  over: argument overrides for the refusal
    tests; expect: the exception type a refused call must raise (the buffer must then come back untouched)."""
    qkv, o, table = L["qkv"].to(DEV), L["o"].to(DEV), L["table"].contiguous().to(DEV)
    a = dict(ld_qkv=qkv.shape[1], ld_o=o.shape[1], mode=MODE[L["mode"]], B=L["B"], H=L["H"], W=L["W"], heads=L["heads"], shift=L["shift"])
    a.update(over)
    rc = lib.gyre_op_hat_attn(_st(), _p(qkv), a["ld_qkv"], _p(o), a["ld_o"], _p(table), a["mode"], a["B"], a["H"], a["W"], a["heads"],
                              a["shift"])
    torch.cuda.synchronize()
    if expect is not None:
        with pytest.raises(expect):
            _lib.check(rc, lib)
        assert torch.equal(R.bits(o.cpu()), R.bits(L["o"])), "a refused call wrote to the output buffer"
        return None
    _lib.check(rc, lib)
    return o.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_hat_attn_element_by_element(case, storage, sdt):
    L = R.case(sdt, *case)
    lib = _lib.lib(storage)
    got = run_attn(L, lib)
    n = 30 * L["heads"]
    assert bool(torch.isfinite(got[:, :n].float()).all()), "a live column was left unwritten"
    worst, rest = R.verdict(L, got)
    print(f"[hat] hat_attn {sdt} {case}: worst |got - value64| / bound = {worst:.3f}")
    assert rest, "an element outside the live columns changed"
    assert worst <= 1.0
    assert torch.equal(R.bits(got), R.bits(run_attn(L, lib))), "two calls differ"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
def test_hat_attn_refusals_write_nothing(storage, sdt):
    lib = _lib.lib(storage)
    L = R.case(sdt, "sa", 1, 16, 32, 2, 8)
    for over, exc in ((dict(H=24), ValueError), (dict(W=40), ValueError), (dict(H=8), ValueError), (dict(H=0), ValueError),
                      (dict(shift=4), NotImplementedError), (dict(shift=16), NotImplementedError), (dict(heads=9), NotImplementedError),
                      (dict(heads=0), NotImplementedError), (dict(ld_qkv=100), ValueError), (dict(ld_o=40), ValueError),
                      (dict(ld_qkv=196), NotImplementedError), (dict(B=0), ValueError), (dict(mode=2), ValueError),
                      (dict(mode=1), ValueError)):                          # (the overlapping form is not shifted)
        run_attn(L, lib, expect=exc, **over)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", R.CAB_CASES, ids=["-".join(map(str, c)) for c in R.CAB_CASES])
def test_pool_gate_scale_add_against_fp64(case, storage, sdt):
    lib = _lib.lib(storage)
    L = R.cab_case(sdt, *case)
    B, HW, C_, Cs, ld = L["B"], L["H"] * L["W"], L["C"], L["Cs"], L["ld"]
    c2d, yd = L["c2"].to(DEV), L["y"].to(DEV)
    need = lib.gyre_op_chan_pool_workspace(B, HW, C_)
    assert need == B * ((HW + 63) // 64) * C_ * 4
    part = torch.full((need // 4 + 4,), float("nan"), device=DEV)
    pool = torch.full((B * C_ + 4,), float("nan"), device=DEV)
    gate = torch.full((B, ld), float("nan"), device=DEV)
    w = {k: L[k].contiguous().to(DEV) for k in ("w1", "b1", "w2", "b2")}
    _lib.check(lib.gyre_op_chan_pool(_st(), _p(c2d), ld, B, HW, C_, _p(part), _p(pool)), lib)
    _lib.check(lib.gyre_op_chan_gate(_st(), _p(pool), B, C_, Cs, _p(w["w1"]), _p(w["b1"]), _p(w["w2"]), _p(w["b2"]), L["scale"], _p(gate), ld), lib)
    _lib.check(lib.gyre_op_scale_add(_st(), _p(yd), ld, _p(c2d), ld, _p(gate), ld, B, HW, ld), lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pool[B * C_:]).all()) and bool(torch.isnan(part[need // 4:]).all()), "the pool wrote past its outputs"
    pref, pbd = R.pool_ref(L["c2"], C_)
    gotp = pool[:B * C_].cpu().view(B, C_).double()
    wp = float(((gotp - pref).abs() / pbd.clamp_min(1e-300)).max())
    sref, sbd = R.gate_ref(pref, pbd, L)
    gots = gate.cpu().double()
    wg = float(((gots[:, :C_] - sref).abs() / sbd).max())
    assert bool((gots[:, C_:] == 0).all()), "the gate's padding channels must be zero"
    wy = R.cab_verdict(L, yd.cpu())
    print(f"[hat] cab {sdt} {case}: worst ratio pool {wp:.3f}, gate {wg:.3f}, scale-add {wy:.3f}")
    assert wp <= 1.0 and wg <= 1.0 and wy <= 1.0
    assert bool((yd.cpu()[..., C_:].float() == 0).all()), "padding channels must stay exactly zero"
    # a sample alone gives the bits it gives in the batch: the pool's order does not depend on B
    pool1 = torch.empty(C_, device=DEV)
    one = c2d[B - 1:].contiguous()
    _lib.check(lib.gyre_op_chan_pool(_st(), _p(one), ld, 1, HW, C_, _p(part), _p(pool1)), lib)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(pool1.cpu()), R.bits(pool[(B - 1) * C_:B * C_].cpu()))


def test_cab_op_refusals():
    lib = _lib.lib(_lib.BF16)
    x = torch.zeros((1, 64, 264), dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    for args, exc in (((_p(x), 264, 1, 64, 257, _p(f), _p(f)), NotImplementedError), ((_p(x), 60, 1, 64, 60, _p(f), _p(f)), ValueError),
                      ((_p(x), 260, 1, 64, 60, _p(f), _p(f)), NotImplementedError), ((_p(x), 264, 0, 64, 60, _p(f), _p(f)), ValueError),
                      ((None, 264, 1, 64, 60, _p(f), _p(f)), ValueError)):
        with pytest.raises(exc):
            _lib.check(lib.gyre_op_chan_pool(_st(), *args), lib)
    for C_, Cs, lds, exc in ((257, 8, 264, NotImplementedError), (60, 9, 64, NotImplementedError), (60, 2, 56, ValueError), (0, 2, 64, ValueError)):
        with pytest.raises(exc):
            _lib.check(lib.gyre_op_chan_gate(_st(), _p(f), 1, C_, Cs, _p(f), _p(f), _p(f), _p(f), 0.01, _p(f), lds), lib)
    for ldy, ldc, lds, Cn, exc in ((264, 264, 264, 60, NotImplementedError), (260, 264, 264, 64, NotImplementedError), (56, 264, 264, 64, ValueError),
                                   (264, 264, 62, 64, ValueError), (264, 264, 66, 64, NotImplementedError)):
        with pytest.raises(exc):
            _lib.check(lib.gyre_op_scale_add(_st(), _p(x), ldy, _p(x), ldc, _p(f), lds, 1, 64, Cn), lib)
    for ldx, Co, ldo, exc in ((264, 60, 64, NotImplementedError), (248, 64, 64, ValueError), (264, 64, 56, ValueError), (260, 64, 64, NotImplementedError)):
        with pytest.raises(exc):
            _lib.check(lib.gyre_op_pixel_shuffle2(_st(), _p(x), ldx, 1, 2, 2, Co, _p(x), ldo), lib)
    torch.cuda.synchronize()
    assert not bool(x.any()) and not bool(f.any()), "a refused call wrote"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("B,H,W,Co,ld_x,ld_o", [(2, 5, 7, 64, 256, 64), (1, 3, 37, 8, 40, 16), (1, 17, 9, 16, 64, 16)])
def test_pixel_shuffle2_is_exact(B, H, W, Co, ld_x, ld_o, storage, sdt):
    lib = _lib.lib(storage)
    x = torch.randn((B, H, W, ld_x), generator=torch.Generator().manual_seed(H)).to(sdt)
    out = torch.full((B, 2 * H, 2 * W, ld_o), float("nan"), dtype=sdt)
    od = out.to(DEV)
    _lib.check(lib.gyre_op_pixel_shuffle2(_st(), _p(x.to(DEV)), ld_x, B, H, W, Co, _p(od), ld_o), lib)
    torch.cuda.synchronize()
    got = od.cpu()
    assert torch.equal(R.bits(got[..., :Co]), R.bits(R.pixel_shuffle_nhwc(x[..., :4 * Co])))
    assert torch.equal(R.bits(got[..., Co:]), R.bits(out[..., Co:])), "columns past Co were touched"
