"""The kernels of the MLSD line detector (-m gpu; kernels_mlsd.hip) through their raw-operator entry points, on both storage flavours
in this process: each kernel alone against fp64 on the storage-rounded operands, element by element under the bound derived in
tests/mlsd_ref.py (half a storage ulp of the result plus the fp32 accumulation term of the operand magnitudes; held against seeded
mistakes in tests/test_mlsd_ref_host.py); non-finite inputs propagate as in torch; two runs give equal bits; a sample alone gives the
bits it gives inside a batch.  Shapes are the smallest at which each kernel can go wrong: one pixel, a stride-2 window that hangs over
the right / bottom edge (2x2 -> 1x1, 3x5), the first and the widest channel count, a dilation reaching past every edge (4x4: only the
centre tap is inside) and across several waves (11x13, batch 2: 286 pixels), odd image sides at the entry."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import mlsd_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
SIDS = ["bf16", "f16"]
NAN = float("nan")


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    """the device pointer of a tensor the CALLER keeps alive"""
    return None if t is None else C.c_void_p(t.data_ptr())


def wf_layout(wf, kind, O, I, taps, o_pad, i_pad, sdt):
    """the host fold's weights (mlsd_ref.fold) in the kernel's destination order"""
    if kind == 0:
        want = torch.zeros((o_pad, taps, i_pad), dtype=sdt)
        want[:O, :, :I] = wf.reshape(O, I, taps).permute(0, 2, 1)
        return want.reshape(-1)
    return (wf.reshape(O, 9).t() if kind == 1 else wf.permute(2, 3, 1, 0)).contiguous().reshape(-1)


def _dw(lib, xd, wd, bd, stride, rin):
    B, H, W, C_ = xd.shape
    y = torch.full((B, H // stride, W // stride, C_), NAN, dtype=xd.dtype, device=DEV)
    _lib.check(lib.gyre_op_dwconv3(_st(), _p(xd), B, H, W, C_, _p(wd), _p(bd), stride, rin, _p(y)), lib)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("C_", [32, 576])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 2), (3, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_depthwise(shape, C_, storage, sdt):
    lib = _lib.lib(storage)
    B, H, W = shape
    x, w, b = R.dw_case(sdt, B, H, W, C_)
    xd, wd, bd = x.to(DEV), w.reshape(C_, 9).t().contiguous().to(DEV), b.to(DEV)
    for stride in ((1,) if H < 2 else (1, 2)):
        for rin in (0, 1):
            ref, t = R.dw_ref(x, w, b, stride, bool(rin))
            got = _dw(lib, xd, wd, bd, stride, rin)
            worst = R.verdict(got, ref, R.stored_bound(ref, t, sdt))
            print(f"[mlsd] depthwise C {C_} {B}x{H}x{W} stride {stride} relu6_in {rin} {sdt}: worst |got - value64| / bound = {worst:.3f}")
            assert tuple(got.shape) == tuple(ref.shape) and worst <= 1.0
            assert torch.equal(R.bits(got), R.bits(_dw(lib, xd, wd, bd, stride, rin))), "two runs differ"
            if B > 1:
                one = _dw(lib, xd[1:2].contiguous(), wd, bd, stride, rin)
                assert torch.equal(R.bits(one), R.bits(got[1:2])), "sample 1 alone"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_depthwise_non_finite_and_refusals(storage, sdt):
    lib = _lib.lib(storage)
    x, w, b = R.dw_case(sdt, 1, 3, 5, 32)
    x[0, 1, 1, 0], x[0, 1, 3, 1], x[0, 0, 4, 2], x[0, 2, 0, 2] = NAN, float("inf"), float("-inf"), float("inf")
    want = F.relu6(F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding=1, groups=32)).permute(0, 2, 3, 1)
    got = _dw(lib, x.to(DEV), w.reshape(32, 9).t().contiguous().to(DEV), b.to(DEV), 1, 0).float()
    assert torch.isnan(want).any() and torch.equal(torch.isnan(got), torch.isnan(want))
    # where an infinity decided and no NaN: relu6(+-inf), 6 or 0, bit for bit
    hit = F.conv2d(torch.isinf(x).float().permute(0, 3, 1, 2), torch.ones((32, 1, 3, 3)), padding=1, groups=32).permute(0, 2, 3, 1) > 0
    hit &= ~torch.isnan(want)
    assert int(hit.sum()) > 0 and torch.equal(got[hit], want[hit]) and not bool(torch.isinf(got).any())
    xd, wd, bd = torch.zeros((1, 2, 2, 36), dtype=sdt, device=DEV), torch.zeros((9, 36), dtype=sdt, device=DEV), torch.zeros(36, device=DEV)
    y = torch.zeros((1, 2, 2, 36), dtype=sdt, device=DEV)
    with pytest.raises(NotImplementedError):                         # channels in eights
        _lib.check(lib.gyre_op_dwconv3(_st(), _p(xd), 1, 2, 2, 36, _p(wd), _p(bd), 1, 0, _p(y)), lib)
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_dwconv3(_st(), _p(xd), 1, 2, 2, 32, _p(wd), _p(bd), 3, 0, _p(y)), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_dwconv3(_st(), _p(xd), 1, 1, 2, 32, _p(wd), _p(bd), 2, 0, _p(y)), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_dwconv3(_st(), None, 1, 2, 2, 32, _p(wd), _p(bd), 1, 0, _p(y)), lib)


def _up(lib, xd, rin, ldy=128, off=64):
    B, H, W, C_ = xd.shape
    y = torch.full((B, 2 * H, 2 * W, ldy), NAN, dtype=xd.dtype, device=DEV)
    _lib.check(lib.gyre_op_upsample2_ac(_st(), _p(xd), B, H, W, C_, C_, rin, C.c_void_p(y.data_ptr() + 2 * off), ldy), lib)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_upsample(shape, storage, sdt):
    lib = _lib.lib(storage)
    x = R.up2_case(sdt, *shape)
    xd = x.to(DEV)
    for rin in (0, 1):
        ref, t = R.up2_ref(x, bool(rin))
        full = _up(lib, xd, rin)
        got = full[..., 64:]
        worst = R.verdict(got, ref, R.stored_bound(ref, t, sdt))
        print(f"[mlsd] upsample {shape} relu_in {rin} {sdt}: worst |got - value64| / bound = {worst:.3f}")
        assert worst <= 1.0
        assert bool(torch.isnan(full[..., :64].float()).all()), "channels [0, 64) of the concat buffer were written"
        assert torch.equal(R.bits(got), R.bits(_up(lib, xd, rin)[..., 64:])), "two runs differ"
        if shape[0] > 1:
            assert torch.equal(R.bits(_up(lib, xd[1:2].contiguous(), rin)[..., 64:]), R.bits(got[1:2])), "sample 1 alone"
    # the corners are copies (align_corners=True), whatever the size
    plain = _up(lib, xd, 0)[..., 64:]
    assert torch.equal(R.bits(plain[:, 0, 0]), R.bits(x[:, 0, 0])) and torch.equal(R.bits(plain[:, -1, -1]), R.bits(x[:, -1, -1]))


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_upsample_non_finite_and_refusals(storage, sdt):
    lib = _lib.lib(storage)
    x = R.up2_case(sdt, 1, 3, 5)
    # in the first source row, away from the last row / column: torch's own fp32 coordinate of the LAST output row may fall a hair
    # below the last source row and then reads the row above with a weight near 1e-7, which an infinity turns into a difference
    x[0, 0, 1, 0], x[0, 0, 2, 1] = NAN, float("inf")
    want = R.upsample2_ac(x.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    got = _up(lib, x.to(DEV), 0)[..., 64:].float()
    assert torch.isnan(want).any() and torch.isinf(want).any()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    xd = torch.zeros((1, 2, 2, 64), dtype=sdt, device=DEV)
    y = torch.zeros((1, 4, 4, 64), dtype=sdt, device=DEV)
    with pytest.raises(NotImplementedError):                         # a pixel stride below the channel count
        _lib.check(lib.gyre_op_upsample2_ac(_st(), _p(xd), 1, 2, 2, 64, 64, 0, _p(y), 32), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_upsample2_ac(_st(), _p(xd), 1, 0, 2, 64, 64, 0, _p(y), 64), lib)


def _dconv(lib, xd, wd, bd):
    y = torch.full(tuple(xd.shape), NAN, dtype=xd.dtype, device=DEV)
    B, H, W, _ = xd.shape
    _lib.check(lib.gyre_op_dconv3_d5(_st(), _p(xd), B, H, W, _p(wd), _p(bd), _p(y)), lib)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 11, 13)], ids=lambda s: "x".join(map(str, s)))
def test_dilated_convolution(shape, storage, sdt):
    lib = _lib.lib(storage)
    x, w, b = R.dconv_case(sdt, *shape)
    ref, t = R.dconv_ref(x, w, b)
    xd, wd, bd = x.to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), b.to(DEV)
    got = _dconv(lib, xd, wd, bd)
    worst = R.verdict(got, ref, R.stored_bound(ref, t, sdt))
    print(f"[mlsd] dilated convolution {shape} {sdt}: worst |got - value64| / bound = {worst:.3f}; {float((ref > 0).double().mean()):.0%} of the outputs above 0")
    assert worst <= 1.0
    assert torch.equal(R.bits(got), R.bits(_dconv(lib, xd, wd, bd))), "two runs differ"
    if shape[0] > 1:
        assert torch.equal(R.bits(_dconv(lib, xd[1:2].contiguous(), wd, bd)), R.bits(got[1:2])), "sample 1 alone"
        xn = x.clone()
        xn[1, 5, 6, 3] = NAN                                         # reaches the nine pixels whose taps read it, nothing else
        gn = _dconv(lib, xn.to(DEV), wd, bd).float()
        wn = F.relu(F.conv2d(xn.float().permute(0, 3, 1, 2), w.float(), b, padding=5, dilation=5)).permute(0, 2, 3, 1)
        assert int(torch.isnan(wn).any(-1).sum()) == 9 and torch.equal(torch.isnan(gn), torch.isnan(wn))
        assert torch.equal(R.bits(gn[~torch.isnan(wn)].to(sdt)), R.bits(got[~torch.isnan(wn)]))


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("idt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("hw", [(16, 16), (17, 49)], ids=lambda s: "x".join(map(str, s)))
def test_entry_convolution(hw, idt, storage, sdt):
    lib = _lib.lib(storage)
    H, W = hw
    x, w, b = R.entry_case(sdt, idt, 2, H, W)
    ref, t = R.entry_ref(x, w, b)
    xd, wd, bd = x.to(DEV), w.permute(2, 3, 1, 0).contiguous().to(DEV), b.to(DEV)

    def run(xx):
        y = torch.full((xx.shape[0], H // 2, W // 2, 32), NAN, dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_mlsd_entry(_st(), _p(xx), _lib.dtype_code(xx), xx.shape[0], H, W, _p(wd), _p(bd), _p(y)), lib)
        torch.cuda.synchronize()
        return y.cpu()

    got = run(xd)
    worst = R.verdict(got, ref, R.stored_bound(ref, t, sdt))
    print(f"[mlsd] entry {H}x{W} {idt} -> {sdt}: worst |got - value64| / bound = {worst:.3f}; {float((ref >= 6).double().mean()):.0%} at 6")
    assert worst <= 1.0 and torch.equal(R.bits(got), R.bits(run(xd)))
    assert torch.equal(R.bits(run(xd[1:2].contiguous())), R.bits(got[1:2])), "sample 1 alone"
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_mlsd_entry(_st(), _p(xd), 7, 2, H, W, _p(wd), _p(bd), _p(wd)), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_fold_activation_and_exit_kernels(storage, sdt):
    lib = _lib.lib(storage)
    g = torch.Generator().manual_seed(3)
    # BatchNorm fold, dense 1x1 with padding (24 -> 144 at pitches 32 / 160) and biased 3x3, depthwise, entry
    for kind, O, I, taps, o_pad, i_pad, has_bias in ((0, 144, 24, 1, 160, 32, False), (0, 64, 64, 9, 64, 64, True), (1, 96, 96, 9, 96, 96, False),
                                                      (2, 32, 4, 9, 32, 4, False)):
        k = 3 if taps == 9 else 1
        w = torch.randn((O, 1 if kind == 1 else I, k, k), generator=g)
        cb = torch.randn(O, generator=g) if has_bias else None
        gam, bet, mean, var = tuple(torch.randn(O, generator=g) for _ in range(3)) + (0.5 + torch.rand(O, generator=g),)
        wf, bf = R.fold(w, cb, gam, bet, mean, var, sdt)
        n_out = {0: o_pad * taps * i_pad, 1: 9 * o_pad, 2: 9 * I * o_pad}[kind]
        out = torch.full((n_out,), NAN, dtype=sdt, device=DEV)
        bias = torch.full((o_pad,), NAN, device=DEV)
        dev = [t.to(DEV) if t is not None else None for t in (w, cb, gam, bet, mean, var)]
        a = _lib.MlsdFoldArgs(w=dev[0].data_ptr(), conv_bias=dev[1].data_ptr() if has_bias else None, gamma=dev[2].data_ptr(), beta=dev[3].data_ptr(),
                              mean=dev[4].data_ptr(), var=dev[5].data_ptr(), out=out.data_ptr(), bias=bias.data_ptr(), kind=kind, O=O, I=I, taps=taps,
                              o_pad=o_pad, i_pad=i_pad)
        _lib.check(lib.gyre_op_mlsd_fold(_st(), C.byref(a)), lib)
        torch.cuda.synchronize()
        # s takes three fp32 roundings (add, sqrt, divide), the product a fourth: t = 4 E |w s|, then one rounding to storage
        s64 = gam.double() / torch.sqrt(var.double() + 1e-5)
        w64 = w.double() * s64.reshape(-1, 1, 1, 1)
        if kind == 0:
            ref = torch.zeros((o_pad, taps, i_pad), dtype=torch.float64)
            ref[:O, :, :I] = w64.reshape(O, I, taps).permute(0, 2, 1)
        elif kind == 1:
            ref = w64.reshape(O, 9).t().contiguous()
        else:
            ref = w64.permute(2, 3, 1, 0).contiguous()
        ref = ref.reshape(-1)
        worst = R.verdict(out.cpu(), ref, R.stored_bound(ref, 4 * R.E * ref.abs(), sdt))
        same = float((R.bits(out.cpu()) == R.bits(wf_layout(wf, kind, O, I, taps, o_pad, i_pad, sdt))).double().mean())
        print(f"[mlsd] fold kind {kind} {sdt}: worst |got - value64| / bound = {worst:.3f}; {same:.4%} of the bits equal the host fold's")
        assert worst <= 1.0 and bool((out.cpu().reshape(ref.shape)[ref == 0] == 0).all()), f"folded weights, kind {kind}"
        got_b = bias.cpu()
        mag = bet.double().abs() + (((cb.double() if has_bias else 0) - mean.double()) * s64).abs()
        assert bool((got_b[O:] == 0).all()) and bool(((got_b[:O].double() - bf.double()).abs() <= 8 * R.E * mag).all()), f"folded bias, kind {kind}"
    # in-place activation over a channel slice of a wider buffer; relu-then-add; the x[:, 7:] hand-off
    x = (torch.randn((37, 128), generator=g) * 5).to(sdt)
    x[3, 5], x[4, 6] = NAN, float("inf")
    for relu6 in (0, 1):
        xd = x.to(DEV)
        _lib.check(lib.gyre_op_mlsd_act(_st(), _p(xd), 37, 64, 128, relu6), lib)
        torch.cuda.synchronize()
        want = x.clone()
        want[:, :64] = (F.relu6 if relu6 else F.relu)(x[:, :64].float()).to(sdt)
        got, nan = xd.cpu(), torch.isnan(want)                        # (a NaN stays a NaN; its payload is not part of the contract)
        assert int(nan.sum()) == 1 and torch.equal(torch.isnan(got), nan) and torch.equal(R.bits(got)[~nan], R.bits(want)[~nan])
    y, r = (torch.randn((3, 5, 128), generator=g) * 2).to(sdt), (torch.randn((3, 5, 128), generator=g) * 2).to(sdt)
    yd = y.to(DEV)
    _lib.check(lib.gyre_op_mlsd_relu_add(_st(), _p(yd), _p(r.to(DEV)), y.numel()), lib)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(yd.cpu()), R.bits((F.relu(y.float()) + r.float()).to(sdt)))
    t16 = torch.randn((2, 3, 5, 16), generator=g).to(sdt)
    for odt in (torch.float32, sdt):
        out = torch.full((2, 9, 3, 5), NAN, dtype=odt, device=DEV)
        _lib.check(lib.gyre_op_mlsd_exit(_st(), _p(t16.to(DEV)), 2, 3, 5, _p(out), _lib.dtype_code(out)), lib)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), t16.permute(0, 3, 1, 2)[:, 7:].to(odt))
