"""The masked forms of the two hand-off kernels of the ControlNet path (-m gpu), through their raw-operator entry points, on both storage
flavours in this process:

  gyre_op_ctrl_emit_masked      out = rnd(fl(fl(scale f) m) [+ old]) - the residual hand-off of a masked hint (kernels_ctrl.hip)
  gyre_op_nchw_to_nhwc_masked   y = rnd(x m) - the entry pass of a control model next to a 9-channel inpaint UNet (kernels_elem.hip)

The reference is numpy float32 arithmetic on the storage-rounded inputs: every float32 product of numpy is the correctly rounded one,
which is what __fmul_rn is, so an assign is held to BIT equality (one more rounding for a 16-bit output).  An accumulate is held to the
bound tests/ctrl_ref.py derives for the unmasked kernel, widened by the one extra fp32 product: with mag = |scale f m| and E = scale f m
+ old exact,
    a = 2^-24 mag + 2^-24 |E| + 2^-149   (ctrl_ref.emit_bound)   +   2^-24 (1 + 2^-24) mag + 2^-149   (the second product, its denormal step)
    bound = a + u_out (|E| + a) + f_out.
Cpad: the next multiple of 8 and that plus 8 - the padded strides a zero convolution's output can have (the stride must be a multiple of
8, so "C + 8" is taken from the padded count; the two agree for every C that is a multiple of 8).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ctrl_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
HWS = [1, 63, 64, 65, 130]
CS = [1, 17, 64, 65, 320]
SOFT = 0.8 * float(torch.logspace(-1, 0, 13)[3])


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _np32(t):
    return t.float().numpy().astype(np.float32)


def make_mask(mB, HW, g):
    """values in [0, 1] with exact zeros and ones among them"""
    m = torch.rand((mB, HW), generator=g)
    pick = torch.rand((mB, HW), generator=g)
    m[pick < 0.2] = 0.0
    m[pick > 0.8] = 1.0
    return m


def emit_masked(L, f, C_, scale, accumulate, out, b0, mask):
    B, HW, Cpad = f.shape
    fd, od, md = f.to(DEV), out.to(DEV), mask.to(DEV)
    _lib.check(L.gyre_op_ctrl_emit_masked(_st(), _p(fd), B, C_, HW, Cpad, scale, int(accumulate), _p(od), _lib.dtype_code(od), od.shape[0], b0,
                                          _p(md), md.shape[0]), L)
    torch.cuda.synchronize()
    return od.cpu()


def emit_plain(L, f, C_, scale, accumulate, out, b0):
    B, HW, Cpad = f.shape
    fd, od = f.to(DEV), out.to(DEV)
    _lib.check(L.gyre_op_ctrl_emit(_st(), _p(fd), B, C_, HW, Cpad, scale, int(accumulate), _p(od), _lib.dtype_code(od), od.shape[0], b0), L)
    torch.cuda.synchronize()
    return od.cpu()


def products(f, C_, scale, mask):
    """fl(fl(scale f) m) as float32 [B][C][HW], numpy arithmetic"""
    fv = _np32(f)[:, :, :C_].transpose(0, 2, 1)
    m = _np32(mask)[:, None, :]
    return (np.float32(scale) * fv) * m


def cases():
    for HW in HWS:
        for C_ in CS:
            for Cpad in ((C_ + 7) // 8 * 8, (C_ + 7) // 8 * 8 + 8):
                for B in (1, 3):
                    for mB in sorted({1, B}):
                        yield HW, C_, Cpad, B, mB


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("out", ["f32", "storage", "other16"])
def test_emit_masked_assign_is_bit_equal(storage, sdt, out):
    L = _lib.lib(storage)
    odt = {"f32": torch.float32, "storage": sdt, "other16": torch.float16 if sdt == torch.bfloat16 else torch.bfloat16}[out]
    n = 0
    for HW, C_, Cpad, B, mB in cases():
        g = torch.Generator().manual_seed(HW * 1000 + C_ + Cpad + 7 * B + mB)
        f = torch.randn((B, HW, Cpad), generator=g).to(sdt)
        mask = make_mask(mB, HW, g)
        scale = (SOFT, -1.7)[n % 2]
        out_B, b0 = ((B, 0), (B + 2, 1), (2 * B, B))[n % 3]                     # the whole batch, a window inside, the upper half
        poison = torch.full((out_B, C_, HW), float("nan"), dtype=odt)
        got = emit_masked(L, f, C_, scale, False, poison, b0, mask)
        want = torch.zeros((out_B, C_, HW), dtype=odt)
        want[b0:b0 + B] = torch.from_numpy(products(f, C_, scale, mask)).to(odt)
        assert torch.equal(_bits(got), _bits(want)), (HW, C_, Cpad, B, mB, out_B, b0)
        outside = torch.cat([got[:b0], got[b0 + B:]])
        assert bool((outside == 0).all()) and not bool(torch.signbit(outside).any())
        n += 1
    assert n == 150                                                    # 5 HW x 5 C x 2 Cpad x (B = 1; B = 3 with mask_B 1 and 3)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("out", ["f32", "storage", "other16"])
def test_emit_masked_accumulate_within_the_bound(storage, sdt, out):
    L = _lib.lib(storage)
    odt = {"f32": torch.float32, "storage": sdt, "other16": torch.float16 if sdt == torch.bfloat16 else torch.bfloat16}[out]
    worst, n = 0.0, 0
    for HW, C_, Cpad, B, mB in cases():
        g = torch.Generator().manual_seed(HW * 1000 + C_ + Cpad + 7 * B + mB + 1)
        f = torch.randn((B, HW, Cpad), generator=g).to(sdt)
        mask = make_mask(mB, HW, g)
        scale = (SOFT, -1.7)[n % 2]
        out_B, b0 = ((B, 0), (B + 2, 1), (2 * B, B))[n % 3]
        old = torch.randn((out_B, C_, HW), generator=g).to(odt)
        got = emit_masked(L, f, C_, scale, True, old, b0, mask)
        assert torch.equal(_bits(got[:b0]), _bits(old[:b0])) and torch.equal(_bits(got[b0 + B:]), _bits(old[b0 + B:]))     # outside: untouched
        s = float(torch.tensor(scale, dtype=torch.float32))
        prod = s * f.double()[:, :, :C_].transpose(1, 2) * mask.double()[:, None, :]
        exact, mag = old.double().clone(), torch.zeros(old.shape, dtype=torch.float64)
        exact[b0:b0 + B] += prod
        mag[b0:b0 + B] = prod.abs()
        a = R.E32 * mag + R.E32 * exact.abs() + 2.0 ** -149 + R.E32 * (1 + R.E32) * mag + 2.0 ** -149
        a = torch.where(mag > 0, a, torch.zeros_like(a))
        bound = a + torch.where(mag > 0, R.UNIT[odt] * (exact.abs() + a) + R.FLOOR[odt], torch.zeros_like(a))
        ratio = float(((got.double() - exact).abs() / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (HW, C_, Cpad, B, mB, out_B, b0, ratio)
        n += 1
    print(f"[ctrl] emit_masked accumulate {sdt} -> {odt}: worst err / bound {worst:.3f} over {n} shapes")


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_emit_masked_ones_zeros_and_nan(storage, sdt, accumulate):
    L = _lib.lib(storage)
    for HW, C_, Cpad, B in ((65, 17, 24, 3), (130, 320, 328, 1), (1, 1, 8, 3)):
        g = torch.Generator().manual_seed(HW + C_)
        f = torch.randn((B, HW, Cpad), generator=g).to(sdt)
        for odt in (torch.float32, torch.bfloat16, torch.float16):
            old = torch.randn((B + 1, C_, HW), generator=g).to(odt)
            for mB in sorted({1, B}):
                ones = torch.ones((mB, HW))
                assert torch.equal(_bits(emit_masked(L, f, C_, SOFT, accumulate, old, 1, ones)), _bits(emit_plain(L, f, C_, SOFT, accumulate, old, 1)))
                got = emit_masked(L, f, C_, SOFT, accumulate, old, 1, torch.zeros((mB, HW)))
                if accumulate:
                    assert torch.equal(_bits(got), _bits(old))                               # old + (+-0) = old, bit for bit
                else:
                    assert bool((got == 0).all())
        # a NaN in f under m == 0 stays NaN; its neighbours under m == 0 are zero
        fn = f.clone()
        fn[0, 0, 0] = float("nan")
        got = emit_masked(L, fn, C_, 1.0, False, torch.zeros((B, C_, HW)), 0, torch.zeros((1, HW)))
        assert bool(torch.isnan(got[0, 0, 0])) and int(torch.isnan(got).sum()) == 1 and int((got != 0).sum()) == 1


def test_emit_masked_refuses_bad_arguments():
    L = _lib.lib(_lib.BF16)
    f = torch.zeros((2, 4, 8), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((2, 8, 4), dtype=torch.float32, device=DEV)
    m = torch.ones((2, 4), device=DEV)
    for mB in (0, 3):                                                  # a mask batch that is neither 1 nor B
        with pytest.raises(ValueError):
            _lib.check(L.gyre_op_ctrl_emit_masked(_st(), _p(f), 2, 8, 4, 8, 1.0, 0, _p(out), 0, 2, 0, _p(m), mB), L)
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_ctrl_emit_masked(_st(), _p(f), 2, 8, 4, 8, 1.0, 0, _p(out), 0, 2, 0, None, 1), L)
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_nchw_to_nhwc_masked(_st(), _p(out), 0, 2, 8, 4, 8, _p(m), 3, _p(f)), L)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("src", [torch.float32, torch.bfloat16, torch.float16])
def test_nchw_to_nhwc_masked_is_the_rounded_product(storage, sdt, src):
    L = _lib.lib(storage)
    B = 3
    for C_ in (4, 9):
        Cpad = (C_ + 7) // 8 * 8
        for HW in (1, 63, 64, 65):
            for mB in (1, B):
                g = torch.Generator().manual_seed(C_ * 100 + HW + mB)
                x = (torch.randn((B, C_, HW), generator=g) * 3).to(src)
                mask = make_mask(mB, HW, g)
                xd, md = x.to(DEV), mask.to(DEV)
                y = torch.full((B, HW, Cpad), float("nan"), dtype=sdt, device=DEV)
                _lib.check(L.gyre_op_nchw_to_nhwc_masked(_st(), _p(xd), _lib.dtype_code(xd), B, C_, HW, Cpad, _p(md), mB, _p(y)), L)
                torch.cuda.synchronize()
                want = torch.zeros((B, HW, Cpad), dtype=sdt)
                want[:, :, :C_] = torch.from_numpy(_np32(x) * _np32(mask)[:, None, :]).to(sdt).transpose(1, 2)
                assert torch.equal(_bits(y), _bits(want)), (C_, HW, mB)
                assert bool((y[:, :, C_:] == 0).all())                                       # pad channels
                ones = torch.ones((mB, HW), device=DEV)
                y1, y0 = torch.empty_like(y), torch.empty_like(y)
                _lib.check(L.gyre_op_nchw_to_nhwc_masked(_st(), _p(xd), _lib.dtype_code(xd), B, C_, HW, Cpad, _p(ones), mB, _p(y1)), L)
                _lib.check(L.gyre_op_nchw_to_nhwc(_st(), _p(xd), _lib.dtype_code(xd), B, C_, HW, Cpad, _p(y0)), L)
                torch.cuda.synchronize()
                assert torch.equal(_bits(y1), _bits(y0))
