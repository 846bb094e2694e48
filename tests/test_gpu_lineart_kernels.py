"""The kernels of the line-art hinter (-m gpu; kernels_inorm.hip) through their raw-operator entry points, on both storage flavours in
this process: the instance-normalisation statistics and apply passes in every mode, the sub-pixel weight composition, the transposed
convolution as the graph builds it (patch rows -> GEMM -> shuffled read), the two 7x7 convolutions, and the planner convolution in its
no-padding form over a reflect-padded image.  Values, inputs and the element-wise bounds: tests/lineart_ref.py (derived there, held
against seeded mistakes in tests/test_lineart_ref_host.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import lineart_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
SIDS = ["bf16", "f16"]
_INORM = {}


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    """the device pointer of a tensor the CALLER keeps alive (a temporary would hand its memory to the next allocation)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stats_of(lib, x, C_):
    """gyre_op_inorm_stats over x viewed as [B][rows][C_] -> [B, C_, 2] fp32 on the device"""
    B = x.shape[0]
    rows = x[0].numel() // C_
    part = torch.empty(max(1, lib.gyre_op_inorm_workspace(B, rows, C_)), dtype=torch.uint8, device=DEV)
    stats = torch.empty((B, C_, 2), dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_inorm_stats(_st(), _p(x), C_, B, rows, C_, R.EPS, _p(part), _p(stats)), lib)
    torch.cuda.synchronize()
    return stats


def apply_of(lib, x, stats, B, H, W, C_, shuffled=0, relu=0, res=None, res_pad=0, pad=0, patch=0):
    """gyre_op_inorm_apply -> the output tensor (on the device), allocated with the mode's shape and poisoned first"""
    shape = (B, H, W, 4 * C_) if patch else (B, H + 2 * pad, W + 2 * pad, C_)
    out = torch.full(shape, float("nan"), dtype=x.dtype, device=DEV)
    a = _lib.InormApplyArgs(x=x.data_ptr(), stats=stats.data_ptr(), res=None if res is None else res.data_ptr(), out=out.data_ptr(),
                            B=B, H=H, W=W, C=C_, shuffled=shuffled, relu=relu, res_pad=res_pad, pad=pad, patch=patch)
    _lib.check(lib.gyre_op_inorm_apply(_st(), C.byref(a)), lib)
    torch.cuda.synchronize()
    return out


def _identity_stats(B, C_):
    s = torch.zeros((B, C_, 2), dtype=torch.float32, device=DEV)
    s[..., 1] = 1.0
    return s


def _inorm(sdt, shape, family):
    """input, fp64 reference and bound of an INORM case, computed once and shared"""
    key = (sdt, shape, family)
    if key not in _INORM:
        x = R.inorm_input(sdt, *shape, family=family)
        _INORM[key] = (x,) + R.inorm_ref(x)
    return _INORM[key]


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("family", R.INORM_FAMILIES)
@pytest.mark.parametrize("shape", R.INORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inorm_statistics_and_plain_apply(shape, family, storage, sdt):
    lib = _lib.lib(storage)
    B, H, W, C_ = shape
    x, m, rstd, y, t = _inorm(sdt, shape, family)
    xd = x.to(DEV)
    stats = stats_of(lib, xd, C_)
    # the statistics themselves: fp32 mean and rstd against float64 within their own derived bounds
    m64, r64, _, dm, _, dr = (v.reshape(B, C_) for v in R.inorm_stats_ref(x))
    sc = stats.cpu().double()
    assert bool(torch.isfinite(sc).all())
    wm, wr = float(((sc[..., 0] - m64).abs() / dm).max()), float(((sc[..., 1] - r64).abs() / dr).max())
    got = apply_of(lib, xd, stats, B, H, W, C_).cpu()
    worst = R.verdict(got, y, R.stored_bound(y, t, sdt))
    print(f"[lineart] inorm {family} {shape} {sdt}: worst |got - value64| / bound = {worst:.3f} (mean {wm:.3f}, rstd {wr:.3f} of their bounds)")
    assert wm <= 1.0 and wr <= 1.0
    assert worst <= 1.0
    if family == "constant":                                      # variance 0: exact zeros, not eps-sized noise
        assert float(got[0, :, :, 0].float().abs().max()) == 0.0 and float(got[-1].float().abs().max()) == 0.0
    if B > 1:                                                     # a sample alone gives the bits it gives inside the batch
        for b in range(B):
            s1 = stats_of(lib, xd[b:b + 1].contiguous(), C_)
            assert torch.equal(s1.cpu().view(torch.int32), stats[b:b + 1].cpu().view(torch.int32)), f"statistics of sample {b}"
            one = apply_of(lib, xd[b:b + 1].contiguous(), s1, 1, H, W, C_).cpu()
            assert torch.equal(R.bits(one), R.bits(got[b:b + 1])), f"sample {b}"
    assert torch.equal(stats.cpu().view(torch.int32), stats_of(lib, xd, C_).cpu().view(torch.int32)), "two calls differ"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("shape", [(3, 13, 18, 64), (1, 4, 5, 256), (2, 6, 8, 64), (1, 96, 80, 128)], ids=lambda s: "x".join(map(str, s)))
def test_inorm_apply_modes(shape, storage, sdt):
    lib = _lib.lib(storage)
    B, H, W, C_ = shape
    x = R.inorm_input(sdt, *shape)
    _, _, y, t = R.inorm_ref(x)
    xd = x.to(DEV)
    stats = stats_of(lib, xd, C_)
    plain = apply_of(lib, xd, stats, B, H, W, C_).cpu()
    # ReLU: max(., 0) of the plain result, bit for bit
    relu = apply_of(lib, xd, stats, B, H, W, C_, relu=1).cpu()
    assert torch.equal(R.bits(relu), R.bits(torch.where(plain.float() > 0, plain, torch.zeros_like(plain))))
    # residual, stored with a border of 0 and of 1 pixel: against fp64 with one more fp32 rounding in the bound
    g = torch.Generator().manual_seed(5)
    r = torch.randn(shape, generator=g).to(sdt)
    ref = y + r.double()
    bound = R.stored_bound(ref, t + R.E * ref.abs(), sdt)
    for rp in (0, 1):
        rbuf = torch.randn((B, H + 2 * rp, W + 2 * rp, C_), generator=g).to(sdt)
        rbuf[:, rp:rp + H, rp:rp + W] = r
        got = apply_of(lib, xd, stats, B, H, W, C_, res=rbuf.to(DEV), res_pad=rp).cpu()
        worst = R.verdict(got, ref, bound)
        print(f"[lineart] apply + residual (border {rp}) {shape} {sdt}: worst ratio {worst:.3f}")
        assert worst <= 1.0
        if rp == 1:
            # the two launches a residual block closes with: the residual read from a pad-1 image while the result is written as the
            # next pad-1 image, or as the patch rows of the first transposed convolution - the plain result, laid out, bit for bit
            rd = rbuf.to(DEV)
            both = apply_of(lib, xd, stats, B, H, W, C_, res=rd, res_pad=1, pad=1).cpu()
            assert torch.equal(R.bits(both), R.bits(R.reflect_nhwc(got.float(), 1).to(sdt))), "residual + pad 1"
            both = apply_of(lib, xd, stats, B, H, W, C_, res=rd, res_pad=1, patch=1).cpu()
            assert torch.equal(R.bits(both), R.bits(R.patch_rows(got))), "residual + patch rows"
    # reflection-padded writes: the interior is the plain result and the border the interior values it mirrors, bit for bit
    for p in (1, 3):
        got = apply_of(lib, xd, stats, B, H, W, C_, relu=1, pad=p).cpu()
        assert torch.equal(R.bits(got), R.bits(R.reflect_nhwc(relu.float(), p).to(sdt))), f"pad {p}"
    # 2x2 patch rows with their zero edge
    got = apply_of(lib, xd, stats, B, H, W, C_, relu=1, patch=1).cpu()
    assert torch.equal(R.bits(got), R.bits(R.patch_rows(relu)))
    assert float(got[:, -1, :, 2 * C_:].float().abs().max()) == 0.0 and float(got[:, :, -1, C_:2 * C_].float().abs().max()) == 0.0
    assert float(got[:, :, -1, 3 * C_:].float().abs().max()) == 0.0
    # the shuffled read: the same image stored as [H / 2][W / 2][(a, b, C)] gives the same statistics input and the same outputs
    if H % 2 == 0 and W % 2 == 0:
        xs = R.shuffle_rows(x).contiguous().to(DEV)
        st2 = stats_of(lib, xs, C_)
        m2 = R.inorm_ref(x)[0].reshape(B, C_)
        assert float((st2[..., 0].cpu().double() - m2).abs().max()) <= float((t / R.inorm_ref(x)[1]).max()) + 8 * R.E * float(m2.abs().max())
        for kw in (dict(), dict(pad=3), dict(patch=1)):
            a = apply_of(lib, xs, st2, B, H, W, C_, shuffled=1, relu=1, **kw).cpu()
            b = apply_of(lib, xd, st2, B, H, W, C_, relu=1, **kw).cpu()
            assert torch.equal(R.bits(a), R.bits(b)), f"shuffled {kw}"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_inorm_refusals(storage, sdt):
    lib = _lib.lib(storage)
    x = R.inorm_input(sdt, 1, 4, 6, 64).to(DEV)
    stats = stats_of(lib, x, 64)
    for kw, exc in ((dict(pad=2), NotImplementedError), (dict(pad=1, patch=1), ValueError), (dict(shuffled=1, H=3, W=8), ValueError),
                    (dict(C_=96), NotImplementedError), (dict(pad=3, H=3, W=8), ValueError)):
        a = dict(B=1, H=4, W=6, C_=64)
        a.update(kw)
        with pytest.raises(exc):
            apply_of(lib, x, stats, **a)
    with pytest.raises(NotImplementedError):
        stats_of(lib, torch.zeros((1, 2, 2, 96), dtype=sdt, device=DEV), 96)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("widths", R.TCONV_WIDTHS, ids=lambda w: f"{w[0]}to{w[1]}")
def test_weight_composition_is_exact(widths, storage, sdt):
    lib = _lib.lib(storage)
    cin, cout = widths
    w = (torch.randn((cin, cout, 3, 3), generator=torch.Generator().manual_seed(cin)) / 24).to(sdt)
    for src in (w, w.float()):                                    # storage values from either dtype: moved, not rounded
        out = torch.full((4 * cout, 4 * cin), float("nan"), dtype=sdt, device=DEV)
        srcd = src.to(DEV)
        _lib.check(lib.gyre_op_tconv_compose(_st(), _p(srcd), _lib.dtype_code(src), cin, cout, _p(out)), lib)
        torch.cuda.synchronize()
        want = R.compose_tconv(w)
        assert torch.equal(R.bits(out.cpu()), R.bits(want))
        blocks = out.cpu().float().reshape(4, cout, 4, cin).abs().amax((1, 3))
        assert int((blocks == 0).sum()) == 7 and R.bits(out.cpu())[blocks.repeat_interleave(cout, 0).repeat_interleave(cin, 1) == 0].eq(0).all()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("widths", R.TCONV_WIDTHS, ids=lambda w: f"{w[0]}to{w[1]}")
@pytest.mark.parametrize("shape", R.TCONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transposed_conv_as_built(shape, widths, storage, sdt):
    lib = _lib.lib(storage)
    (B, H, W), (cin, cout) = shape, widths
    x, w, b = R.tconv_case(sdt, B, H, W, cin, cout)
    ref, t = R.tconv_ref(x, w, b)
    ident = _identity_stats(B, max(cin, cout))
    xd = x.to(DEV)
    rows = apply_of(lib, xd, ident[:, :cin].contiguous(), B, H, W, cin, patch=1)                     # (x - 0) * 1: the patch rows of x itself
    assert torch.equal(R.bits(rows.cpu()), R.bits(R.patch_rows(x)))
    wc, wd = torch.empty((4 * cout, 4 * cin), dtype=sdt, device=DEV), w.to(DEV)
    _lib.check(lib.gyre_op_tconv_compose(_st(), _p(wd), _lib.dtype_code(w), cin, cout, _p(wc)), lib)
    b4 = b.repeat(4).to(DEV)
    y = torch.empty((B, H, W, 4 * cout), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_linear(_st(), _p(rows), B * H * W, 4 * cin, _p(wc), 4 * cout, _p(b4), None, 0, _p(y)), lib)
    torch.cuda.synchronize()
    got = apply_of(lib, y, ident[:, :cout].contiguous(), B, 2 * H, 2 * W, cout, shuffled=1).cpu()   # the shuffled read, values untouched
    worst = R.verdict(got, ref, R.stored_bound(ref, t, sdt))
    print(f"[lineart] transposed conv {shape} {widths} {sdt}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("shape", R.CONV7_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv7_in(shape, storage, sdt):
    lib = _lib.lib(storage)
    B, H, W = shape
    x, w, b = R.conv7_in_case(sdt, B, H, W)
    ref, t = R.conv7_in_ref(x, w, b)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    x8 = torch.empty((B, H, W, 8), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_nchw_to_nhwc(_st(), _p(xd), _lib.dtype_code(x), B, 3, H * W, 8, _p(x8)), lib)
    scratch = torch.empty(64 * 49 * 8, dtype=sdt, device=DEV)
    out = torch.full((B, H, W, 64), float("nan"), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_conv7_in(_st(), _p(x8), B, H, W, _p(wd), _lib.dtype_code(w), _p(scratch), _p(bd), _p(out)), lib)
    torch.cuda.synchronize()
    worst = R.verdict(out.cpu(), ref, R.stored_bound(ref, t, sdt))
    print(f"[lineart] conv7_in {shape} {sdt}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0
    with pytest.raises(ValueError):                               # a side of 3 has nothing to mirror at padding 3
        _lib.check(lib.gyre_op_conv7_in(_st(), _p(x8), B, 3, W, _p(wd), _lib.dtype_code(w), _p(scratch), _p(bd), _p(out)), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("sigmoid", [0, 1])
@pytest.mark.parametrize("shape", R.CONV7_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv7_out(shape, sigmoid, storage, sdt):
    lib = _lib.lib(storage)
    B, H, W = shape
    xp, w, b = R.conv7_out_case(sdt, B, H, W)
    ref, t = R.conv7_out_ref(xp, w, b, sigmoid)
    scratch = torch.empty(49 * 64, dtype=sdt, device=DEV)
    xd, wd, bd = xp.to(DEV), w.to(DEV), b.to(DEV)
    for odt in (torch.float32, sdt):
        out = torch.full((B, 1, H, W), float("nan"), dtype=odt, device=DEV)
        _lib.check(lib.gyre_op_conv7_out(_st(), _p(xd), B, H, W, _p(wd), _lib.dtype_code(w), _p(scratch), _p(bd), sigmoid, _p(out),
                                         _lib.dtype_code(out)), lib)
        torch.cuda.synchronize()
        worst = R.verdict(out.cpu(), ref, R.stored_bound(ref, t, odt))
        print(f"[lineart] conv7_out {shape} sigmoid {sigmoid} {sdt} -> {odt}: worst |got - value64| / bound = {worst:.3f}")
        assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("hw", [(8, 8), (33, 20)], ids=lambda s: "x".join(map(str, s)))
def test_planner_conv_over_a_reflect_padded_image(hw, storage, sdt):
    """pad 0, stride 1, Ho = Hi - 2, Cin = Cout = 256: the form the residual blocks run, against the fp64 convolution of the same
    padded image without any padding of its own"""
    lib = _lib.lib(storage)
    H, W = hw
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn((2, H, W, 256), generator=g).to(sdt)
    xp = R.reflect_nhwc(x.float(), 1).to(sdt).contiguous()
    w = (torch.randn((256, 256, 3, 3), generator=g) / 48).to(sdt)
    b = torch.randn((256,), generator=g) * 0.05
    xd = xp.double().permute(0, 3, 1, 2)
    ref = F.conv2d(xd, w.double(), b.double()).permute(0, 2, 3, 1)
    t = (9 * 256 + 2) * R.E * F.conv2d(xd.abs(), w.double().abs(), b.double().abs()).permute(0, 2, 3, 1)
    wk = w.permute(0, 2, 3, 1).contiguous().to(DEV)                # the library's conv layout [Cout][3][3][Cin]
    y = torch.full((2, H, W, 256), float("nan"), dtype=sdt, device=DEV)
    xpd, bd = xp.to(DEV), b.to(DEV)
    _lib.check(lib.gyre_op_conv3x3_valid(_st(), _p(xpd), 2, H + 2, W + 2, 256, _p(wk), 256, _p(bd), _p(y)), lib)
    torch.cuda.synchronize()
    worst = R.verdict(y.cpu(), ref, R.stored_bound(ref, t, sdt))
    print(f"[lineart] planner conv over the padded {H + 2} x {W + 2} image {sdt}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0
