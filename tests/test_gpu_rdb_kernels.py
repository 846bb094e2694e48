"""The kernels of the RRDBNet upscaler (-m gpu; kernels_rdb.hip) through their raw-operator entry points, on both storage flavours in
this process: the dense-block convolution gyre_op_rdb_conv, the in-place epilogue gyre_op_rdb_epilogue and gyre_op_pixel_unshuffle.
Values, host emulation and the element-wise bound: tests/rrdb_ref.py (derived there, held against seeded mistakes in
tests/test_rrdb_ref_host.py)."""
import ctypes as C

import pytest
import torch

import rrdb_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
# (Cin, NT, live, ldo, c0, form, ups): prefixes 32 .. 192 of a 192-channel source, N = 32 into slice 64 of 192, N = 64 into a 64-channel
# buffer and into slice 0 of 192, conv_last's 3 live channels, the upsampling gather for N = 64, the five residual forms
CASES = [(32, 32, 32, 192, 64, "act", 0), (64, 32, 32, 192, 64, "plain", 0), (96, 32, 32, 192, 64, "plus", 0), (192, 32, 32, 192, 64, "act", 0),
         (192, 64, 64, 64, 0, "block", 0), (192, 64, 64, 192, 0, "rrdb", 0), (64, 64, 64, 64, 0, "body", 0), (64, 64, 64, 64, 0, "act", 1),
         (96, 64, 64, 192, 0, "block", 1), (64, 32, 3, 8, 0, "plain", 0), (64, 32, 3, 8, 0, "act", 1)]
IDS = [f"cin{c[0]}-n{c[1]}-live{c[2]}-ldo{c[3]}-c{c[4]}-{c[5]}-ups{c[6]}" for c in CASES]


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def tile_geometry():
    th, tw = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib(_lib.BF16).gyre_op_rdb_tile(C.byref(th), C.byref(tw)))
    return th.value, tw.value


def sizes():
    th, tw = tile_geometry()
    return [(1, 1), (th - 1, tw + 1), (th, tw), (th + 1, 2 * tw + 1)]


def _resid(r, ld):
    """a residual [.., live] inside a NaN buffer of pixel stride ld, on the device"""
    if r is None:
        return None
    base = torch.full(r.shape[:-1] + (ld,), float("nan"), dtype=r.dtype)
    base[..., :r.shape[-1]] = r
    return base.to(DEV)


def run_conv(L, lib, expect=None, epi_over=None, **over):
    """one gyre_op_rdb_conv call on the data of L (rrdb_ref.launch); returns the output buffer.  over: argument overrides for the
    refusal tests; expect: the exception type a refused call must raise (the buffer must then come back untouched)."""
    sdt = L["out"].dtype
    x, w, out = L["x"].to(DEV), L["w"].contiguous().to(DEV), L["out"].to(DEV)
    bias = L["bias"].to(DEV)
    B, H, W, ldx = x.shape
    live = L["live"]
    r1 = None if L["alias"] else _resid(L["r1"], 192 if L["r2"] is not None else max(64, live))
    r2 = _resid(L["r2"], 64)
    epi = _lib.RdbEpilogue()
    epi.bias, epi.alpha, epi.act = bias.data_ptr(), L["alpha"], L["act"]
    if L["alias"]:
        epi.r1, epi.ldr1, epi.beta1 = out.data_ptr() + 2 * L["c0"], out.shape[-1], L["beta1"]
    elif r1 is not None:
        epi.r1, epi.ldr1, epi.beta1 = r1.data_ptr(), r1.shape[-1], L["beta1"]
    if r2 is not None:
        epi.r2, epi.ldr2, epi.beta2 = r2.data_ptr(), r2.shape[-1], L["beta2"]
    for k, v in (epi_over or {}).items():
        setattr(epi, k, v)
    wpack = torch.full((L["NT"] * 9 * L["Cin"],), 7.0, dtype=sdt, device=DEV)
    a = _lib.RdbConvArgs()
    a.x, a.ldx, a.Cin, a.B, a.H, a.W, a.ups = x.data_ptr(), ldx, L["Cin"], B, H, W, L["ups"]
    a.w, a.w_rows, a.NT, a.N_live = w.data_ptr(), L["NT"], L["NT"], live
    a.out, a.c0, a.ldo, a.epi = out.data_ptr(), L["c0"], out.shape[-1], C.pointer(epi)
    a.wpack, a.wpack_bytes = wpack.data_ptr(), wpack.numel() * 2
    for k, v in over.items():
        setattr(a, k, v)
    rc = lib.gyre_op_rdb_conv(_st(), C.byref(a))
    torch.cuda.synchronize()
    if expect is not None:
        with pytest.raises(expect):
            _lib.check(rc, lib)
        assert torch.equal(R.bits(out.cpu()), R.bits(L["out"])), "a refused call wrote to the output buffer"
        assert bool((wpack == 7.0).all()), "a refused call wrote to the weight scratch"
        return None
    _lib.check(rc, lib)
    return out.cpu()


def _launch(sdt, case, H, W, B=2, **kw):
    Cin, NT, live, ldo, c0, form, ups = case
    return R.launch(sdt, B, H, W, Cin, NT, live, 192, ldo, c0, form=form, ups=ups, **kw)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rdb_conv_lattice_is_bit_exact(storage, sdt, case):
    lib = _lib.lib(storage)
    for H, W in sizes():
        L = _launch(sdt, case, H, W, lattice=True)
        got = run_conv(L, lib)
        s = slice(L["c0"], L["c0"] + L["live"])
        assert torch.equal(R.bits(got[..., s]), R.bits(R.lattice_expected(L))), (case, H, W)
        assert R.verdict(L, got)[1], "bytes outside the slice changed"


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rdb_conv_random_within_bound(storage, sdt, case):
    lib = _lib.lib(storage)
    for H, W in sizes():
        L = _launch(sdt, case, H, W)
        got = run_conv(L, lib)
        worst, rest = R.verdict(L, got)
        print(f"[rdb] conv {IDS[CASES.index(case)]} {H}x{W} {sdt}: worst err / bound {worst:.3f}")
        assert worst <= 1.0, (case, H, W, worst)
        assert rest, "bytes outside the written slice changed"
        assert torch.equal(R.bits(got), R.bits(run_conv(L, lib))), "two launches differ"


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("case", [CASES[2], CASES[5], CASES[8]], ids=[IDS[2], IDS[5], IDS[8]])
def test_rdb_conv_is_batch_independent(storage, sdt, case):
    lib = _lib.lib(storage)
    th, tw = tile_geometry()
    L3 = _launch(sdt, case, th + 1, tw + 1, B=3)
    L1 = dict(L3)
    for k in ("x", "out", "r1", "r2"):
        if torch.is_tensor(L3[k]):
            L1[k] = L3[k][1:2].clone()
    assert torch.equal(R.bits(run_conv(L3, lib)[1:2]), R.bits(run_conv(L1, lib)))


def test_rdb_conv_refusals_write_nothing():
    lib = _lib.lib(_lib.BF16)
    L = _launch(torch.bfloat16, CASES[0], 5, 7)
    for over in (dict(NT=48), dict(Cin=40), dict(ldx=196), dict(c0=68), dict(ldo=196), dict(B=65536)):
        run_conv(L, lib, expect=NotImplementedError, **over)
    for over in (dict(N_live=0), dict(N_live=33), dict(ldo=80), dict(x=None), dict(out=None), dict(wpack=None), dict(B=0), dict(H=0), dict(ldx=16),
                 dict(w_rows=0), dict(Cin=0)):
        run_conv(L, lib, expect=ValueError, **over)
    run_conv(L, lib, expect=_lib.GyreError, wpack_bytes=64)
    # the epilogue's own refusals come before the weight scratch is written, too
    Lr = _launch(torch.bfloat16, CASES[4], 5, 7)                     # the block form: a residual r1
    for eo in (dict(alpha=float("nan")), dict(beta1=float("inf")), dict(ldr1=32)):
        run_conv(Lr, lib, expect=ValueError, epi_over=eo)
    run_conv(Lr, lib, expect=NotImplementedError, epi_over=dict(ldr1=68))


EPI_FORMS = [(32, 64, 192, 0.2, 1, 1.0, None), (64, 0, 64, 0.04, 0, 0.2, 1.0), (3, 0, 8, 1.0, 1, None, None), (32, 96, 192, 1.0, 1, 1.0, None),
             (64, 0, 192, 1.0, 0, 1.0, None)]


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("form", EPI_FORMS)
def test_rdb_epilogue_matches_host_bitwise(storage, sdt, form):
    lib = _lib.lib(storage)
    live, c0, ldo, alpha, act, beta1, beta2 = form
    g = torch.Generator().manual_seed(live + c0 + ldo)
    npix = 2 * 37 * 5
    buf = torch.randn((npix, ldo), generator=g).to(sdt)
    buf[0, c0] = float("nan")
    r1 = torch.randn((npix, live), generator=g).to(sdt) if beta1 is not None else None
    r2 = torch.randn((npix, live), generator=g).to(sdt) if beta2 is not None else None
    bias = torch.randn(live, generator=g)
    for with_bias in (False, True):
        want = R.epilogue_inplace(buf, c0, live, bias if with_bias else None, alpha, act, r1, beta1 or 0.0, r2, beta2 or 0.0)
        d, db = buf.to(DEV), bias.to(DEV)
        d1, d2 = _resid(r1, 64), _resid(r2, 64)
        epi = _lib.RdbEpilogue()
        epi.bias, epi.alpha, epi.act = (db.data_ptr() if with_bias else None), alpha, act
        if d1 is not None:
            epi.r1, epi.ldr1, epi.beta1 = d1.data_ptr(), 64, beta1
        if d2 is not None:
            epi.r2, epi.ldr2, epi.beta2 = d2.data_ptr(), 64, beta2
        _lib.check(lib.gyre_op_rdb_epilogue(_st(), C.c_void_p(d.data_ptr()), c0, ldo, live, npix, C.byref(epi)), lib)
        torch.cuda.synchronize()
        got = d.cpu()
        assert bool(torch.isnan(got[0, c0])) and bool(torch.isnan(want[0, c0]))        # NaN stays NaN (its payload is not compared)
        got[0, c0] = want[0, c0] = 0
        diff = (R.bits(got) != R.bits(want)).nonzero()
        if len(diff):
            i = tuple(diff[0].tolist())
            print(f"[rdb] epilogue {form} {sdt}: {len(diff)} elements differ, first at {i}: got {float(got[i])!r} want {float(want[i])!r} in {float(buf[i])!r}")
        assert len(diff) == 0, form
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_rdb_epilogue(_st(), C.c_void_p(d.data_ptr()), c0 + 4, ldo, 1, npix, C.byref(epi)), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_rdb_epilogue(_st(), C.c_void_p(d.data_ptr()), c0, ldo, ldo + 8, npix, C.byref(epi)), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("r", [1, 2, 4])
def test_pixel_unshuffle_is_exact(storage, sdt, r):
    lib = _lib.lib(storage)
    for idt in (torch.float32, torch.bfloat16, torch.float16):
        for B, c, H, W in ((2, 3, 8, 12), (1, 4, 36, 20)):
            x = torch.randn((B, c, H, W), generator=torch.Generator().manual_seed(H + r)).to(idt)
            want = R.unshuffle(x, r, sdt)
            y = torch.full(want.shape, float("nan"), dtype=sdt, device=DEV)
            xd = x.to(DEV)
            _lib.check(lib.gyre_op_pixel_unshuffle(_st(), C.c_void_p(xd.data_ptr()), _lib.dtype_code(xd), B, c, H, W, r, C.c_void_p(y.data_ptr())), lib)
            torch.cuda.synchronize()
            assert torch.equal(R.bits(y.cpu()), R.bits(want)), (idt, r)
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_pixel_unshuffle(_st(), C.c_void_p(xd.data_ptr()), 0, 1, 3, 8, 12, 3, C.c_void_p(y.data_ptr())), lib)
    if r > 1:
        with pytest.raises(ValueError):
            _lib.check(lib.gyre_op_pixel_unshuffle(_st(), C.c_void_p(xd.data_ptr()), 0, 1, 3, 9, 12, r, C.c_void_p(y.data_ptr())), lib)
