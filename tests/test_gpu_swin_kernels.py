"""The kernels of the SwinIR upscaler (-m gpu; kernels_swin.hip) through their raw-operator entry points, on both storage flavours in
this process: the shifted-window attention gyre_op_win_attn (with gyre_op_win_bias), the live-channel LayerNorm gyre_op_ln_live, the
in-place GELU / leaky ReLU gyre_op_swin_act and the entry / exit passes.  Values, host emulation and the element-wise bound of the
attention: tests/swinir_ref.py (derived there, held against seeded mistakes in tests/test_swinir_ref_host.py); the LayerNorm bound is
that of tests/norm_fwd_ref.py (two-pass form)."""
import ctypes as C

import pytest
import torch

import gpu_util
import norm_fwd_ref as N
import swinir_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
IDS = ["-".join(map(str, c)) for c in R.CASES]


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_attn(L, lib, expect=None, **over):
    """one gyre_op_win_bias + gyre_op_win_attn call on the data of L (swinir_ref.case); returns the output buffer.  over: argument
    overrides for the refusal tests; expect: the exception type a refused call must raise (the buffer must then come back untouched)."""
    qkv, o, table = L["qkv"].to(DEV), L["o"].to(DEV), L["table"].contiguous().to(DEV)
    bias = torch.empty(L["heads"] * 4096, dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_win_bias(_st(), _p(table), L["heads"], _p(bias)), lib)
    a = dict(ld_qkv=qkv.shape[1], ld_o=o.shape[1], B=L["B"], H=L["H"], W=L["W"], heads=L["heads"], shift=L["shift"])
    a.update(over)
    rc = lib.gyre_op_win_attn(_st(), _p(qkv), a["ld_qkv"], _p(o), a["ld_o"], _p(bias), a["B"], a["H"], a["W"], a["heads"], a["shift"])
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
def test_win_attn_element_by_element(case, storage, sdt):
    L = R.case(sdt, *case)
    got = run_attn(L, _lib.lib(storage))
    n = 30 * L["heads"]
    assert bool(torch.isfinite(got[:, :n].float()).all()), "a live column was left unwritten"
    worst, rest = R.verdict(L, got)
    print(f"[swin] win_attn {sdt} {case}: worst |got - value64| / bound = {worst:.3f}")
    assert rest, "an element outside the live columns changed"
    assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
def test_win_bias_is_the_indexed_table(storage, sdt):
    """the expanded bias, read back through its documented order [head][query tile][key tile][reg >> 2][lane][reg & 3], is the table
    gathered by the reference's relative_position_index - exactly (fp32 copies)"""
    lib = _lib.lib(storage)
    table = torch.randn((225, 6), generator=torch.Generator().manual_seed(3))
    out = torch.empty(6 * 4096, dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_win_bias(_st(), _p(table.to(DEV)), 6, _p(out)), lib)
    torch.cuda.synchronize()
    got = out.cpu().view(6, 2, 2, 4, 64, 4)                     # h, qt, kt, g, lane, i
    want = R.expanded_bias(table)
    lane = torch.arange(64)
    a = (32 * torch.arange(2)[:, None, None, None, None] + (lane & 31)[None, None, None, :, None]).expand(2, 2, 4, 64, 4)
    b = (32 * torch.arange(2)[None, :, None, None, None] + 8 * torch.arange(4)[None, None, :, None, None]
         + 4 * (lane >> 5)[None, None, None, :, None] + torch.arange(4)[None, None, None, None, :]).expand(2, 2, 4, 64, 4)
    assert torch.equal(got, want[:, a, b])


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
def test_win_attn_refusals_write_nothing(storage, sdt):
    lib = _lib.lib(storage)
    L = R.case(sdt, 1, 16, 16, 2, 4)
    for over, exc in ((dict(H=12), ValueError), (dict(W=20), ValueError), (dict(H=0), ValueError), (dict(shift=2), NotImplementedError),
                      (dict(shift=8), NotImplementedError), (dict(heads=9), NotImplementedError), (dict(heads=0), NotImplementedError),
                      (dict(ld_qkv=100), ValueError), (dict(ld_o=40), ValueError), (dict(ld_qkv=196), NotImplementedError), (dict(B=0), ValueError)):
        run_attn(L, lib, expect=exc, **over)
    one = R.case(sdt, 1, 8, 16, 2, 0)
    run_attn(one, lib, expect=ValueError, shift=4)              # one window per side is not shifted


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("C_live,ld,M", [(60, 64, 37), (180, 192, 37), (240, 256, 37), (30, 40, 37), (30, 42, 37), (510, 512, 37),
                                         (60, 64, 2 * 16384 + 5), (30, 42, 16384 + 3)])
def test_ln_live_against_fp64(C_live, ld, M, storage, sdt):
    """statistics over the live channels only (NaN in the source padding must not leak), zeros written to the output padding; strides
    that are multiples of 4 take the 8-byte form of the kernel, 42 the element-wise one, 510 of 512 uses both channel quads of a lane;
    more than 16384 rows (the kernel's wave count) make a wave walk two or three rows"""
    lib = _lib.lib(storage)
    x, gamma, beta = N.ln_inputs(M, C_live, sdt, seed=C_live)
    x = x.to(sdt)
    src = torch.full((M, ld), float("nan"), dtype=sdt)
    src[:, :C_live] = x
    y = torch.full((M, ld), float("nan"), dtype=sdt, device=DEV)
    sd, g, b = src.to(DEV), gamma.float().to(DEV), beta.float().to(DEV)
    _lib.check(lib.gyre_op_ln_live(_st(), _p(sd), ld, M, C_live, _p(g), _p(b), 1e-5, _p(y), ld), lib)
    torch.cuda.synchronize()
    got = y.cpu()
    assert bool((got[:, C_live:].float() == 0).all()), "the padding channels must be written as zeros"
    ref, bound, tiny = N.ln_ref(x, gamma, beta, 1e-5)
    gpu_util.check_bound(f"ln_live C={C_live} {sdt}", got[:, :C_live], ref, bound, k=N.k_of(sdt), tiny=tiny, hdt=sdt)
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_ln_live(_st(), _p(sd), 640, M, 600, _p(g), _p(b), 1e-5, _p(y), 640), lib)     # (refused before any launch)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_ln_live(_st(), _p(sd), C_live - 1, M, C_live, _p(g), _p(b), 1e-5, _p(y), ld), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("mode,slope", [(0, 0.0), (1, 0.2), (1, 0.01)], ids=["gelu", "lrelu0.2", "lrelu0.01"])
def test_swin_act_against_fp64(mode, slope, storage, sdt):
    lib = _lib.lib(storage)
    n = 8 * 1031                                                # more than one block, not a multiple of the block
    x = (torch.randn(n, generator=torch.Generator().manual_seed(mode)) * 3).to(sdt)
    x[:16] = torch.tensor([0.0, -0.0, 1.0, -1.0, 6.0, -6.0, 12.0, -12.0, 1e-3, -1e-3, 0.5, -0.5, 2.0, -2.0, 30.0, -30.0]).to(sdt)
    buf = torch.cat([x, torch.full((8,), float("nan"), dtype=sdt)]).to(DEV)
    _lib.check(lib.gyre_op_swin_act(_st(), _p(buf), n, mode, slope), lib)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[n:].float()).all()), "elements past n were touched"
    ref, bd = R.act_bound(x, mode, slope)
    worst = float(((got[:n].double() - ref).abs() / bd).nan_to_num(nan=float("inf")).max())
    print(f"[swin] act mode {mode} slope {slope} {sdt}: worst ratio {worst:.3f}")
    assert worst <= 1.0
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_swin_act(_st(), _p(buf), n - 3, mode, slope), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_swin_act(_st(), _p(buf), n, 2, slope), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("img_range", [1.0, 255.0])
def test_entry_and_exit_against_fp64(img_range, storage, sdt):
    lib = _lib.lib(storage)
    B, HW = 2, 16 * 24 + 5
    mean = torch.tensor(R.MEAN, dtype=torch.float32)
    x = torch.rand((B, 3, HW), generator=torch.Generator().manual_seed(5))
    y = torch.full((B, HW, 8), float("nan"), dtype=sdt, device=DEV)
    xd = x.to(DEV)
    _lib.check(lib.gyre_op_swin_entry(_st(), _p(xd), 0, B, HW, _p(mean), img_range, _p(y)), lib)
    torch.cuda.synchronize()
    got = y.cpu()
    ref, bd = R.entry_ref(x, img_range, sdt)
    assert bool((got[..., 3:].float() == 0).all())
    worst = float(((got.double() - ref).abs() / bd.clamp_min(1e-300))[..., :3].nan_to_num(nan=float("inf")).max())
    print(f"[swin] entry range {img_range} {sdt}: worst ratio {worst:.3f}")
    assert worst <= 1.0
    for odt, code in ((torch.float32, 0), (sdt, _lib.BF16 if sdt == torch.bfloat16 else _lib.F16)):
        src = (torch.randn((B, HW, 8), generator=torch.Generator().manual_seed(6)) * img_range).to(sdt)
        src[..., 3:] = float("nan")
        out = torch.full((B, 3, HW), float("nan"), dtype=odt, device=DEV)
        sdv = src.to(DEV)
        _lib.check(lib.gyre_op_swin_exit(_st(), _p(sdv), 8, B, HW, _p(mean), img_range, _p(out), code), lib)
        torch.cuda.synchronize()
        ref, bd = R.exit_ref(src, img_range, odt)
        worst = float(((out.cpu().double() - ref).abs() / bd).nan_to_num(nan=float("inf")).max())
        print(f"[swin] exit range {img_range} {sdt} -> {odt}: worst ratio {worst:.3f}")
        assert worst <= 1.0
