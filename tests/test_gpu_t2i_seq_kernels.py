"""The kernels of the token-sequence T2I networks (-m gpu; kernels_seq.hip) through their raw-operator entry points, on both storage
flavours in this process: gyre_op_seq_attn, gyre_op_quick_gelu, gyre_op_fuser_pool and gyre_op_fuser_gain.  Values, host emulation and
the element-wise bounds: tests/t2i_seq_ref.py (derived there, held against seeded mistakes in tests/test_t2i_seq_host.py)."""
import ctypes as C

import pytest
import torch

import t2i_seq_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
SIDS = ["bf16", "f16"]


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_attn(c, lib, expect=None, **over):
    """one gyre_op_seq_attn call on the data of c (t2i_seq_ref.attn_case); returns the output buffer.  over: argument overrides for the
    refusal tests; expect: the exception type a refused call must raise (the buffer must then come back untouched)."""
    qkv, o = c["qkv"].to(DEV), c["o"].to(DEV)
    a = dict(ld_qkv=qkv.shape[1], ld_o=o.shape[1], N=c["N"], L=c["L"], heads=c["heads"], D=c["D"])
    a.update(over)
    rc = lib.gyre_op_seq_attn(_st(), _p(qkv), a["ld_qkv"], _p(o), a["ld_o"], a["N"], a["L"], a["heads"], a["D"])
    torch.cuda.synchronize()
    if expect is not None:
        with pytest.raises(expect):
            _lib.check(rc, lib)
        assert torch.equal(R.bits(o.cpu()), R.bits(c["o"])), "a refused call wrote to the output buffer"
        return None
    _lib.check(rc, lib)
    return o.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=["-".join(map(str, c)) for c in R.ATTN_CASES])
def test_seq_attn_element_by_element(case, storage, sdt):
    c = R.attn_case(sdt, *case)
    lib = _lib.lib(storage)
    got = run_attn(c, lib)
    rows, cols = c["N"] * c["L"], c["heads"] * c["D"]
    assert bool(torch.isfinite(got[:rows, :cols].float()).all()), "a live element was left unwritten, or padding reached a result"
    worst, rest = R.verdict(c, got)
    print(f"[t2i_seq] seq_attn {sdt} {case}: worst |got - value64| / bound = {worst:.3f}")
    assert rest, "an element outside the live rows and columns changed"
    assert worst <= 1.0
    assert torch.equal(R.bits(got), R.bits(run_attn(c, lib))), "two calls differ"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_seq_attn_limits_and_refusals_write_nothing(storage, sdt):
    lib = _lib.lib(storage)
    for D, want in R.MAX_LEN.items():
        assert lib.gyre_op_seq_attn_max_len(D) == want
    assert lib.gyre_op_seq_attn_max_len(40) == 0 and R.MAX_LEN[128] >= 265
    c = R.attn_case(sdt, 1, 1, R.MAX_LEN[128] + 1, 128)                # one token past what K and V of a head fit
    run_attn(c, lib, expect=NotImplementedError)
    c = R.attn_case(sdt, 2, 2, 4, 32)
    for over, exc in ((dict(D=40), NotImplementedError), (dict(D=0), NotImplementedError), (dict(D=160), NotImplementedError),
                      (dict(L=R.MAX_LEN[32] + 1), NotImplementedError), (dict(L=0), ValueError), (dict(N=0), ValueError),
                      (dict(heads=0), ValueError), (dict(ld_qkv=184), ValueError), (dict(ld_o=56), ValueError),
                      (dict(ld_qkv=196), NotImplementedError)):
        run_attn(c, lib, expect=exc, **over)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_quick_gelu_against_fp64(storage, sdt):
    lib = _lib.lib(storage)
    pts = R.quick_gelu_points(sdt)
    x = torch.cat([pts, torch.randn(4096, generator=torch.Generator().manual_seed(3)).mul(3).to(sdt)])       # (more than one block)
    buf = torch.cat([x, torch.full((8,), float("nan"), dtype=sdt)]).to(DEV)
    _lib.check(lib.gyre_op_quick_gelu(_st(), _p(buf), x.numel()), lib)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[x.numel():]).all()), "elements past n were written"
    got = got[:x.numel()]
    v, bd = R.quick_gelu_ref(x)
    worst = float(((got.double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    print(f"[t2i_seq] quick_gelu {sdt}: worst |got - value64| / bound = {worst:.3f}")
    assert bool(torch.isfinite(got.float()).all()), "an in-range value was lost"
    assert worst <= 1.0
    top = x.float().abs().max()                                         # the end of the range: y = x on the right, -0 on the left
    assert float(got[x.float() == top][0]) == float(top) and float(got[x.float() == -top][0]) == 0.0
    for n, exc in ((0, NotImplementedError), (12, NotImplementedError)):
        with pytest.raises(exc):
            _lib.check(lib.gyre_op_quick_gelu(_st(), _p(buf), n), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_quick_gelu(_st(), None, 8), lib)


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=["-".join(map(str, c)) for c in R.POOL_CASES])
def test_fuser_pool_against_fp64(case, storage, sdt):
    lib = _lib.lib(storage)
    N, C_, h, w = case
    x = R.pool_case(sdt, *case)
    ld = C_ + 5
    out = torch.full((N + 1, ld), float("nan"), dtype=sdt)
    od = out.to(DEV)
    xd = torch.cat([x.reshape(-1), torch.full((64,), float("nan"), dtype=sdt)]).to(DEV)      # NaN behind the last map
    _lib.check(lib.gyre_op_fuser_pool(_st(), _p(xd), N, C_, h * w, _p(od), ld), lib)
    torch.cuda.synchronize()
    got = od.cpu()
    v, bd = R.pool_ref(x)
    worst = float(((got[:N, :C_].double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    print(f"[t2i_seq] fuser_pool {sdt} {case}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert bool(torch.isnan(got[:N, C_:]).all()) and bool(torch.isnan(got[N:]).all()), "the pool wrote past its outputs"
    # the order of the sum depends on h w alone: the last sample alone gives the bits it gives in the batch, and so does a second call
    one, last = torch.full((1, ld), float("nan"), dtype=sdt).to(DEV), x[N - 1:].contiguous().to(DEV)
    _lib.check(lib.gyre_op_fuser_pool(_st(), _p(last), 1, C_, h * w, _p(one), ld), lib)
    again = out.to(DEV)
    _lib.check(lib.gyre_op_fuser_pool(_st(), _p(xd), N, C_, h * w, _p(again), ld), lib)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(one.cpu()[0, :C_]), R.bits(got[N - 1, :C_])) and torch.equal(R.bits(again.cpu()), R.bits(got))


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("case", [(2, 32, 3, 5), (1, 320, 8, 8), (3, 33, 1, 1)], ids=["2-32-3-5", "1-320-8-8", "3-33-1-1"])
def test_fuser_gain_is_the_fp32_expression_narrowed_once(case, storage, sdt):
    lib = _lib.lib(storage)
    N, C_, h, w = case
    g = torch.Generator().manual_seed(11 * N + C_ + h)
    x, x2 = R.pool_case(sdt, *case), R.pool_case(sdt, *case, seed=1)
    ld_a = C_ + 3
    alpha = torch.full((N, ld_a), float("nan"))
    alpha[:, :C_] = torch.randn((N, C_), generator=g) * 0.5
    a2 = torch.randn((N, ld_a), generator=g) * 0.5
    n = x.numel()
    od = torch.full((n + 16,), float("nan"), dtype=sdt).to(DEV)
    xg, x2g, ag, a2g, zg = x.to(DEV), x2.to(DEV), alpha.to(DEV), a2.to(DEV), torch.zeros((N, ld_a)).to(DEV)
    _lib.check(lib.gyre_op_fuser_gain(_st(), _p(xg), _p(ag), ld_a, N, C_, h * w, _p(od), 0), lib)
    torch.cuda.synchronize()
    first = od.cpu()
    want = R.gain_expr(x, alpha[:, :C_])
    assert torch.equal(R.bits(first[:n]), R.bits(want.reshape(-1))), "assign differs from fl(x fl(alpha + 1)) narrowed once"
    _lib.check(lib.gyre_op_fuser_gain(_st(), _p(x2g), _p(a2g), ld_a, N, C_, h * w, _p(od), 1), lib)
    torch.cuda.synchronize()
    second = od.cpu()
    want2 = R.gain_expr(x2, a2[:, :C_], out=want)
    assert torch.equal(R.bits(second[:n]), R.bits(want2.reshape(-1))), "accumulate differs from fl(out + fl(x fl(alpha + 1))) narrowed once"
    assert bool(torch.isnan(first[n:]).all()) and bool(torch.isnan(second[n:]).all()), "elements past the map were written"
    # alpha = 0 (the checkpoint's initial spatial_ch_projs) returns the input bit for bit
    _lib.check(lib.gyre_op_fuser_gain(_st(), _p(xg), _p(zg), ld_a, N, C_, h * w, _p(od), 0), lib)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(od.cpu()[:n]), R.bits(x.reshape(-1)))


def test_fuser_op_refusals():
    lib = _lib.lib(_lib.BF16)
    x = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, device=DEV)
    for args in ((None, 1, 8, 4, _p(x), 8), (_p(x), 0, 8, 4, _p(x), 8), (_p(x), 1, 0, 4, _p(x), 8), (_p(x), 1, 8, 0, _p(x), 8),
                 (_p(x), 1, 8, 4, _p(x), 7), (_p(x), 1, 8, 4, None, 8)):
        with pytest.raises(ValueError):
            _lib.check(lib.gyre_op_fuser_pool(_st(), *args), lib)
    for args in ((None, _p(f), 8, 1, 8, 4, _p(x), 0), (_p(x), None, 8, 1, 8, 4, _p(x), 0), (_p(x), _p(f), 7, 1, 8, 4, _p(x), 0),
                 (_p(x), _p(f), 8, 1, 8, 4, _p(x), 2), (_p(x), _p(f), 8, 0, 8, 4, _p(x), 0), (_p(x), _p(f), 8, 1, 8, 4, None, 0)):
        with pytest.raises(ValueError):
            _lib.check(lib.gyre_op_fuser_gain(_st(), *args), lib)
    torch.cuda.synchronize()
    assert not bool(x.any()) and not bool(f.any()), "a refused call wrote"
