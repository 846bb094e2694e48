"""The two element-wise kernels of the ControlNet path (-m gpu; kernels_ctrl.hip) through their raw-operator entry points, on both
storage flavours in this process: gyre_op_ctrl_emit - the scaled, accumulating, batch-offset NHWC -> NCHW hand-off to the UNet's
residual inputs - and gyre_op_silu.  Values, host emulation and the element-wise bounds: tests/ctrl_ref.py (derived there, and held
against seeded mistakes in tests/test_ctrl_host.py)."""
import ctypes as C

import pytest
import torch

import ctrl_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
EMIT_SHAPES = [(2, 32, 32, 6), (3, 20, 24, 35), (1, 320, 320, 64), (2, 1280, 1280, 1)]      # (B, C, Cpad, HW)
SOFT = 0.8 * float(torch.logspace(-1, 0, 13)[3])


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def emit(L, f, C_, scale, accumulate, out, b0):
    B, HW, Cpad = f.shape
    fd, od = f.to(DEV), out.to(DEV)
    _lib.check(L.gyre_op_ctrl_emit(_st(), _p(fd), B, C_, HW, Cpad, scale, int(accumulate), _p(od), _lib.dtype_code(od), od.shape[0], b0), L)
    torch.cuda.synchronize()
    return od.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("shape", EMIT_SHAPES)
@pytest.mark.parametrize("out_f32", [True, False])
def test_ctrl_emit_assign(storage, sdt, shape, out_f32):
    L = _lib.lib(storage)
    B, C_, Cpad, HW = shape
    odt = torch.float32 if out_f32 else sdt
    f = torch.randn((B, HW, Cpad), generator=torch.Generator().manual_seed(HW + C_)).to(sdt)
    poison = torch.full((2 * B, C_, HW), float("nan"), dtype=odt)
    for scale in (1.0, 0.5, 0.0):                                     # exact products: bit for bit the host's
        got = emit(L, f, C_, scale, False, poison, B)
        assert bool((got[:B] == 0).all()) and not bool(torch.signbit(got[:B]).any())
        assert torch.equal(_bits(got), _bits(R.emit_host(f, C_, scale, False, poison, B))), (shape, scale)
    for scale in (-1.7, SOFT):
        got = emit(L, f, C_, scale, False, poison, B)
        assert bool((got[:B] == 0).all())
        exact, mag = R.emit_exact(f, C_, scale, False, poison, B)
        ratio = float(((got.double() - exact).abs() / R.emit_bound(exact, mag, odt, False).clamp_min(1e-300)).max())
        print(f"[ctrl] emit assign {shape} {sdt} -> {odt} scale {scale:.4f}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0
        assert torch.equal(_bits(got), _bits(emit(L, f, C_, scale, False, poison, B)))          # two launches agree bitwise


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("shape", EMIT_SHAPES)
@pytest.mark.parametrize("out_f32", [True, False])
def test_ctrl_emit_accumulate(storage, sdt, shape, out_f32):
    L = _lib.lib(storage)
    B, C_, Cpad, HW = shape
    odt = torch.float32 if out_f32 else sdt
    g = torch.Generator().manual_seed(HW * 7 + C_)
    f = torch.randn((B, HW, Cpad), generator=g).to(sdt)
    old = torch.randn((B + 2, C_, HW), generator=g).to(odt)
    for scale in (1.0, -1.7, SOFT):
        got = emit(L, f, C_, scale, True, old, 1)
        assert torch.equal(_bits(got[:1]), _bits(old[:1])) and torch.equal(_bits(got[B + 1:]), _bits(old[B + 1:]))    # outside: untouched
        exact, mag = R.emit_exact(f, C_, scale, True, old, 1)
        ratio = float(((got.double() - exact).abs() / R.emit_bound(exact, mag, odt, True).clamp_min(1e-300)).max())
        print(f"[ctrl] emit accumulate {shape} {sdt} -> {odt} scale {scale:.4f}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0
        assert torch.equal(_bits(got), _bits(emit(L, f, C_, scale, True, old, 1)))


def test_ctrl_emit_refuses_bad_arguments():
    L = _lib.lib(_lib.BF16)
    f = torch.zeros((1, 4, 8), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((2, 8, 4), dtype=torch.float32, device=DEV)
    for args in ((1, 8, 4, 8, 1.0, 0, 2, 2), (1, 9, 4, 8, 1.0, 0, 2, 0), (1, 8, 4, 12, 1.0, 0, 2, 0), (1, 8, 4, 8, 1.0, 0, 2, -1)):
        B, C_, HW, Cpad, scale, acc, oB, b0 = args
        with pytest.raises(ValueError):
            _lib.check(L.gyre_op_ctrl_emit(_st(), _p(f), B, C_, HW, Cpad, scale, acc, _p(out), 0, oB, b0), L)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("n", [8, 8 * 1031])
def test_silu_against_float64(storage, sdt, n):
    L = _lib.lib(storage)
    x = R.silu_inputs(n, sdt, seed=n)
    y = x.clone().to(DEV)
    _lib.check(L.gyre_op_silu(_st(), _p(y), n), L)
    torch.cuda.synchronize()
    ratio, nan_kept, finite = R.silu_check(x, y.cpu())
    print(f"[ctrl] silu n={n} {sdt}: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0 and nan_kept and finite
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_silu(_st(), _p(y), n - 1), L)
