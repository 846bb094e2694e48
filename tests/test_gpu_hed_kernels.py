"""The kernels of the HED edge detector (-m gpu; kernels_hed.hip) through their raw-operator entry points, on both storage flavours in
this process: the entry pass (exact), the stage tail (pooled output bit for bit, score within its derived bound, batch independence)
and the fuse kernel on every MODEL_CASES geometry.  Values, inputs and the element-wise bounds: tests/hed_ref.py (derived there, held
against seeded mistakes in tests/test_hed_ref_host.py)."""
import ctypes as C

import pytest
import torch

import hed_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
SIDS = ["bf16", "f16"]
_FUSE = {}


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    """the device pointer of a tensor the CALLER keeps alive"""
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("idt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_entry_is_exact(hw, idt, storage, sdt):
    lib = _lib.lib(storage)
    (H, W), B = hw, 2
    x = ((torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(H)) - 0.45) * 255).to(idt)
    xd = x.to(DEV)
    y = torch.full((B, H + 68, W + 68, 8), float("nan"), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_hed_entry(_st(), _p(xd), _lib.dtype_code(x), B, H, W, _p(y)), lib)
    torch.cuda.synchronize()
    want = torch.zeros((B, H + 68, W + 68, 8), dtype=sdt)
    want[:, 34:34 + H, 34:34 + W, :3] = x.float().to(sdt).permute(0, 2, 3, 1)
    assert torch.equal(R.bits(y.cpu()), R.bits(want))                # border and padding channels: +0 bit patterns


def _tail(lib, xd, wd, bd, pool):
    B, Hs, Ws, C_ = xd.shape
    po = torch.full((B, -(-Hs // 2), -(-Ws // 2), C_), float("nan"), dtype=xd.dtype, device=DEV) if pool else None
    so = torch.full((B, Hs, Ws), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_hed_tail(_st(), _p(xd), B, Hs, Ws, C_, _p(wd), _p(bd), _p(po), _p(so)), lib)
    torch.cuda.synchronize()
    return (po.cpu() if pool else None), so.cpu()


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("size", R.TAIL_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C_", R.TAIL_WIDTHS)
def test_tail(C_, size, storage, sdt):
    lib = _lib.lib(storage)
    Hs, Ws = size
    for B in R.TAIL_BATCHES:
        x, w, b = R.tail_case(sdt, B, Hs, Ws, C_)
        pooled, ref, bound = R.tail_ref(x, w, b)
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
        po, so = _tail(lib, xd, wd, bd, True)
        assert torch.equal(R.bits(po), R.bits(pooled)), "pooled output"
        worst = R.verdict(so, ref, bound)
        print(f"[hed] tail C {C_} {Hs}x{Ws} B {B} {sdt}: worst |score - value64| / bound = {worst:.3f}")
        assert worst <= 1.0
        none, so_only = _tail(lib, xd, wd, bd, False)                # stage 5: no pooled output, the same scores
        assert none is None and torch.equal(R.bits(so_only), R.bits(so))
        for i in range(B if B > 1 else 0):                           # a sample alone gives the bits it gives inside the batch
            p1, s1 = _tail(lib, xd[i:i + 1].contiguous(), wd, bd, True)
            assert torch.equal(R.bits(p1), R.bits(po[i:i + 1])) and torch.equal(R.bits(s1), R.bits(so[i:i + 1])), f"sample {i}"


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
def test_tail_refusals(storage, sdt):
    lib = _lib.lib(storage)
    x = torch.zeros((1, 2, 2, 96), dtype=sdt, device=DEV)
    w, b, so = torch.zeros(96, device=DEV), torch.zeros(1, device=DEV), torch.zeros((1, 2, 2), device=DEV)
    with pytest.raises(NotImplementedError):
        _lib.check(lib.gyre_op_hed_tail(_st(), _p(x), 1, 2, 2, 96, _p(w), _p(b), None, _p(so)), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_hed_tail(_st(), _p(x), 1, 0, 2, 64, _p(w), _p(b), None, _p(so)), lib)
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_hed_tail(_st(), _p(x), 1, 2, 2, 64, _p(w), _p(b), None, None), lib)


def _fuse_case(name):
    """inputs, fp64 reference and bound share of a MODEL_CASES geometry, computed once and shared"""
    if name not in _FUSE:
        so, wf, bf = R.fuse_case(name)
        _FUSE[name] = (so, wf, bf) + R.fuse_ref(so, wf, bf, *R.MODEL_CASES[name])
    return _FUSE[name]


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=SIDS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_fuse(name, storage, sdt):
    lib = _lib.lib(storage)
    H, W = R.MODEL_CASES[name]
    so, wf, bf, ref, t = _fuse_case(name)
    B = so[0].shape[0]
    sod, wfd, bfd = [s.to(DEV) for s in so], wf.to(DEV), bf.to(DEV)
    sizes, offs = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    geo = {}
    for n in (H, W):                                                 # the graph's own geometry is the reference's
        _lib.check(lib.gyre_hed_geometry(n, sizes, offs), lib)
        geo[n] = (list(sizes), list(offs))
        assert geo[n] == (R.stage_sizes(n), R.crop_offsets(n))
    for odt in (torch.float32, sdt):
        out = torch.full((6, B, 1, H, W), float("nan"), dtype=odt, device=DEV)
        a = _lib.HedFuseArgs(wf=wfd.data_ptr(), bf=bfd.data_ptr(), out=out.data_ptr(), out_dtype=_lib.dtype_code(out), B=B, H=H, W=W)
        for k in range(5):
            a.so[k], a.Hk[k], a.Wk[k], a.oy[k], a.ox[k] = sod[k].data_ptr(), geo[H][0][k], geo[W][0][k], geo[H][1][k], geo[W][1][k]
        _lib.check(lib.gyre_op_hed_fuse(_st(), C.byref(a)), lib)
        torch.cuda.synchronize()
        got = out.cpu()
        worst = [R.verdict(got[k], ref[k], R.stored_bound(ref[k], t[k], odt)) for k in range(6)]
        print(f"[hed] fuse {name} -> {odt}: worst |got - value64| / bound per map {[round(v, 3) for v in worst]}")
        assert max(worst) <= 1.0                                     # the layout too: map k of sample b at [k][b]
    a.oy[4] = a.oy[4] + 16 * (geo[H][0][4] + 1)                      # a crop window outside the upsampled map: refused, nothing read
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_op_hed_fuse(_st(), C.byref(a)), lib)


def test_geometry_hook_equals_the_stored_reference_geometry():
    """tests/golden/hed_vectors.npz: the reference's own stage sizes and crop offsets for sides 1 .. 80 (round-half-even on the host)"""
    import os

    import numpy as np
    stored = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hed_vectors.npz"))
    lib = _lib.lib(_lib.BF16)
    sizes, offs = (C.c_int32 * 5)(), (C.c_int32 * 5)()
    for n, s, o in zip(stored["sides"].tolist(), stored["stage_sizes"].tolist(), stored["crop_offsets"].tolist()):
        _lib.check(lib.gyre_hed_geometry(n, sizes, offs), lib)
        assert (list(sizes), list(offs)) == (s, o), n
    with pytest.raises(ValueError):
        _lib.check(lib.gyre_hed_geometry(0, sizes, offs), lib)
