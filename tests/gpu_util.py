"""Helpers for the -m gpu parity tests: call libgyre_hip through its C ABI on torch-allocated
device buffers and compare with fp32 ATen references."""
import ctypes as C

import torch

from gyre_amd import _lib

DEV = "cuda:0"
# the 16-bit storage dtype of the library flavour under test: bfloat16, or float16 when the suite runs with GYRE_STORAGE=f16
# (tests/test_gpu_f16_flavour.py re-runs the operator / model parity files that way)
HDT = _lib.STORAGE_TORCH_DTYPE[_lib.default_storage()]


_KEEP = []  # device tensors whose raw pointers were handed to the library; cleared (after a sync) per test


def vp(t):
    if t is None:
        return None
    _KEEP.append(t)  # the C ABI sees raw pointers only: keep the tensor alive until the kernel has run
    return C.c_void_p(t.data_ptr())


def release_kept():
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def report(name, got, ref, tol):
    e = rel_l2(got, ref)
    d = (got.double().cpu() - ref.double().cpu()).abs()
    print(f"[parity] {name}: rel_l2={e:.3e} max_abs={float(d.max()):.3e} ref_absmax={float(ref.abs().max()):.3e} tol={tol}")
    if not e <= tol:
        idx = int(d.flatten().argmax())
        print(f"   worst at flat index {idx}: got {float(got.flatten()[idx]):.5f} ref {float(ref.flatten()[idx]):.5f}")
        # error distribution along the last axis helps to spot layout bugs
        if d.ndim >= 2:
            print("   per-last-axis mean abs err (first 16):", d.reshape(-1, d.shape[-1]).mean(0)[:16].tolist())
    assert e <= tol, f"{name}: rel_l2 {e:.3e} > {tol}"


def check_bound(name, got, ref, bound, k=4.0, tiny=0.0, dims=None, hdt=None, enforce=True):
    """Element-wise  |got - ref| <= k u bound + u |ref| + tiny  (u = unit roundoff of the 16-bit storage, HDT: 2^-8 bf16, 2^-11
    fp16; 2^-24 for hdt = torch.float32, an output that is stored unrounded); bound = the float64 absolute-value form of the same
    computation, tiny an absolute floor (scalar or tensor).  Prints the
    worst ratio |got - ref| / tolerance and where it is (dims names the axes), pass or fail; NaN / inf in got fails.  hdt: judge for
    that storage type instead of the flavour under test (host self-tests of an error model); enforce = False: return the ratio
    without asserting (seeded mistakes that are meant to exceed it)."""
    hdt = HDT if hdt is None else hdt
    u = 2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -24 if hdt == torch.float32 else 2.0 ** -11
    g, r, b = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    tiny = tiny.double().cpu() if torch.is_tensor(tiny) else tiny
    # half the smallest subnormal: the output's own rounding floor
    floor = 2.0 ** -134 if hdt == torch.bfloat16 else 2.0 ** -150 if hdt == torch.float32 else 2.0 ** -25
    tol = k * u * b + u * r.abs() + tiny + floor
    ratio = ((g - r).abs() / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf"))
    flat = int(ratio.flatten().argmax())
    worst = float(ratio.flatten()[flat])
    idx = list(zip(dims, _unravel(flat, ratio.shape))) if dims else _unravel(flat, ratio.shape)
    print(f"[bound] {name}: worst ratio {worst:.3g} (k={k}) at {idx}: got {float(g.flatten()[flat]):.6g} "
          f"ref {float(r.flatten()[flat]):.6g} bound {float(b.flatten()[flat]):.6g}")
    assert worst <= 1.0 or not enforce, f"{name}: |got - ref| exceeds k u bound + u |ref| + tiny by {worst:.3g}x at {idx}"
    return worst


def _unravel(flat, shape):
    out = []
    for n in reversed(shape):
        out.append(flat % n)
        flat //= n
    return tuple(reversed(out))


def bf16_round(t):
    """Round to the library's 16-bit storage dtype (HDT: bf16, or fp16 for the fp16 flavour) and back."""
    return t.to(HDT).to(torch.float32)


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def repack_conv(w_oihw: torch.Tensor, cin_pad=None) -> torch.Tensor:
    L = _lib.lib()
    O, I, KH, KW = w_oihw.shape
    cin_pad = cin_pad or (I + 7) // 8 * 8
    src = w_oihw.float().contiguous().to(DEV)
    out = torch.zeros(O * KH * KW * cin_pad, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_repack_conv_weight(st(), vp(src), O, I, KH, KW, cin_pad, vp(out)))
    return out


def repack_linear(w: torch.Tensor, geglu=False) -> torch.Tensor:
    L = _lib.lib()
    O, I = w.shape
    src = w.float().contiguous().to(DEV)
    out = torch.zeros(O * I, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_repack_linear_weight(st(), vp(src), O, I, int(geglu), vp(out)))
    return out


def repack_bias(b: torch.Tensor, geglu=False) -> torch.Tensor:
    L = _lib.lib()
    src = b.float().contiguous().to(DEV)
    out = torch.zeros(b.numel(), dtype=torch.float32, device=DEV)
    _lib.check(L.gyre_op_repack_bias(st(), vp(src), b.numel(), int(geglu), vp(out)))
    return out
