"""Token merging (csrc/kernels_tome.hip) judged exactly: on lattice keys (tests/tome_exact_ref.py) the selection - order, node_idx,
dstlist - must equal the float64 reference index for index, ties included; the merge and its adjoint are judged element by element
against float64 within  u |ref| + (cnt + 2) 2^-24 mean|x|  and  u |ref| + 2 2^-24 |dy|  (derivation in that module), copied rows bit
for bit.  Cases are data in tests/tome_cases.py; tests/test_tome_ref_host.py proves on the host that the lattice is exact and tied,
that the tolerance is achievable and that seeded mistakes are caught."""
import pytest
import torch

import tome_exact_ref as X
from gyre_amd import _lib
from gpu_util import DEV, HDT, st, vp
from tome_cases import ADJOINT, GAUSS, LATTICE, MERGE_REFUSALS

pytestmark = pytest.mark.gpu
U = 2.0 ** -8 if HDT == torch.bfloat16 else 2.0 ** -11
SENTINEL = 777.0


def _id(c):
    return "x".join(str(int(v)) for v in c)


_KEYS = {}


def _lattice(case):
    if case not in _KEYS:
        B, N, C, r, star = case
        _KEYS[case] = X.lattice_keys(B, N, C, seed=1000 + N, star=star, r=r)
    return _KEYS[case]


def _gauss(B, N, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, C, generator=g).to(HDT).float(), torch.randn(B, N, C, generator=g).to(HDT).float()


def _gapped(x, ld, off):
    """x [B, N, C] as rows of a NaN-filled [B, N, ld] device buffer at column offset off; returns (buffer, view at the offset)."""
    B, N, C = x.shape
    buf = torch.full((B, N, ld), float("nan"), dtype=HDT, device=DEV)
    buf[:, :, off:off + C] = x.to(HDT).to(DEV)
    return buf, buf.view(-1)[off:]


def _merge(k, v, r, gaps=True, ldvt_extra=16, with_vrows=True):
    """gyre_op_tome_merge_ex on k, v [B, N, C] (CPU, storage-exact values).  gaps: ldk = 2C, ldv = 3C (v at column offset C) with NaN
    between the rows.  Every output buffer is pre-filled with NaN (indices with -1)."""
    L = _lib.lib()
    B, N, C = k.shape
    half, reff = N // 2, max(0, min(r, N // 2))
    nout = N - reff
    ldk, ldv, voff = (2 * C, 3 * C, C) if gaps else (C, C, 0)
    kb, kp = _gapped(k, ldk, 0)
    vb, vptr = _gapped(v, ldv, voff)
    ldvt = (nout + 7) // 8 * 8 + ldvt_extra
    nan = float("nan")
    k_out = torch.full((B, nout, C), nan, dtype=HDT, device=DEV)
    vt_out = torch.full((B, C, ldvt), nan, dtype=HDT, device=DEV)
    vrows = torch.full((B, nout, C), nan, dtype=HDT, device=DEV) if with_vrows else None
    order, nidx, dl = (torch.full((B, half), -1, dtype=torch.int32, device=DEV) for _ in range(3))
    wsb = L.gyre_op_tome_workspace(B, N, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.check(L.gyre_op_tome_merge_ex(st(), vp(kp), ldk, vp(vptr), ldv, B, N, C, r, vp(ws), wsb, vp(k_out), vp(vt_out), ldvt,
                                       vp(order), vp(nidx), vp(dl), vp(vrows)))
    torch.cuda.synchronize()
    return dict(k_out=k_out.cpu(), vt_out=vt_out.cpu(), vrows=None if vrows is None else vrows.cpu(), order=order.cpu().long(),
                node_idx=nidx.cpu().long(), dstlist=dl.cpu().long(), reff=reff, nout=nout, dev=dict(order=order, dstlist=dl))


def _judge(name, got, x, order, node_idx, reff):
    """Element-wise judgement of merged rows got [B, N - r, C] (storage dtype) against float64; copies bit for bit."""
    ref, cnt, absmean = X.merge_wavg64(x, order, node_idx, reff)
    tol = X.merge_tolerance(ref, cnt, absmean, U)
    g = got.double()
    ratio = ((g - ref).abs() / tol).nan_to_num(nan=float("inf"))
    flat = int(ratio.argmax())
    print(f"[bound] {name}: worst ratio {float(ratio.max()):.3g} at flat index {flat} (row count {int(cnt.flatten()[flat // ref.shape[2]])}, "
          f"max count {int(cnt.max())})")
    assert float(ratio.max()) <= 1.0, name
    copies = cnt == 1
    assert torch.equal(got[copies], ref.to(HDT)[copies]), f"{name}: copied rows must be bit-equal"
    return float(ratio.max())


def _judge_outputs(name, out, k, v):
    o, n, reff, nout = out["order"], out["node_idx"], out["reff"], out["nout"]
    _judge(f"tome k_out {name}", out["k_out"], k, o, n, reff)
    _judge(f"tome vrows_out {name}", out["vrows"], v, o, n, reff)
    _judge(f"tome vt_out {name}", out["vt_out"][:, :, :nout].transpose(1, 2), v, o, n, reff)
    pad = out["vt_out"][:, :, nout:]
    assert pad.shape[2] >= 16 and bool((pad == 0).all()), "pad columns of vt_out must be exactly zero"


@pytest.mark.parametrize("case", LATTICE, ids=_id)
def test_selection_is_exact_on_lattice_keys(case):
    B, N, C, r, star = case
    k = _lattice(case)
    v = _gauss(B, N, C, N)[1]
    out = _merge(k, v, r)
    order, node_idx, _, reff = X.select64(k, r)
    dl = X.dstlist_of(order, node_idx, reff)
    for name, got, ref in (("node_idx", out["node_idx"], node_idx), ("order", out["order"], order), ("dstlist", out["dstlist"][:, :reff], dl)):
        agree = float((got == ref).double().mean())
        print(f"[exact] tome {name} {_id(case)}: agreement {agree:.6f}")
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.numel()} indices differ from the float64 selection"
    _judge_outputs(_id(case), out, k, v)


def test_r_above_half_clamps():
    B, N, C, r, star = LATTICE[1]
    k, v = _lattice(LATTICE[1]), _gauss(B, N, C, 5)[1]
    out = _merge(k, v, 10 ** 6)
    order, node_idx, _, reff = X.select64(k, 10 ** 6)
    assert reff == N // 2 == out["reff"] and torch.equal(out["order"], order) and torch.equal(out["node_idx"], node_idx)
    assert torch.equal(out["dstlist"], X.dstlist_of(order, node_idx, reff))
    _judge_outputs("r clamped", out, k, v)


@pytest.mark.parametrize("case", GAUSS, ids=_id)
def test_merge_arithmetic_element_wise(case):
    """Gaussian keys and values merged with the kernel's OWN selection (Gaussian scores are not exact, the selection is judged on
    the lattice); every layout of the launcher gives the same bits."""
    B, N, C, r = case
    k, v = _gauss(B, N, C, 300 + N)
    out = _merge(k, v, r)
    half = N // 2
    for b in range(B):
        assert sorted(out["order"][b].tolist()) == list(range(half)) and 0 <= int(out["node_idx"][b].min()) and int(out["node_idx"][b].max()) < half
    assert torch.equal(out["dstlist"][:, :out["reff"]], X.dstlist_of(out["order"], out["node_idx"], out["reff"]))
    _judge_outputs(_id(case), out, k, v)
    plain = _merge(k, v, r, gaps=False, ldvt_extra=0, with_vrows=False)          # dense rows, minimal ldvt, vrows_out NULL
    assert torch.equal(plain["order"], out["order"]) and torch.equal(plain["node_idx"], out["node_idx"])
    assert torch.equal(plain["k_out"], out["k_out"])
    assert torch.equal(plain["vt_out"][:, :, :out["nout"]], out["vt_out"][:, :, :out["nout"]])
    assert bool((plain["vt_out"][:, :, out["nout"]:] == 0).all())


@pytest.mark.parametrize("case", ADJOINT, ids=_id)
def test_unmerge_against_the_float64_transpose(case):
    L = _lib.lib()
    B, N, C, r, star = case
    k = _lattice(case)
    out = _merge(k, k, r)
    order, node_idx, _, reff = X.select64(k, r)
    dl = X.dstlist_of(order, node_idx, reff)
    assert torch.equal(out["order"], order) and torch.equal(out["dstlist"][:, :reff], dl)
    nout, half = N - reff, N // 2
    dy = torch.randn(B, nout, C, generator=torch.Generator().manual_seed(N + 1)).to(HDT)
    ldx = 3 * C
    dxb = torch.full((B, N, ldx), SENTINEL, dtype=HDT, device=DEV)
    inv = torch.full((B, half), -1, dtype=torch.int32, device=DEV)
    _lib.check(L.gyre_op_tome_unmerge(st(), vp(dy.to(DEV)), B, N, C, reff, vp(out["dev"]["order"]), vp(out["dev"]["dstlist"]), vp(inv),
                                      vp(dxb.view(-1)[C:]), ldx))
    torch.cuda.synchronize()
    dxb = dxb.cpu()
    got = dxb[:, :, C:2 * C]
    assert bool((dxb[:, :, :C] == SENTINEL).all()) and bool((dxb[:, :, 2 * C:] == SENTINEL).all()), "the gaps of dx must stay untouched"
    ref, w, src = X.unmerge64(dy.float(), order, dl, reff, N)
    ratio = ((got.double() - ref).abs() / X.unmerge_tolerance(ref, src, U)).nan_to_num(nan=float("inf"))
    print(f"[bound] tome unmerge {_id(case)}: worst ratio {float(ratio.max()):.3g}, smallest weight 1/{int(round(1 / float(w.min())))}")
    assert float(ratio.max()) <= 1.0
    pow2 = torch.log2(w) == torch.log2(w).round()
    assert int(pow2.sum()) > 0 and torch.equal(got[pow2], ref.to(HDT)[pow2]), "weight 1 or a power of two: bit-equal"
    if star:
        assert int(round(1 / float(w.min()))) == half + 1


def test_refusals_are_error_codes_and_launch_nothing():
    L = _lib.lib()
    base = dict(B=1, N=64, C=64, r=8, ldvt=64)
    x = torch.zeros(1, 64, 1544, dtype=HDT, device=DEV)
    out = torch.zeros(1, 64, 1544, dtype=HDT, device=DEV)
    idx = torch.zeros(64, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.gyre_op_tome_workspace(1, 64, 1544), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    for what, over, code in MERGE_REFUSALS:
        a = {**base, "ws_bytes": ws.numel(), **over}
        before = L.gyre_last_launch_count()
        rc = L.gyre_op_tome_merge_ex(st(), vp(x), a["C"], vp(x), a["C"], a["B"], a["N"], a["C"], a["r"], vp(ws), a["ws_bytes"], vp(out), vp(out),
                                     a["ldvt"], None, None, None, None)
        assert rc == code, f"{what}: status {rc}, expected {code}"
        assert L.gyre_last_launch_count() == before, f"{what}: refused after a launch"
    before = L.gyre_last_launch_count()
    assert L.gyre_op_tome_unmerge(st(), vp(x), 1, 64, 64, 33, vp(idx), vp(idx), vp(idx), vp(out), 64) == -1             # r > N / 2
    assert L.gyre_op_tome_unmerge(st(), vp(x), 1, 64, 64, 8, vp(idx), vp(idx), vp(idx), vp(out), 68) == -1              # ldx % 8
    assert L.gyre_op_tome_unmerge(st(), vp(x), 1, 64, 64, 8, None, vp(idx), vp(idx), vp(out), 64) == -1                 # null argument
    assert L.gyre_op_tome_merge_ex(st(), None, 64, vp(x), 64, 1, 64, 64, 8, vp(ws), ws.numel(), vp(out), vp(out), 64, None, None, None, None) == -1
    assert L.gyre_last_launch_count() == before
