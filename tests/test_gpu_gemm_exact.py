"""GEMM / implicit-GEMM convolution kernels (kernels_gemm.hip, kernels_gemm4s.hip, kernels_gemm_ar.hip, kernels_gemm_sm.hip,
kernels_conv_out.hip) on every tile config and dispatch branch, element-wise (-m gpu).

Walks tests/gemm_cases.py.  Lattice and wide-lattice rows: the output must EQUAL the exact value / its one RNE rounding bit for bit
(tests/gemm_ref.py explains why that holds for any tile, order, split factor, ring depth and weight layout); on a mismatch the test
prints how many elements differ, the first one, and the histogram of mismatches per 64-row x 64-column tile and per column - layout
mistakes show there.  Gaussian rows: gpu_util.check_bound with the derived constant (gemm_ref.gauss_k), printing the worst ratio and
a lower bound of the fp32 error before the store.  Rows a kernel refuses assert the error code.  Every output buffer carries sentinel
rows after M and sentinel columns between N and ldc: they must come back untouched.

Inputs no gyre_op_* entry can express (row bias, cropped upsample, circular padding, a second source, padded strides, an output off
its 16-byte alignment) go through gyre_op_gemm_test."""
import ctypes as C

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from gyre_amd import _lib
from gpu_util import DEV, HDT, check_bound, st, vp

pytestmark = pytest.mark.gpu
U = 2.0 ** -8 if HDT == torch.bfloat16 else 2.0 ** -11
NCHW_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def dev(t, dt=None):
    return None if t is None else t.to(dt or HDT).contiguous().to(DEV)


def canary_buffer(rows, ld, dt=None, off_bytes=0):
    """rows + CANARY_ROWS rows of ld elements holding the sentinel; the tensor returned for the kernel starts off_bytes in."""
    dt = dt or HDT
    esz = torch.empty(0, dtype=dt).element_size()
    flat = torch.full(((rows + R.CANARY_ROWS) * ld + 16,), R.CANARY, dtype=dt, device=DEV)
    assert off_bytes % esz == 0
    o = off_bytes // esz
    return flat, flat[o:o + (rows + R.CANARY_ROWS) * ld].view(rows + R.CANARY_ROWS, ld)


def assert_canaries(name, flat, view, rows, cols):
    v = view.float().cpu()
    assert bool((v[rows:] == R.CANARY).all()), f"{name}: rows after M were written"
    assert bool((v[:rows, cols:] == R.CANARY).all()), f"{name}: columns between N and the row stride were written"
    f = flat.float().cpu()
    n_view = view.numel()
    o = view.data_ptr() - flat.data_ptr()
    o //= flat.element_size()
    assert bool((f[:o] == R.CANARY).all()) and bool((f[o + n_view:] == R.CANARY).all()), f"{name}: bytes around the output were written"


def assert_exact(name, got, want):
    """torch.equal with a diagnosis: count, first mismatch, per-tile and per-column histogram."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    # (-0.0 == 0.0: an exact zero may carry either sign through bias / residual adds)
    bad = ~((got == want) | ((got == 0) & (want == 0)))
    n = int(bad.sum())
    print(f"[exact] {name}: {got.numel()} elements, {n} differ")
    if n:
        b2 = bad.reshape(-1, bad.shape[-1])
        idx = torch.nonzero(b2)[0].tolist()
        g2, w2 = got.reshape(b2.shape), want.reshape(b2.shape)
        print(f"   first at (row {idx[0]}, column {idx[1]}): got {float(g2[idx[0], idx[1]])} want {float(w2[idx[0], idx[1]])}")
        rows, cols = b2.shape
        tiles = {}
        for r_, c_ in torch.nonzero(b2).tolist():
            tiles[(r_ // 64, c_ // 64)] = tiles.get((r_ // 64, c_ // 64), 0) + 1
        print("   mismatches per 64 x 64 tile (tile row, tile column): count:", dict(sorted(tiles.items())[:32]))
        percol = b2.sum(0)
        print("   mismatches per column (first 48 non-zero):", [(int(c_), int(percol[c_])) for c_ in torch.nonzero(percol).flatten()[:48]])
        print("   mismatches per row (first 48 non-zero):", [(int(r_), int(b2[r_].sum())) for r_ in torch.nonzero(b2.sum(1)).flatten()[:48]])
    assert n == 0, f"{name}: {n} of {got.numel()} elements differ from the exact value"


def judge(name, c, got, value, bound=None, hdt=None, tiny=None):
    """got: the stored output in the layout of `value` (float64)."""
    hdt = hdt or HDT
    kind = c.row["kind"]
    if kind == "gauss":
        k = R.gauss_k(c.Ktot, hdt) if hdt != torch.float32 else c.Ktot * 2.0 ** -23 / 2.0 ** -24
        tiny = c.tiny if tiny is None else tiny
        worst = check_bound(name, got, value, bound, k=k, tiny=tiny, hdt=hdt)
        # what the 16-bit store alone explains is u |ref|: the rest is a lower bound of the fp32 error before the store
        u = 2.0 ** -24 if hdt == torch.float32 else 2.0 ** -8 if hdt == torch.bfloat16 else 2.0 ** -11
        low = ((got.double().cpu() - value).abs() - u * value.abs()).clamp_min(0)
        rel = float((low / bound.clamp_min(1e-300)).max())
        print(f"[bound] {name}: worst ratio {worst:.3g}; fp32 error before the store >= {rel:.3g} x bound "
              f"(allowed {c.Ktot * 2.0 ** -23:.3g} x bound)")
        return
    assert_exact(name, got.to(hdt), R.rne(value, hdt))


class Forced:
    """The thread's planner state for one row: forced config | splits, tuning bits, scratch buffers - restored on exit."""

    def __init__(self, r, c):
        self.r, self.c = r, c

    def __enter__(self):
        r, c, L = self.r, self.c, _lib.lib()
        self.L = L
        force = r["cfg"] | (r["splits"] << 8 if r["splits"] > 1 else 0)
        self.old_cfg = L.gyre_debug_force_gemm_cfg(force)
        self.old_abl = L.gyre_debug_gemm_ablation(r["abl"])
        if r["cfg"] == GC.AR:
            self.ar = torch.empty(c.Nw * c.K * 2 + 4096, dtype=torch.uint8, device=DEV)
            L.gyre_debug_set_ar_workspace(vp(self.ar), self.ar.numel())
        if r["feats"].get("wblk"):
            self.blk = torch.empty(c.Nw * c.Ktot * 2 + 4096, dtype=torch.uint8, device=DEV)
            L.gyre_debug_set_wblk_workspace(vp(self.blk), self.blk.numel())
        # split-K slabs: the forced factor's, or room for the planner's own factor on the small unforced rows
        slabs = r["splits"] if r["splits"] > 1 else (8 if c.M * c.Nw <= (1 << 20) and not r["cfg"] else 0)
        self.ws = torch.empty(slabs * c.M * c.Nw * 4 + 256, dtype=torch.uint8, device=DEV)
        if slabs:
            L.gyre_debug_set_splitk_workspace(vp(self.ws), self.ws.numel())
        return self

    def __exit__(self, *exc):
        L = self.L
        torch.cuda.synchronize()
        L.gyre_debug_force_gemm_cfg(self.old_cfg)
        L.gyre_debug_gemm_ablation(self.old_abl)
        L.gyre_debug_set_ar_workspace(None, 0)
        L.gyre_debug_set_wblk_workspace(None, 0)
        L.gyre_debug_set_splitk_workspace(None, 0)
        return False


def expect_rc(r, rc):
    if r["rc"]:
        assert rc == r["rc"], f"{r['id']}: status {rc}, expected {r['rc']} ({r['why']}): {_lib.lib().gyre_last_error().decode()}"
        return True
    _lib.check(rc)
    return False


def run_gemm_test(r, c):
    L = _lib.lib()
    f = r["feats"]
    ptr = dict(a1=dev(c.a1), a2=dev(c.a2), w=dev(c.w), bias=dev(c.bias, torch.float32), rowbias=dev(c.rowbias, torch.float32),
               residual=dev(c.residual))
    addr = {k: (vp(v).value if v is not None else 0) for k, v in ptr.items()}
    if r["op"] == "linear_t":
        B = c.M // f["tokens"]
        flat, out = canary_buffer(B * c.N, f["ldt"])
        rows, cols = B * c.N, f["tokens"]
    else:
        flat, out = canary_buffer(c.M, c.ldc, off_bytes=f.get("out_off", 0))
        rows, cols = c.M, c.N
    vp(flat)
    with Forced(r, c) as fz:
        a = R.gemm_test_args(c, addr, out.data_ptr(), (vp(fz.ws).value, fz.ws.numel()))
        prc, plan = R.plan_query(L, a)
        if prc == 0:
            # the plan that is reported is the plan that runs: its slab space is there (too little is an error of the entry point)
            assert fz.ws.numel() >= plan["ws_lo"] + (plan["ws_hi"] << 32) and (r["splits"] <= 1 or plan["splits"] == r["splits"]), plan
        rc = L.gyre_op_gemm_test(st(), C.byref(a))
        if expect_rc(r, rc):
            torch.cuda.synchronize()
            assert bool((flat.float().cpu() == R.CANARY).all()), f"{r['id']}: a refused launch wrote to the output"
            return
    assert_canaries(r["id"], flat, out, rows, cols)
    got = out[:rows, :cols].float().cpu()
    if r["op"] == "linear_t":
        want = R.transposed(c.value, f["tokens"], f["tokens"], 0.0).reshape(rows, cols)
        bound = R.transposed(c.bound, f["tokens"], f["tokens"], 0.0).reshape(rows, cols) if c.bound is not None else None
        judge(r["id"], c, got, want, bound)
    else:
        judge(r["id"], c, got, c.value, c.bound)


def run_qkv(r, c):
    L = _lib.lib()
    f = r["feats"]
    Cc, tok, ldt = c.K, f["tokens"], f["ldt"]
    B = c.M // tok
    fq, qk = canary_buffer(c.M, 2 * Cc)
    fv, vt = canary_buffer(B * Cc, ldt)
    vp(fq), vp(fv)
    with Forced(r, c):
        rc = L.gyre_op_qkv(st(), vp(dev(c.a1)), c.M, Cc, vp(dev(c.w)), tok, C.c_void_p(qk.data_ptr()), C.c_void_p(vt.data_ptr()), ldt)
        if expect_rc(r, rc):
            return
    assert_canaries(r["id"] + " Q|K", fq, qk, c.M, 2 * Cc)
    assert_canaries(r["id"] + " V^T", fv, vt, B * Cc, tok)
    judge(r["id"] + " Q|K", c, qk[:c.M].float().cpu(), c.value[:, :2 * Cc])
    want_vt = R.transposed(c.value[:, 2 * Cc:], tok, tok, 0.0).reshape(B * Cc, tok)
    judge(r["id"] + " V^T", c, vt[:B * Cc, :tok].float().cpu(), want_vt)


def run_conv_nchw(r, c):
    L = _lib.lib()
    s, f = r["shape"], r["feats"]
    odt = NCHW_DT[f["dtype"]]
    B, H, W = s["B"], s["H"], s["W"]
    flat, out = canary_buffer(B * c.N, H * W, dt=odt)
    vp(flat)
    with Forced(r, c):
        rc = L.gyre_op_conv3x3_nchw(st(), vp(dev(c.a1)), B, H, W, s["Cin"], vp(dev(c.w)), c.N, vp(dev(c.bias, torch.float32)),
                                    C.c_void_p(out.data_ptr()), f["dtype"], f["force_tiles"])
        if expect_rc(r, rc):
            return
    assert_canaries(r["id"], flat, out, B * c.N, H * W)
    got = out[:B * c.N].reshape(B, c.N, H, W).float().cpu()
    want = R.nchw(c.value, B, H, W)
    judge(r["id"], c, got, want, R.nchw(c.bound, B, H, W) if c.bound is not None else None, hdt=odt)


def run_colstats(r, c):
    L = _lib.lib()
    s, f = r["shape"], r["feats"]
    unit = f["unit"]
    flat, y = canary_buffer(c.M, c.N)
    stats = torch.full((c.M // 16 * (c.N // unit) * 2 + 64,), R.CANARY, dtype=torch.float32, device=DEV)
    rows = C.c_int(0)
    vp(flat)
    with Forced(r, c) as fz:
        if r["op"] == "colstats_conv":
            rc = L.gyre_op_conv3x3_colstats(st(), vp(dev(c.a1)), s["B"], s["H"], s["W"], s["Cin"], vp(dev(c.w)), c.N, vp(dev(c.bias, torch.float32)),
                                            vp(dev(c.residual)), 1, 0, unit, C.c_void_p(y.data_ptr()), vp(stats), stats.numel() * 4 - 256,
                                            vp(fz.ws), fz.ws.numel(), C.byref(rows))
        else:
            rc = L.gyre_op_linear_colstats(st(), vp(dev(c.a1)), c.M, c.K, vp(dev(c.w)), c.N, vp(dev(c.bias, torch.float32)), vp(dev(c.residual)),
                                           f["rps"], unit, C.c_void_p(y.data_ptr()), vp(stats), stats.numel() * 4 - 256, vp(fz.ws), fz.ws.numel(),
                                           C.byref(rows))
        _lib.check(rc)
    assert rows.value == r["plan"]["colstat_rows"], (rows.value, r["plan"])
    assert_canaries(r["id"], flat, y, c.M, c.N)
    judge(r["id"], c, y[:c.M].float().cpu(), c.value)
    want = R.colstats(c.value, rows.value, unit)
    assert float(want[..., 1].max()) < 2.0 ** 24                  # every sum of squares the kernel forms is an exact fp32 integer
    n = want.numel()
    got = stats[:n].double().cpu().reshape(want.shape)
    assert_exact(r["id"] + " statistics", got, want)
    assert bool((stats[n:].cpu() == R.CANARY).all()), "statistics written past their block"


def run_rowstats(r, c):
    L = _lib.lib()
    parts = L.gyre_op_linear_rowstats_parts(c.M, c.K, c.N, 1 if c.residual is not None else 0)
    assert parts == r["plan"]["rowstat_parts"]
    flat, y = canary_buffer(c.M, c.N)
    stats = torch.full((parts * c.M * 2 + 64,), R.CANARY, dtype=torch.float32, device=DEV)
    vp(flat)
    with Forced(r, c):
        _lib.check(L.gyre_op_linear_rowstats(st(), vp(dev(c.a1)), c.M, c.K, vp(dev(c.w)), c.N, vp(dev(c.bias, torch.float32)), vp(dev(c.residual)),
                                             C.c_void_p(y.data_ptr()), vp(stats)))
    assert_canaries(r["id"], flat, y, c.M, c.N)
    judge(r["id"], c, y[:c.M].float().cpu(), c.value)
    bn = {t[0]: t[2] for t in tiles()}[r["plan"]["cfg"]]
    want = R.rowstats(c.value, bn)
    assert want.shape[0] == parts and float(want[..., 1].max()) < 2.0 ** 24
    assert_exact(r["id"] + " statistics", stats[:want.numel()].double().cpu().reshape(want.shape), want)
    assert bool((stats[want.numel():].cpu() == R.CANARY).all())


def run_shortcut(r, c):
    L = _lib.lib()
    s, f = r["shape"], r["feats"]
    C1, C2 = f["C1s"], f["C2s"]
    flat, y = canary_buffer(c.M, c.N)
    ws = torch.empty(c.N * c.Ktot * 2 + c.N * 4 + 1024, dtype=torch.uint8, device=DEV)
    vp(flat)
    with Forced(r, c):
        rc = L.gyre_op_conv3x3_shortcut(st(), vp(dev(c.a1)), s["B"], s["H"], s["W"], s["Cin"], vp(dev(c.w)), c.N, vp(dev(c.bias, torch.float32)),
                                        vp(dev(c.sc[:, :C1])), C1, vp(dev(c.sc[:, C1:])) if C2 else None, C2, vp(dev(c.w_sc)),
                                        vp(dev(c.bias_sc, torch.float32)), vp(ws), ws.numel(), C.c_void_p(y.data_ptr()))
        _lib.check(rc)                           # (-6 would mean the planner no longer folds this shape: the row must move)
    assert_canaries(r["id"], flat, y, c.M, c.N)
    judge(r["id"], c, y[:c.M].float().cpu(), c.value)


_TILES = []


def tiles():
    if not _TILES:
        buf = (C.c_int32 * 256)()
        n = _lib.lib().gyre_debug_gemm_tiles(buf, 256)
        _TILES.extend(tuple(buf[4 * i:4 * i + 4]) for i in range(n))
    return _TILES


RUN = {"linear": run_gemm_test, "linear_t": run_gemm_test, "conv": run_gemm_test, "qkv": run_qkv, "conv_nchw": run_conv_nchw,
       "colstats_conv": run_colstats, "colstats_linear": run_colstats, "rowstats": run_rowstats, "shortcut": run_shortcut}


@pytest.mark.parametrize("rid", [r["id"] for r in GC.ROWS])
def test_gemm_row(rid):
    r = GC.BY_ID[rid]
    c = R.build_case(r, HDT)
    RUN[r["op"]](r, c)


def test_gemm_test_entry_rejects_bad_arguments():
    """gyre_op_gemm_test validates its integers and pointers before anything is derived from them: error codes, never a launch."""
    L = _lib.lib()
    x = torch.zeros(64 * 64, dtype=HDT, device=DEV)
    flat, out = canary_buffer(64, 64)
    vp(x), vp(flat)

    def args(**kw):
        a = _lib.GemmTestArgs()
        a.M, a.K, a.N = 64, 64, 64
        a.A = a.W = x.data_ptr()
        a.out = out.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _lib.check(L.gyre_op_gemm_test(st(), C.byref(args())))
    for kw in (dict(M=0), dict(K=-8), dict(K=12), dict(N=0), dict(conv=2), dict(geglu=2), dict(lda=56), dict(ldc=60), dict(lda=-1),
               dict(out_mode=3), dict(out_mode=1), dict(out_dtype=3), dict(A=0), dict(W=0), dict(out=0), dict(rows_per_sample=5),
               dict(samples=5), dict(A2=x.data_ptr(), C1=0), dict(A2=x.data_ptr(), C1=60), dict(A2=x.data_ptr(), C1=64),
               dict(out_mode=2, tokens=0), dict(out_mode=2, tokens=24, ldt=24), dict(out=out.data_ptr() + 2), dict(bias=x.data_ptr() + 4),
               dict(conv=1, B=1, Hi=4, Wi=4, Cin=12), dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=3), dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=2),
               dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=1, wrap=4), dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=0, wrap=1),
               dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=1, Hup=7), dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=1, ups=1, Hup=6),
               dict(conv=1, B=0, Hi=4, Wi=4, Cin=8, stride=1, pad=1), dict(conv=1, B=1, Hi=4, Wi=4, Cin=8, stride=1, pad=1, geglu=1)):
        rc = L.gyre_op_gemm_test(st(), C.byref(args(**kw)))
        assert rc == -1, (kw, rc)
    assert L.gyre_op_gemm_test(st(), None) == -1
    for kw in (dict(sc_K=64, sc_A=x.data_ptr()), dict(conv=1, B=1, Hi=4, Wi=4, Cin=64, stride=1, pad=1, sc_K=12, sc_A=x.data_ptr()),
               dict(conv=1, B=1, Hi=4, Wi=4, Cin=64, stride=1, pad=1, sc_K=64), dict(conv=1, B=1, Hi=4, Wi=4, Cin=64, stride=2, pad=1, sc_K=64, sc_A=x.data_ptr()),
               dict(conv=1, B=1, Hi=4, Wi=4, Cin=64, stride=1, pad=1, sc_K=64, sc_A=x.data_ptr(), sc_A2=x.data_ptr(), sc_C1=64)):
        assert L.gyre_op_gemm_test(st(), C.byref(args(**kw))) == -1, kw
    # a plan in K slices without its slab space is an error, not a silent run of another configuration
    old = L.gyre_debug_force_gemm_cfg(8 | (2 << 8))
    try:
        big = torch.zeros(64 * 256, dtype=HDT, device=DEV)
        vp(big)
        assert L.gyre_op_gemm_test(st(), C.byref(args(K=256, A=big.data_ptr(), W=big.data_ptr()))) == -4
        ws = torch.empty(2 * 64 * 64 * 4, dtype=torch.uint8, device=DEV)
        vp(ws)
        assert L.gyre_op_gemm_test(st(), C.byref(args(K=256, A=big.data_ptr(), W=big.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel() - 4))) == -4
        _lib.check(L.gyre_op_gemm_test(st(), C.byref(args(K=256, A=big.data_ptr(), W=big.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel()))))
    finally:
        L.gyre_debug_force_gemm_cfg(old)
    torch.cuda.synchronize()
    assert_canaries("bad arguments", flat, out, 64, 64)
