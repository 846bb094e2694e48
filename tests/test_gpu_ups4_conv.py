"""The four-parity form of an upsampler convolution on the pipelined 256x320 tile (k_gemm4s U4, kernels_gemm4s.hip) through the
operator entry gyre_op_upsample_conv_test, with tuning bit 30 (config 24 whatever the tile count) on the smallest shapes at which each
part can still go wrong (-m gpu; the f16 flavour re-runs the file with GYRE_STORAGE=f16).

  exact lattice   x integers in [-2, 2], w integers in [-4, 4], integer bias: every composed weight (|.| <= 16) and every fp32 partial
                  sum (<= 4 * 320 * 2 * 16 < 2^24) is exact, so the stored output must equal the library's own NINE-TAP launch of the
                  same problem bit for bit, and one RNE rounding of the float64 value.  Pins tap grouping, borders, the row map, the
                  parity -> weight-row mapping and the slab order behind the untouched reduction kernel.
  random data     element-wise |got - ref| <= comp + K 2^-23 bound + u |ref| against the float64 nine-tap value of the stored operands:
                  comp = sum |x| * (half a storage ulp of each composed weight), the one new rounding; K 2^-23 bound = the fp32
                  accumulation term of the GEMM tests (gemm_ref.gauss_k, K = 4 Cin products); u |ref| = the output's rounding.
  statistics      the partials, indexed (sample, parity, local tile), against the float64 sums of the stored output; a GroupNorm fed
                  with them against the same GroupNorm running its own statistics pass.
"""
import ctypes as C
import math

import pytest
import torch

import gemm_ref as R
import ups4_ref as U4
from gyre_amd import _lib
from gpu_util import DEV, HDT, check_bound, st, vp

pytestmark = pytest.mark.gpu
F64 = torch.float64
UPS4_ALL = 1 << 30
MANT = 7 if HDT == torch.bfloat16 else 10          # stored significand bits
CANARY = -3.0

# (B, Hi, Wi, Cin, N, splits, colstat unit)
CASES = {
    "ragged-tile-per-parity": (2, 8, 8, 64, 40, 1, 0),        # Mp = 128 < 256: one ragged tile per parity spanning both samples, partial N tile
    "two-chunks-two-n-tiles": (1, 16, 16, 128, 328, 1, 8),    # Mp = 256 exactly, chunk-outer / tap-inner over 2 chunks, 8 live columns in N tile 2
    "non-square-ragged-last": (3, 16, 8, 64, 64, 1, 0),       # Mp = 384: a full and a half tile per parity
    "two-k-slices": (2, 8, 8, 320, 64, 2, 0),                 # slabs in output-row order, k_splitk_reduce behind
    "four-k-slices": (2, 8, 8, 320, 64, 4, 0),
}


def operands(case, kind, seed=0):
    B, Hi, Wi, Cin, N = case[:5]
    g = torch.Generator().manual_seed(seed)
    if kind == "lattice":
        x = torch.randint(-2, 3, (B, Hi, Wi, Cin), generator=g).to(F64)
        w = torch.randint(-4, 5, (N, 3, 3, Cin), generator=g).to(F64)
        bias = torch.randint(-8, 9, (N,), generator=g).to(F64)
    else:
        x = torch.randn(B, Hi, Wi, Cin, generator=g).to(HDT).to(F64)
        w = (torch.randn(N, 3, 3, Cin, generator=g) / math.sqrt(9 * Cin)).to(HDT).to(F64)
        bias = torch.randn(N, generator=g).float().to(F64)
    return x, w, bias


_REF = {}


def nine_tap_ref(name, kind, seed=0):
    """(x, w, bias, value, abs-form bound) of a case, float64, computed once per (case, kind, seed)."""
    key = (name, kind, seed)
    if key not in _REF:
        x, w, bias = operands(CASES[name], kind, seed)
        A = R.conv_gather(x, ups=1)
        M, _, Cc = A.shape
        v, b = R.reference(A.reshape(M, 9 * Cc), w.reshape(w.shape[0], 9 * Cc), bias=bias)
        _REF[key] = (x, w, bias, v, b)
    return _REF[key]


class Bit30:
    def __enter__(self):
        self.L = _lib.lib()
        self.old = self.L.gyre_debug_gemm_ablation(UPS4_ALL)
        return self.L

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.L.gyre_debug_gemm_ablation(self.old)
        return False


def run_ups4(L, case, x, w, bias, scratch=None, want_stats=False):
    """-> (out [M][N] storage on the device, canaried; partials or None; rows)."""
    B, Hi, Wi, Cin, N, splits, unit = case
    M = B * 4 * Hi * Wi
    out = torch.full((M + 4, N), CANARY, dtype=HDT, device=DEV)
    xd, wd, bd = x.to(HDT).to(DEV), w.to(HDT).to(DEV), bias.float().to(DEV)
    scratch = torch.empty(16 * N * Cin + 64, dtype=HDT, device=DEV) if scratch is None else scratch
    ws = torch.empty(max(splits, 1) * M * N + 64, dtype=torch.float32, device=DEV)
    a = _lib.UpsampleConvTestArgs()
    a.B, a.Hi, a.Wi, a.Cin, a.N, a.splits = B, Hi, Wi, Cin, N, splits
    a.x, a.w, a.bias, a.out = vp(xd).value, vp(wd).value, vp(bd).value, vp(out).value
    a.scratch, a.scratch_bytes = vp(scratch).value, 16 * N * Cin * scratch.element_size()
    a.ws, a.ws_bytes = vp(ws).value, ws.numel() * 4
    stats, rows = None, 0
    if want_stats:
        q = (C.c_int32 * 4)()
        _lib.check(L.gyre_debug_ups4_plan(B, Hi, Wi, Cin, N, 0, 0, 0, unit, q))
        assert tuple(q)[:3] == (1, 24, 1) and q[3] == 256, tuple(q)
        rows = q[3]
        stats = torch.full((M // rows, N // unit, 2), float("nan"), dtype=torch.float32, device=DEV)
        a.colstat_unit, a.colstat_out = unit, vp(stats).value
    _lib.check(L.gyre_op_upsample_conv_test(st(), C.byref(a)))
    torch.cuda.synchronize()
    assert bool((out[M:].float() == CANARY).all()), "rows after M were written"
    return out[:M], stats, rows


def run_nine_tap(L, case, x, w, bias):
    """The library's own nine-tap launch of the same problem (gyre_op_gemm_test, the planner's config, ablation bits as they are)."""
    B, Hi, Wi, Cin, N = case[:5]
    M = B * 4 * Hi * Wi
    out = torch.full((M, N), CANARY, dtype=HDT, device=DEV)
    xd, wd, bd = x.to(HDT).to(DEV), w.to(HDT).to(DEV), bias.float().to(DEV)
    ws = torch.empty(16 * M * N + 64, dtype=torch.float32, device=DEV)
    a = _lib.GemmTestArgs()
    a.conv, a.N, a.B, a.Hi, a.Wi, a.Cin, a.stride, a.pad, a.ups = 1, N, B, Hi, Wi, Cin, 1, 1, 1
    a.A, a.W, a.bias, a.out = vp(xd).value, vp(wd).value, vp(bd).value, vp(out).value
    a.ws, a.ws_bytes = vp(ws).value, ws.numel() * 4
    _lib.check(L.gyre_op_gemm_test(st(), C.byref(a)))
    torch.cuda.synchronize()
    return out


def describe_mismatch(name, got, want, case):
    B, Hi, Wi = case[:3]
    bad = ~((got == want) | ((got == 0) & (want == 0)))
    n = int(bad.sum())
    print(f"[exact] {name}: {got.numel()} elements, {n} differ")
    if n:
        rows = torch.nonzero(bad.any(1)).flatten()
        r0 = int(rows[0])
        nn, rem = divmod(r0, 4 * Hi * Wi)
        Y, X = divmod(rem, 2 * Wi)
        c0 = int(torch.nonzero(bad[r0]).flatten()[0])
        print(f"   first at row {r0} (sample {nn}, Y {Y}, X {X}, parity {2 * (Y & 1) + (X & 1)}), column {c0}: got {float(got[r0, c0])} "
              f"want {float(want[r0, c0])}; {len(rows)} rows affected")
        par = [(int(r) % (4 * Hi * Wi)) for r in rows]
        hist = {}
        for r in par:
            Y, X = divmod(r, 2 * Wi)
            hist[2 * (Y & 1) + (X & 1)] = hist.get(2 * (Y & 1) + (X & 1), 0) + 1
        print("   affected rows per parity:", hist, " columns (first 32):", torch.nonzero(bad.any(0)).flatten()[:32].tolist())
    return n


@pytest.mark.parametrize("name", list(CASES))
def test_exact_lattice_equals_the_nine_tap_launch(name):
    case = CASES[name]
    x, w, bias, value, _ = nine_tap_ref(name, "lattice")
    with Bit30() as L:
        got, _, _ = run_ups4(L, case, x, w, bias)
        nine = run_nine_tap(L, case, x, w, bias)
    got, nine = got.float().cpu(), nine.float().cpu()
    assert float(value.abs().max()) < 2.0 ** 24
    n1 = describe_mismatch(name + " vs nine-tap launch", got, nine, case)
    n2 = describe_mismatch(name + " vs RNE(float64)", got, R.rne(value, HDT).float(), case)
    assert n1 == 0 and n2 == 0


def half_ulp(wc):
    """Half a storage ulp of every (exact) composed weight: the most its one rounding can move it."""
    e = torch.floor(torch.log2(wc.abs().clamp_min(2.0 ** -120)))
    return torch.where(wc == 0, torch.zeros_like(wc), torch.exp2(e - MANT - 1))


@pytest.mark.parametrize("name", list(CASES))
def test_random_data_within_the_derived_bound(name):
    case = CASES[name]
    Cin = case[3]
    x, w, bias, value, bound = nine_tap_ref(name, "gauss")
    with Bit30() as L:
        got, _, _ = run_ups4(L, case, x, w, bias)
    comp = U4.forward(x, half_ulp(U4.compose(w)), absolute=True)
    worst = check_bound(name, got.float().cpu(), value, bound, k=R.gauss_k(4 * Cin, HDT), tiny=comp)
    # how much of the allowance the composition term is, and the error in units of the output's own rounding
    u = 2.0 ** -(MANT + 1)
    print(f"[ups4] {name}: worst ratio {worst:.3g}; composition term / output rounding (median) = "
          f"{float((comp / (u * value.abs()).clamp_min(1e-30)).median()):.3g}; rel-L2 vs float64 = "
          f"{float((got.double().cpu() - value).norm() / value.norm()):.3e}")


def test_column_statistics_feed_the_groupnorm():
    name = "two-chunks-two-n-tiles"
    case = CASES[name]
    B, Hi, Wi, Cin, N, _, unit = case
    x, w, bias, value, bound = nine_tap_ref(name, "gauss")
    with Bit30() as L:
        out, stats, rows = run_ups4(L, case, x, w, bias, want_stats=True)
    y = out.double().cpu()
    stats = stats.double().cpu()
    assert not bool(torch.isnan(stats).any()), "a statistics block was not written"
    # block (sample, parity, local tile): the 256 source pixels lt * 256 .. of that sample and parity, scattered to their output rows
    tps = Hi * Wi // rows
    want = torch.zeros_like(stats)
    mags = torch.zeros_like(stats)
    for n in range(B):
        for par in range(4):
            orow = U4.out_rows(1, Hi, Wi, par >> 1, par & 1) + n * 4 * Hi * Wi
            for lt in range(tps):
                blk = y[orow[lt * rows:(lt + 1) * rows]].reshape(rows, N // unit, unit)
                i = n * 4 * tps + par * tps + lt
                want[i, :, 0], want[i, :, 1] = blk.sum(dim=(0, 2)), (blk * blk).sum(dim=(0, 2))
                mags[i, :, 0], mags[i, :, 1] = blk.abs().sum(dim=(0, 2)), (blk * blk).sum(dim=(0, 2))
    # fp32 sums of rows * unit = 2048 values in a fixed tree-like order: 2048 2^-24 of the sum of magnitudes covers any order
    tol = rows * unit * 2.0 ** -24 * mags + 1e-30
    ratio = float(((stats - want).abs() / tol).max())
    print(f"[ups4 colstats] per-block partials: worst |diff| / (n 2^-24 sum|.|) = {ratio:.3g}")
    assert ratio <= 1.0
    # summed per sample they are the sample's statistics, as the consumer adds them
    per_sample = stats.reshape(B, 4 * tps, N // unit, 2).sum(1)
    full = R.colstats(y, 4 * Hi * Wi, unit)
    assert float(((per_sample - full).abs() / (4 * Hi * Wi * unit * 2.0 ** -24 * mags.reshape(B, 4 * tps, N // unit, 2).sum(1) + 1e-30)).max()) <= 1.0
    # ... and through the consumer: GroupNorm fed with the partials against its own statistics pass over the same stored tensor
    G = N // unit
    HW = 4 * Hi * Wi
    gamma = (1.0 + 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(3))).float()
    beta = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(4))).float()
    wsb = int(L.gyre_op_groupnorm_workspace(B, HW, N, G))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=DEV)
    y1 = torch.empty(B * HW, N, dtype=HDT, device=DEV)
    y2 = torch.empty_like(y1)
    cs = stats.float().to(DEV).contiguous()
    gd, bd = gamma.to(DEV), beta.to(DEV)
    _lib.check(L.gyre_op_groupnorm_colstats(st(), vp(out), None, N, B, HW, N, G, vp(gd), vp(bd), 1e-5, 1, vp(cs), 4 * tps, None, 0, unit,
                                            vp(ws), wsb, vp(y1)))
    _lib.check(L.gyre_op_groupnorm(st(), vp(out), None, N, B, HW, N, G, vp(gd), vp(bd), 1e-5, 1, vp(ws), wsb, vp(y2)))
    torch.cuda.synchronize()
    t = y.reshape(B, HW, G, unit)
    mean = t.mean(dim=(1, 3), keepdim=True)
    var = (t * t).mean(dim=(1, 3), keepdim=True) - mean * mean
    z = ((t - mean) / torch.sqrt(var + 1e-5)).reshape(B * HW, N) * gamma.double() + beta.double()
    ref = z * torch.sigmoid(z)
    # both forms: fp32 statistics (sums of 8192 values: <= 8192 2^-24 = 2^-11 relative on the mean and on E[x^2], so <= ~2^-10 on z,
    # which is 0.25 u (bf16) or 2 u (fp16) of |z|), fp32 affine, one rounding: k = 4 on |z - beta| + |beta| covers SiLU's slope of 1.1
    gb = (z - beta.double()).abs() + beta.double().abs()
    check_bound("groupnorm fed with the partials", y1.float().cpu(), ref, gb, k=4.0)
    check_bound("groupnorm with its own statistics pass", y2.float().cpu(), ref, gb, k=4.0)
    d = (y1.double() - y2.double()).abs().cpu()
    print(f"[ups4 colstats] consumer fed with partials vs own pass: max |diff| = {float(d.max()):.3g}, differing elements {int((d > 0).sum())}")


def test_second_call_follows_the_new_weights():
    name = "ragged-tile-per-parity"
    case = CASES[name]
    x, w, bias, value, _ = nine_tap_ref(name, "lattice")
    _, w2, _ = operands(case, "lattice", seed=7)
    A = R.conv_gather(x, ups=1)
    value_new, _ = R.reference(A.reshape(A.shape[0], -1), w2.reshape(w2.shape[0], -1), bias=bias)
    scratch = torch.empty(16 * case[4] * case[3] + 64, dtype=HDT, device=DEV)
    with Bit30() as L:
        got1, _, _ = run_ups4(L, case, x, w, bias, scratch=scratch)
        got2, _, _ = run_ups4(L, case, x, w2, bias, scratch=scratch)
    assert describe_mismatch("first weights", got1.float().cpu(), R.rne(value, HDT).float(), case) == 0
    assert describe_mismatch("changed weights, same scratch", got2.float().cpu(), R.rne(value_new, HDT).float(), case) == 0
    assert not torch.equal(got1.cpu(), got2.cpu())


def test_refused_without_the_rule_and_bad_arguments():
    """Without bit 30 the small shapes are not the planner's: GYRE_ERR_UNSUPPORTED and no launch, never nine taps instead."""
    name = "ragged-tile-per-parity"
    case = CASES[name]
    x, w, bias, _, _ = nine_tap_ref(name, "lattice")
    L = _lib.lib()
    old = L.gyre_debug_gemm_ablation(0)
    try:
        B, Hi, Wi, Cin, N = case[:5]
        out = torch.full((B * 4 * Hi * Wi, N), CANARY, dtype=HDT, device=DEV)
        xd, wd = x.to(HDT).to(DEV), w.to(HDT).to(DEV)
        scratch = torch.empty(16 * N * Cin, dtype=HDT, device=DEV)
        a = _lib.UpsampleConvTestArgs()
        a.B, a.Hi, a.Wi, a.Cin, a.N = B, Hi, Wi, Cin, N
        a.x, a.w, a.out, a.scratch, a.scratch_bytes = vp(xd).value, vp(wd).value, vp(out).value, vp(scratch).value, scratch.numel() * 2
        assert L.gyre_op_upsample_conv_test(st(), C.byref(a)) == -6
        L.gyre_debug_gemm_ablation(UPS4_ALL)
        a.scratch_bytes = scratch.numel() * 2 - 2
        assert L.gyre_op_upsample_conv_test(st(), C.byref(a)) == -4
        a.scratch_bytes = scratch.numel() * 2
        a.splits = 2                                          # K slices without slab space
        assert L.gyre_op_upsample_conv_test(st(), C.byref(a)) == -4
        a.splits = 0
        a.x = None
        assert L.gyre_op_upsample_conv_test(st(), C.byref(a)) == -1
        assert L.gyre_op_upsample_conv_test(st(), None) == -1
        torch.cuda.synchronize()
        assert bool((out.float() == CANARY).all()), "a refused call wrote to the output"
    finally:
        L.gyre_debug_gemm_ablation(old)
