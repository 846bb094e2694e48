"""Forward GroupNorm / LayerNorm (-m gpu): every kernel path of csrc/kernels_elem.hip and the statistics finish of the GEMM epilogue
against float64, element by element, with the conditioned tolerance of tests/norm_fwd_ref.py (derivation there; its constants are
fixed by the fp32 emulation of tests/test_norm_fwd_ref_host.py).  Outputs start as NaN sentinels, concat sources are separate
allocations.  `expects_small` asks the library (gyre_debug_gn_uses_small) which kernel a shape runs; the two-pass kernels get the
two-pass fp32 term, every other path the one-pass one.  Every check name starts with its kernel path in angle brackets, and next to
each `[bound]` line an `[fp32]` line gives the lower bound of the device's fp32 error that the stored value still shows
(norm_fwd_ref.fp32_floor): with k this small the rounded ratio reaches 1 from the store alone, so that line, not the rounded ratio,
is what compares the device with the host emulation.

Cases the code answers differently from what their names suggest: 7 x 5 at C = 320 has cpg = 10 (not a multiple of 4) and runs the
large path - 7 x 5 at C = 384 is the ragged-last-vector case of k_gn_small; 129 x 129 runs 66 chunks of 253 pixels (last 196), see
test_chunk_rule_matches_the_cases_the_gpu_tests_name.  gyre_op_gn_fold takes one source, so a C1 != C call cannot be formed."""
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import norm_fwd_ref as R
from gyre_amd import _lib
from gpu_util import HDT, DEV, check_bound, rel_l2, release_kept, repack_bias, repack_linear, st, vp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SEPARATE = os.environ.get("GYRE_GN_SEPARATE_FINALIZE") is not None


def dev16(t):
    return t.to(HDT).contiguous().to(DEV)


def expects_small(HW, C, C1, G):
    return bool(_lib.lib().gyre_debug_gn_uses_small(HW, C, C1, G))


def path_of(HW, C, C1, G):
    if expects_small(HW, C, C1, G):
        return "k_gn_small"
    nv = (C // 8 + 255) // 256
    return f"large-{nv}v" + (" separate-finalize" if SEPARATE else "")


def run_gn(x, C1, G, gamma, beta, eps, silu, cs=None, expect=0):
    """x [B, HW, C] float32 of 16-bit values; C1 in (0, C): two sources.  cs = (cs_a, chunks_a, cs_b, chunks_b, unit): producer statistics."""
    L = _lib.lib()
    B, HW, C = x.shape
    two = 0 < C1 < C
    a = dev16(x[..., :C1]) if two else dev16(x)
    b = dev16(x[..., C1:]) if two else None
    y = torch.full((B, HW, C), NAN, dtype=HDT, device=DEV)
    wsb = L.gyre_op_groupnorm_workspace(B, HW, C, G)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    g, bt = gamma.float().to(DEV), beta.float().to(DEV)
    if cs is None:
        rc = L.gyre_op_groupnorm(st(), vp(a), vp(b), C1 if two else 0, B, HW, C, G, vp(g), vp(bt), eps, silu, vp(ws), wsb, vp(y))
    else:
        cs_a, na, cs_b, nb, unit = cs
        rc = L.gyre_op_groupnorm_colstats(st(), vp(a), vp(b), C1 if two else 0, B, HW, C, G, vp(g), vp(bt), eps, silu,
                                          vp(cs_a.to(DEV)), na, vp(cs_b.to(DEV)) if two else None, nb if two else 0, unit, vp(ws), wsb, vp(y))
    release_kept()
    assert rc == expect, rc
    return y.float().cpu()


# B, H, W, C, C1, G: the plain GroupNorm cases (gyre_op_groupnorm)
GN_CASES = [
    (3, 1, 1, 128, 0, 32),            # k_gn_small: one pixel
    (2, 9, 9, 2080, 0, 8),            # k_gn_small: cpg = 260 > GNS_MAXC, gamma / beta from global memory
    (2, 16, 16, 3072, 0, 32),         # k_gn_small: exactly 24 vectors per thread
    (3, 16, 16, 384, 200, 32),        # k_gn_small: the concat split falls inside group 16
    (3, 7, 5, 384, 0, 32),            # k_gn_small: ragged last vector (105 vectors over 256 threads)
    (3, 7, 5, 320, 0, 32),            # cpg = 10: large path at 35 pixels (three chunks of 12 / 12 / 11)
    (2, 16, 16, 3200, 0, 32),         # one vector over the k_gn_small limit: large path, two vectors per thread
    (3, 1, 257, 320, 0, 32),          # one pixel over HW = 256; last chunk = 1 pixel
    (3, 8, 8, 64, 0, 32),             # cpg = 2
    (3, 33, 33, 320, 0, 32),          # PY = 6 with idle lanes; last chunk = 1 pixel
    (2, 65, 65, 64, 0, 32),           # PY = 32
    (2, 33, 33, 1280, 0, 32),         # PY = 1, 17-pixel chunks: a second GN_U trip
    (2, 129, 129, 64, 0, 32),         # VAE-sized chunks: many GN_U trips
    (2, 33, 33, 960, 640, 32),        # group 21 straddles the two sources
    (2, 33, 33, 2048, 0, 32),         # the last C with one vector per lane
    (2, 17, 17, 2560, 1280, 32),      # two vectors per thread, two sources
    (2, 17, 17, 5120, 0, 32),         # three
    (2, 17, 17, 8192, 0, 32),         # four
    (3, 33, 33, 192, 0, 8),           # 256 / G = 32 parts
    (3, 33, 33, 192, 0, 24),          # 256 / G = 10 parts, 16 idle threads
    (2, 17, 17, 2048, 0, 256),        # one part, one group per thread
]


def _case_id(c):
    return "x".join(str(v) for v in c)


def _gn_case(i, B, H, W, C, C1, G, mean_sigma, first=None, tag="gn"):
    HW, silu, eps = H * W, (i + 1) % 2, (1e-5, 1e-6)[(i // 2) % 2]
    x, gamma, beta = R.gn_inputs(B, HW, C, G, HDT, mean_sigma=mean_sigma, seed=10 * i, first=first)
    got = run_gn(x, C1, G, gamma, beta, eps, silu)
    one_pass = not expects_small(HW, C, C1 if C1 else C, G)
    name = f"<{path_of(HW, C, C1 if C1 else C, G)}> {tag} {B}x{H}x{W}x{C} C1={C1} G={G} silu={silu} eps={eps} {'one' if one_pass else 'two'}-pass mean={mean_sigma} first={first}"
    return R.gn_check(name, got, x, G, gamma, beta, eps, silu, one_pass, HDT), x, got, (gamma, beta, eps, silu, one_pass)


@pytest.mark.parametrize("mean_sigma", [0.3, 8.0])
@pytest.mark.parametrize("case", list(enumerate(GN_CASES)), ids=lambda c: _case_id(c[1]))
def test_groupnorm_elementwise(case, mean_sigma):
    i, (B, H, W, C, C1, G) = case
    _gn_case(i, B, H, W, C, C1, G, mean_sigma)


@pytest.mark.parametrize("case", [(0, GN_CASES[2]), (1, GN_CASES[9]), (2, GN_CASES[11]), (3, GN_CASES[15]), (4, GN_CASES[16]),
                                  (5, GN_CASES[17])], ids=lambda c: _case_id(c[1]))
def test_groupnorm_sample_at_64_sigma(case):
    """Sample 0 at 64 standard deviations: the one-pass paths must stay inside the conditioned tolerance."""
    i, (B, H, W, C, C1, G) = case
    _gn_case(i, B, H, W, C, C1, G, 0.3, first=64.0, tag="gn 64 sigma")


def test_two_pass_against_one_pass_error_at_64_sigma_on_neighbouring_shapes():
    """HW = 256 runs k_gn_small (two-pass), HW = 257 the one-pass chunked path: the same family, the error of each against float64
    in units of the PLAIN tolerance (no conditioning term) - on record, not asserted beyond the bound each path is held to."""
    out = {}
    for HW in (256, 257):
        x, gamma, beta = R.gn_inputs(2, HW, 384, 32, HDT, seed=77, first=64.0)
        C = x.shape[-1]
        got = run_gn(x, 0, 32, gamma, beta, 1e-5, 0)
        one_pass = not expects_small(HW, C, C, 32)
        assert one_pass == (HW == 257)
        R.gn_check(f"<{path_of(HW, C, C, 32)}> neighbour HW={HW}", got, x, 32, gamma, beta, 1e-5, 0, one_pass, HDT)
        ref, bound, _ = R.gn_ref(x[:1], 32, gamma, beta, 1e-5, 0, one_pass)
        out[HW] = check_bound(f"neighbour HW={HW}, plain tolerance", got[:1], ref, bound, k=R.k_of(HDT), dims=R.GN_DIMS, enforce=False)
    print(f"[record] 64 sigma, error / unconditioned tolerance: two-pass (HW 256) {out[256]:.3g}, one-pass (HW 257) {out[257]:.3g}, "
          f"one-pass / two-pass {out[257] / out[256]:.3g}")


def test_groupnorm_refusals():
    x = torch.zeros(1, 16, 8200)
    run_gn(x, 0, 8, torch.ones(8200), torch.zeros(8200), 1e-5, 0, expect=-6)              # five vectors per thread
    x = torch.zeros(1, 289, 2056)
    run_gn(x, 0, 257, torch.ones(2056), torch.zeros(2056), 1e-5, 0, expect=-1)            # more than 256 groups


def test_groupnorm_apply_fin_4_headline_shape():
    """B = 16, 64 x 64, C = 320: 42 MB, the smallest tensor that reaches k_gn_apply_fin<4> (>= 32 MiB and nchunks B <= 1024)."""
    t0 = time.time()
    B, HW, C, G = 16, 4096, 320, 32
    assert B * HW * C * 2 >= 32 << 20 and 64 * B <= 1024
    x, gamma, beta = R.gn_inputs(B, HW, C, G, HDT, mean_sigma=8.0, seed=500)
    got = run_gn(x, 0, G, gamma, beta, 1e-5, 1)
    R.gn_check("<apply_fin4> 16x64x64x320", got, x, G, gamma, beta, 1e-5, 1, True, HDT)
    print(f"[time] apply_fin<4> case {time.time() - t0:.1f} s")


# ---- producer statistics --------------------------------------------------------------------------------------------------
def _colstats(x_src, rows, unit):
    """[B][HW / rows][C / unit][2] float32 from float64 sums of the stored values."""
    B, HW, C = x_src.shape
    t = x_src.double().reshape(B, HW // rows, rows, C // unit, unit)
    return torch.stack([t.sum(dim=(2, 4)), (t * t).sum(dim=(2, 4))], dim=-1).float().contiguous()


@pytest.mark.parametrize("first", [None, 64.0])
@pytest.mark.parametrize("mean_sigma", [0.3, 8.0])
@pytest.mark.parametrize("B,H,W,C1,C2,unit,rows_a,rows_b", [
    (3, 32, 32, 320, 0, 10, 256, 16), (2, 32, 32, 320, 320, 5, 256, 16), (3, 24, 32, 64, 0, 2, 256, 16),
    (2, 32, 32, 640, 320, 10, 256, 16), (2, 32, 32, 320, 320, 10, 16, 256)])
def test_groupnorm_from_producer_statistics_elementwise(B, H, W, C1, C2, unit, rows_a, rows_b, mean_sigma, first):
    """Both routes (host-made float64 partials of the stored tensor; the kernel's own statistics pass) against float64."""
    HW, C, G = H * W, C1 + C2, 32
    x, gamma, beta = R.gn_inputs(B, HW, C, G, HDT, mean_sigma=mean_sigma, seed=C + unit, first=first)
    cs = (_colstats(x[..., :C1], rows_a, unit), HW // rows_a, _colstats(x[..., C1:], rows_b, unit) if C2 else None, HW // rows_b, unit)
    silu, eps = unit % 2, 1e-5 if unit != 5 else 1e-6
    got = run_gn(x, C1 if C2 else 0, G, gamma, beta, eps, silu, cs=cs)
    own = run_gn(x, C1 if C2 else 0, G, gamma, beta, eps, silu)
    name = f"{B}x{H}x{W} {C1}+{C2} unit {unit} rows {rows_a}/{rows_b} mean={mean_sigma} first={first}"
    R.gn_check(f"<producer-statistics> gn {name}", got, x, G, gamma, beta, eps, silu, True, HDT)
    R.gn_check(f"<{path_of(HW, C, C1, G)}> gn own statistics {name}", own, x, G, gamma, beta, eps, silu, True, HDT)


# ---- the GroupNorm fold -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,N,bias,producer,mean_sigma", [
    (3, 65, 65, 320, 320, 1, 0, 8.0), (3, 65, 65, 320, 320, 1, 1, 8.0), (2, 33, 33, 640, 640, 0, 0, 0.3),
    (2, 17, 17, 1280, 38, 1, 0, 8.0), (3, 33, 33, 64, 8, 1, 1, 0.3), (2, 33, 33, 320, 6, 0, 0, 64.0)])
def test_gn_fold_weights_and_bias(B, H, W, C, N, bias, producer, mean_sigma):
    L = _lib.lib()
    HW, G, unit, eps = H * W, 32, (10 if C == 320 else 2), 1e-6
    x, gamma, beta = R.gn_inputs(B, HW, C, G, HDT, mean_sigma=0.3, seed=C + N, first=mean_sigma)
    W_ = R.q16(R.randn(N, C, seed=C + N + 5) / math.sqrt(C), HDT)
    bias_t = 0.3 * R.randn(N, seed=C + N + 6) if bias else None
    tail = 64
    wf = torch.full((B * N * C + tail,), NAN, dtype=HDT, device=DEV)
    bf = torch.full((B * N + tail,), NAN, dtype=torch.float32, device=DEV)
    wsb = L.gyre_op_groupnorm_workspace(B, HW, C, G)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    cs, chunks = None, 0
    if producer:
        rows = W                                                      # one map row per block: HW / rows = H chunks
        cs, chunks = _colstats(x, rows, unit).to(DEV), HW // rows
    rc = L.gyre_op_gn_fold(st(), vp(dev16(x)), B, HW, C, G, vp(gamma.to(DEV)), vp(beta.to(DEV)), eps, vp(dev16(W_)),
                           vp(bias_t.to(DEV)) if bias else None, N, vp(cs) if producer else None, chunks, unit if producer else 0,
                           vp(ws), wsb, vp(wf), vp(bf))
    release_kept()
    assert rc == 0, rc
    assert bool(torch.isnan(wf[B * N * C:]).all()) and bool(torch.isnan(bf[B * N:]).all()), "the fold wrote behind its outputs"
    wf_ref, wf_tiny, bf_ref, bf_tol = R.fold_ref(x, G, gamma, beta, eps, W_, bias_t)
    name = f"<fold> gn_fold {B}x{H}x{W} C{C} N{N} bias={bias} producer={producer} first={mean_sigma}"
    check_bound(f"{name} weights", wf[:B * N * C].float().cpu().reshape(B, N, C), wf_ref, wf_ref.abs(), k=R.k_of(HDT), tiny=wf_tiny,
                dims=("sample", "row", "channel"))
    R.fp32_floor(f"{name} weights", wf[:B * N * C].float().cpu().reshape(B, N, C), wf_ref, wf_ref.abs(), wf_tiny, R.k_of(HDT), HDT)
    R.check_abs(f"{name} bias", bf[:B * N].cpu().reshape(B, N), bf_ref, bf_tol)


def test_gn_fold_rejections():
    L = _lib.lib()
    B, HW, C, G, N = 1, 1089, 320, 32, 8
    x, g, w = torch.zeros(B, HW, C, dtype=HDT, device=DEV), torch.ones(C, device=DEV), torch.zeros(N, C, dtype=HDT, device=DEV)
    wf, bf = torch.zeros(B, N, C, dtype=HDT, device=DEV), torch.zeros(B, N, device=DEV)
    wsb = L.gyre_op_groupnorm_workspace(B, HW, C, G)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    cs = torch.zeros(B, 33, C // 10, 2, device=DEV)
    call = lambda unit, cs_, wsb_=wsb, x_=x: L.gyre_op_gn_fold(st(), vp(x_), B, HW, C, G, vp(g), vp(g), 1e-5, vp(w), None, N,
                                                               vp(cs_) if cs_ is not None else None, 33, unit, vp(ws), wsb_, vp(wf), vp(bf))
    assert call(3, cs) == -1 and call(0, cs) == -1             # a unit that does not divide the group / no unit
    assert call(0, None, wsb_=16) == -4
    assert L.gyre_op_gn_fold(st(), None, B, HW, C, G, vp(g), vp(g), 1e-5, vp(w), None, N, None, 0, 0, vp(ws), wsb, vp(wf), vp(bf)) == -1
    assert call(10, cs) == 0
    release_kept()


# ---- the separate-finalize form ----------------------------------------------------------------------------------------------
@pytest.mark.skipif(SEPARATE, reason="already inside the separate-finalize run")
def test_plain_groupnorm_cases_pass_with_the_separate_finalize_kernels():
    """k_gn_finalize + k_gn_apply (the form every call that asks for mean / rstd takes) on this file's plain GroupNorm cases."""
    t0 = time.time()
    env = dict(os.environ, GYRE_GN_SEPARATE_FINALIZE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_norm_fwd.py", "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "test_groupnorm_elementwise or test_groupnorm_sample_at_64_sigma"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    worst = max([float(l.split("worst ratio ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[bound]")] or [NAN])
    low = max([float(l.split(">= ")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("[fp32]")] or [NAN])
    tail = "\n".join(r.stdout.splitlines()[-15:])
    print(tail)
    print(f"[record] separate finalize: worst ratio {worst:.3g}, device fp32 part >= {low:.3g}; child run {time.time() - t0:.1f} s")
    assert r.returncode == 0, f"separate finalize failed:\n{tail}\n{r.stderr[-2000:]}"


# ---- exact properties ----------------------------------------------------------------------------------------------------------
PROP_CASES = [(2, 16, 16, 384, 200, 32), (2, 16, 16, 384, 0, 32), (2, 33, 33, 320, 0, 32), (2, 33, 33, 960, 640, 32), (2, 17, 17, 2560, 1280, 32), (2, 17, 17, 8192, 0, 32)]


@pytest.mark.parametrize("B,H,W,C,C1,G", PROP_CASES, ids=lambda v: str(v))
def test_groupnorm_exact_properties(B, H, W, C, C1, G):
    HW, cpg = H * W, C // G
    x, gamma, beta = R.gn_inputs(B, HW, C, G, HDT, mean_sigma=0.3, seed=C)
    # all-zero input: exactly round16(beta).  With SiLU bit-exactness against round16(silu(beta)) does not hold by construction: silu_f
    # is v_exp_f32 / v_rcp_f32 (1 ulp each) in fp32, and a beta whose silu lies within 2^-23 of a 16-bit rounding boundary may store the
    # neighbour.  So there: every pixel of every sample carries the same bits, and those are held to the float64 silu(beta) with the
    # module's bound (x = 0: xh = 0, ref = silu(beta), kappa = 0).
    z = torch.zeros(B, HW, C)
    assert torch.equal(run_gn(z, C1, G, gamma, beta, 1e-5, 0), R.q16(beta.float(), HDT).expand(B, HW, C))
    zs = run_gn(z, C1, G, gamma, beta, 1e-5, 1)
    assert torch.equal(zs, zs[:1, :1].expand(B, HW, C))
    R.gn_check(f"<{path_of(HW, C, C1 if C1 else C, G)}> zero input with SiLU {B}x{H}x{W}x{C}", zs[:1], z[:1], G, gamma, beta, 1e-5, 1,
               not expects_small(HW, C, C1 if C1 else C, G), HDT)
    # x -> 2 x, eps -> 4 eps: sums, mean and variance scale by exact powers of two, rsqrt(4 v) = rsqrt(v) / 2 bit for bit (the exponent
    # moves by two, the mantissa path is the same), so a x + b is unchanged - on every path by construction
    eps = float(np.float32(1e-5))
    base = run_gn(x, C1, G, gamma, beta, eps, 1)
    assert torch.equal(run_gn(2 * x, C1, G, gamma, beta, float(np.float32(4) * np.float32(1e-5)), 1), base)
    # a sample alone equals the sample inside the batch
    assert torch.equal(run_gn(x[1:2], C1, G, gamma, beta, eps, 1), base[1:2])
    # permuting whole groups (with gamma / beta) permutes the output; one source (a permutation would move channels across the split)
    if not C1:
        perm = torch.randperm(G, generator=torch.Generator().manual_seed(3))
        idx = (perm[:, None] * cpg + torch.arange(cpg)[None, :]).reshape(-1)
        assert torch.equal(run_gn(x[..., idx].contiguous(), 0, G, gamma[idx], beta[idx], eps, 1), base[..., idx])


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def run_ln(x, gamma, beta, eps, expect=0):
    L = _lib.lib()
    M, C = x.shape
    y = torch.full((M, C), NAN, dtype=HDT, device=DEV)
    rc = L.gyre_op_layernorm(st(), vp(dev16(x)), M, C, vp(gamma.float().to(DEV)), vp(beta.float().to(DEV)), eps, vp(y))
    release_kept()
    assert rc == expect, rc
    return y.float().cpu()


@pytest.mark.parametrize("M,C", [(1, 8), (6, 64), (7, 320), (5, 512), (3, 520), (33, 1280), (2, 2048)])
def test_layernorm_elementwise(M, C):
    """Every row ordinary: means from -1 to 1 plus 0 / 8 / 64 sigma in turn (M = 1: one row at 8 sigma, M = 2: 8 and 64).  The constant
    row is a second launch of the same shape, so it replaces no ordinary row."""
    sig = (0.0, 8.0, 64.0) if M >= 3 else (8.0, 64.0)
    x, gamma, beta = R.ln_inputs(M, C, HDT, seed=M + C, sigmas=sig)
    got = run_ln(x, gamma, beta, 1e-5)
    ref, bound, tiny = R.ln_ref(x, gamma, beta, 1e-5)
    check_bound(f"<k_layernorm> layernorm {M}x{C}", got, ref, bound, k=R.k_of(HDT), tiny=tiny, dims=("row", "channel"))
    R.fp32_floor(f"<k_layernorm> layernorm {M}x{C}", got, ref, bound, tiny, R.k_of(HDT), HDT)
    xc = x.clone()
    xc[M // 2] = 1.375                                               # exact in both storage types: mean = 1.375, d = 0: round16(beta)
    gc = run_ln(xc, gamma, beta, 1e-5)
    assert torch.equal(gc[M // 2], R.q16(beta.float(), HDT))
    keep = [m for m in range(M) if m != M // 2]
    assert torch.equal(gc[keep], got[keep])                          # and the other rows do not notice


def test_layernorm_refuses_wide_rows():
    run_ln(torch.zeros(2, 2056), torch.ones(2056), torch.zeros(2056), 1e-5, expect=-6)


# ---- LayerNorm folded into the consuming GEMM ---------------------------------------------------------------------------------------
def _smallest_folded_m(K, N, geglu, need_parts):
    """The smallest M for which the planner keeps the folded form (and, need_parts, gives the producing K x K linear with a residual the
    row-statistics epilogue): asked of the planner on the host, one M after the other."""
    L = _lib.lib()
    for M in range(1, (1 << 17) + 1):
        if L.gyre_debug_ln_linear_folds(M, K, N, geglu) and (not need_parts or L.gyre_op_linear_rowstats_parts(M, K, K, 1) > 0):
            return M
    return 0


def _ln_linear(xd, M, K, gamma, beta, W_, bias, N, geglu, parts=None, nparts=0):
    L = _lib.lib()
    rows = 2 * N if geglu else N
    ws = torch.empty(L.gyre_op_ln_linear_workspace(rows, K, M), dtype=torch.uint8, device=DEV)
    y = torch.full((M, N), NAN, dtype=HDT, device=DEV)
    rc = L.gyre_op_ln_linear(st(), vp(xd), M, K, vp(gamma.to(DEV)), vp(beta.to(DEV)), 1e-5, vp(repack_linear(W_, geglu=bool(geglu))), N,
                             vp(repack_bias(bias, geglu=bool(geglu))), geglu, 0, None, 0, vp(parts) if parts is not None else None, nparts,
                             vp(ws), ws.numel(), vp(y))
    release_kept()
    assert rc == 0, rc                                              # the planner said it folds (gyre_debug_ln_linear_folds): -6 is a failure
    return y.float().cpu()


@pytest.mark.parametrize("K", [320, 640, 1280])
def test_ln_linear_elementwise_pass_and_parts(K):
    """Rows at 0.3, 8 and 64 sigma in one tensor, at the smallest M the planner keeps folded.  Statistics from the pass (two-pass
    fp32 term) and from the producer's row partials (one-pass term; kappa from the producer's STORED 16-bit output)."""
    L = _lib.lib()
    N = K
    M = _smallest_folded_m(K, N, 0, True)
    if not M:
        pytest.skip("planner picks a tile config without the row-statistics epilogue for this shape")
    nparts = L.gyre_op_linear_rowstats_parts(M, K, K, 1)
    r, gamma, beta = R.ln_inputs(M, K, HDT, seed=K, sigmas=(0.3, 8.0, 64.0))
    x0 = R.q16(R.randn(M, K, seed=K + 1), HDT)
    w1 = R.q16(R.randn(K, K, seed=K + 2) / math.sqrt(K) * 0.5, HDT)
    y1 = torch.full((M, K), NAN, dtype=HDT, device=DEV)
    stats = torch.full((nparts, M, 2), NAN, device=DEV)
    rc = L.gyre_op_linear_rowstats(st(), vp(dev16(x0)), M, K, vp(repack_linear(w1)), K, None, vp(dev16(r)), vp(y1), vp(stats))
    release_kept()
    assert rc == 0, rc
    x = y1.float().cpu()                                            # what both routes normalise
    W_ = R.q16(R.randn(N, K, seed=K + 3) / math.sqrt(K), HDT)
    bias = 0.3 * R.randn(N, seed=K + 4)
    out_s = _ln_linear(y1, M, K, gamma, beta, W_, bias, N, 0)
    out_p = _ln_linear(y1, M, K, gamma, beta, W_, bias, N, 0, parts=stats, nparts=nparts)
    for name, got, from_parts in (("pass", out_s, False), ("parts", out_p, True)):
        ref, bound, tiny = R.ln_linear_ref(x, gamma, beta, 1e-5, W_, bias, from_parts)
        check_bound(f"<ln_linear {name}> M{M} K{K} N{N}", got, ref, bound, k=R.k_ln_linear(HDT), tiny=tiny, dims=("row", "column"))
        R.fp32_floor(f"<ln_linear {name}> M{M} K{K} N{N}", got, ref, bound, tiny, R.k_ln_linear(HDT), HDT)
    assert rel_l2(out_p, out_s) < 2e-3


def test_ln_linear_geglu_elementwise():
    K, F_ = 320, 1280
    M = _smallest_folded_m(K, F_, 1, False)
    if not M:
        pytest.skip("planner picks a tile config without the folded form for this shape")
    x, gamma, beta = R.ln_inputs(M, K, HDT, seed=K + 20, sigmas=(0.3, 8.0, 64.0))
    W_ = R.q16(R.randn(2 * F_, K, seed=K + 21) / math.sqrt(K), HDT)
    bias = 0.5 * R.randn(2 * F_, seed=K + 22)
    got = _ln_linear(dev16(x), M, K, gamma, beta, W_, bias, F_, 1)
    ref, bound, tiny = R.ln_linear_ref(x, gamma, beta, 1e-5, W_, bias, False)
    (v, g), (bv, bg), (tv, tg) = ref.chunk(2, -1), bound.chunk(2, -1), tiny.chunk(2, -1)
    # d (v gelu(g)) <= |gelu(g)| dv + |v| sup|gelu'| dg, sup |gelu'| = 1.129; the kernel's erfc form is within 7.1e-7 of gelu (common.h)
    ge = R.gelu64(g)
    check_bound(f"<ln_linear geglu> M{M} K{K} F{F_}", got, v * ge, ge.abs() * bv + 1.13 * v.abs() * bg, k=R.k_ln_linear(HDT),
                tiny=ge.abs() * tv + 1.13 * v.abs() * tg + 1e-6 * v.abs(), dims=("row", "column"))
