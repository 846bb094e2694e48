"""Host self-test of the forward normalisation error model (tests/norm_fwd_ref.py): no GPU.

Each algorithm of csrc/kernels_elem.hip is emulated in numpy float32 in the kernel's summation order and judged with the same
check the GPU tests use, for both storage types:
  one-pass chunked GroupNorm   the chunk rule of gn_pick_chunks; a lane adds its pixel rows in turn (sum, fma sum of squares), then
                               the PY lanes of a channel, the channels of a group, every parts-th chunk, the parts; var = E[x^2] - mean^2;
                               y = fma(rstd gamma, x, beta - mean rstd gamma)
  two-pass GroupNorm           k_gn_small: a thread's vectors in turn, butterfly over the wave, four waves; centred second pass
  two-pass LayerNorm           k_layernorm: the same over one wave
  ln_parts finish              partial (sum, sum of squares) per 160-column tile, finished as the GEMM epilogue does, then
                               rstd acc - rstd mean colsum + bias' over gamma-folded, rounded weights (gyre_op_ln_linear)
The emulation, not the code under test, sets C32_* of norm_fwd_ref.  Two ratios are printed per path, storage type and group mean
(0 / 8 / 32 / 128 / 512 sigma, `[emu]` lines):
  fp32 part       the fp32 result BEFORE the rounding to 16 bits against the tolerance WITHOUT its u |ref| term: what K32 and C32_*
                  govern.  C32_* are chosen so that its worst value is <= 0.5 (a factor 2 for the device's different but equally
                  long order); asserted <= 0.7.
  rounded output  the stored 16-bit value against the full tolerance, judged with hdt=.  The norm kernels round to 16 bits exactly
                  once, so the storage rounding alone reaches u |ref| and this ratio approaches 1 by construction (0.99 at benign
                  means); asserted <= 1.
Worst fp32 part when the constants were fixed (C32_ONE = 10, C32_TWO = 4, C32_GEMM = 8), bf16 / fp16:
  one-pass GroupNorm 0.42 / 0.44 (129 x 129 at 8 and 128 sigma), two-pass GroupNorm 0.42 / 0.40, LayerNorm 0.35 / 0.29,
  ln_linear statistics pass 0.13 / 0.10, ln_linear from row partials 0.10 / 0.10 (dominated by the one 16-bit rounding of the
  folded weights at small means).  Rounded output: 0.996 at most on the norm paths, 0.15 on ln_linear.

Seeded mistakes (mean 0.3 sigma, `enforce=False`) must exceed ratio 1; their rel-L2 is printed next to the ratio to show which of
them the whole-tensor rel-L2 <= 4e-3 of tests/test_gpu_kernels.py lets through."""
import numpy as np
import pytest
import torch

import norm_fwd_ref as R

F32 = np.float32
DTS = (torch.bfloat16, torch.float16)
SIGMAS = (0.0, 8.0, 32.0, 128.0, 512.0)


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


def pick_chunks(HW):
    ppc = min(max(HW // 64, 16), 256)
    return max((HW + ppc - 1) // ppc, 1)


def _fma_sq(f, acc):
    """fmaf(f, f, acc): f holds 16-bit values, so f * f is exact in float64 and the one rounding is that of the sum."""
    return (f.astype(np.float64) ** 2 + acc.astype(np.float64)).astype(F32)


def _rsqrt(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F32)


def _silu32(v):
    return (v / (F32(1.0) + np.exp(-v, dtype=F32))).astype(F32)


def emu_gn_one_pass(x, G, gamma, beta, eps, silu, bug=None):
    """x [B, HW, C] float32 holding 16-bit values -> float32 [B, HW, C] before the output rounding."""
    B, HW, C = x.shape
    cpg, CV = C // G, C // 8
    nch = pick_chunks(HW)
    ppc = (HW + nch - 1) // nch
    TX = min(CV, 256)
    PY = max(256 // TX, 1)
    part = np.zeros((B, nch, G, 2), F32)
    for ch in range(nch):
        p0, p1 = ch * ppc, min(HW, (ch + 1) * ppc)
        if bug == "drop_pixel" and ch == 0:
            p1 -= 1
        if bug == "skip_last_chunk" and ch == nch - 1:
            continue
        n = p1 - p0
        rows = (n + PY - 1) // PY
        blk = np.zeros((B, rows * PY, C), F32)
        blk[:, :n] = x[:, p0:p1]
        blk = blk.reshape(B, rows, PY, C)                       # pixel p0 + ty + i * PY belongs to lane row ty
        s, ss = np.zeros((B, PY, C), F32), np.zeros((B, PY, C), F32)
        for i in range(rows):
            s = s + blk[:, i]
            ss = _fma_sq(blk[:, i], ss)
        a, b = np.zeros((B, C), F32), np.zeros((B, C), F32)
        for y in range(PY):
            a, b = a + s[:, y], b + ss[:, y]
        a, b = a.reshape(B, G, cpg), b.reshape(B, G, cpg)
        ga, gb = np.zeros((B, G), F32), np.zeros((B, G), F32)
        for c in range(cpg):
            ga, gb = ga + a[:, :, c], gb + b[:, :, c]
        part[:, ch, :, 0], part[:, ch, :, 1] = ga, gb
    parts = max(256 // G, 1)
    sa, sb = np.zeros((B, G), F32), np.zeros((B, G), F32)
    for q in range(parts):
        a, b = np.zeros((B, G), F32), np.zeros((B, G), F32)
        for ch in range(q, nch, parts):
            a, b = a + part[:, ch, :, 0], b + part[:, ch, :, 1]
        sa, sb = sa + a, sb + b
    cnt = F32(HW - 1 if bug == "cnt" else HW) * F32(cpg)
    mean = sa / cnt
    var = np.maximum(sb / cnt - mean * mean, F32(0))
    rstd = _rsqrt(var + F32(eps))
    if bug == "next_group":
        mean, rstd = np.roll(mean, 1, axis=1), np.roll(rstd, 1, axis=1)
    g, bt = gamma.astype(F32), beta.astype(F32)
    if bug == "gb_shift":
        g, bt = np.roll(g, 4), np.roll(bt, 4)
    aa = np.repeat(rstd, cpg, axis=1) * g[None, :]
    bb = bt[None, :] - np.repeat(mean, cpg, axis=1) * aa
    y = (aa[:, None, :].astype(np.float64) * x + bb[:, None, :]).astype(F32)         # one fma
    return _silu32(y) if silu and bug != "no_silu" else y


def _thread_sum(v, nthreads):
    """v [..., n] summed as a workgroup does: thread t adds elements t, t + nthreads, ... in turn, then the butterfly
    (lane i + lane i ^ off: halving) over the threads."""
    n = v.shape[-1]
    V = (n + nthreads - 1) // nthreads
    pad = np.zeros(v.shape[:-1] + (V * nthreads,), F32)
    pad[..., :n] = v
    pad = pad.reshape(v.shape[:-1] + (V, nthreads))
    s = np.zeros(v.shape[:-1] + (nthreads,), F32)
    for i in range(V):
        s = s + pad[..., i, :]
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def emu_two_pass(v, gamma, beta, eps, nthreads, silu=False, bug=None):
    """v [S, n] (one normalised set per row, gamma / beta [S, n] or [n]) -> float32 [S, n]: k_gn_small (256 threads) / k_layernorm (64)."""
    n = v.shape[-1]
    cnt = F32(n)
    mean = _thread_sum(v, nthreads) / cnt
    d = v - mean[:, None]
    q = _thread_sum((d.astype(np.float64) ** 2).astype(F32), nthreads)
    rstd = _rsqrt(q / (cnt - F32(1) if bug == "unbiased" else cnt) + F32(eps))
    y = d * rstd[:, None] * gamma.astype(F32) + beta.astype(F32)
    return _silu32(y) if silu else y


def emu_gn_small(x, G, gamma, beta, eps, silu, bug=None):
    B, HW, C = x.shape
    cpg = C // G
    v = x.reshape(B, HW, G, cpg).transpose(0, 2, 1, 3).reshape(B * G, HW * cpg)
    g = np.tile(gamma.reshape(G, 1, cpg), (B, HW, 1)).reshape(B * G, HW * cpg)
    b = np.tile(beta.reshape(G, 1, cpg), (B, HW, 1)).reshape(B * G, HW * cpg)
    y = emu_two_pass(v, g, b, eps, 256, silu, bug)
    return y.reshape(B, G, HW, cpg).transpose(0, 2, 1, 3).reshape(B, HW, C)


def emu_ln_linear(x, gamma, beta, eps, W, bias, dt, from_parts, tile=160):
    """The folded LayerNorm -> GEMM in float32: k_ln_fold (weights rounded after the gamma scaling, column sum over the rounded
    weights, beta W in fp32), statistics from the two-pass kernel or from per-tile partial sums, the epilogue's
    rstd acc - rstd mean colsum + bias'."""
    M, K = x.shape
    wf = R.q16(torch.from_numpy(W.astype(F32) * gamma.astype(F32)[None, :]), dt).numpy()
    colsum = _thread_sum(wf, 64)
    bb = _thread_sum(W.astype(F32) * beta.astype(F32)[None, :], 64) + (bias.astype(F32) if bias is not None else F32(0))
    if from_parts:
        su, sq = np.zeros(M, F32), np.zeros(M, F32)
        for t0 in range(0, K, tile):
            ps, pq = np.zeros(M, F32), np.zeros(M, F32)
            for k in range(t0, min(K, t0 + tile)):
                ps, pq = ps + x[:, k], pq + x[:, k] * x[:, k]
            su, sq = su + ps, sq + pq
        invk = F32(1.0) / F32(K)
        mean = su * invk
        rstd = (F32(1.0) / np.sqrt(np.maximum(sq * invk - mean * mean, F32(0)) + F32(eps))).astype(F32)
    else:
        mean = _thread_sum(x, 64) / F32(K)
        d = x - mean[:, None]
        rstd = _rsqrt(_thread_sum((d.astype(np.float64) ** 2).astype(F32), 64) / F32(K) + F32(eps))
    acc = np.zeros((M, W.shape[0]), F32)
    for k0 in range(0, K, 16):                                   # fp32 accumulation, one MFMA K step at a time
        acc = acc + (x[:, k0:k0 + 16].astype(np.float64) @ wf[:, k0:k0 + 16].astype(np.float64).T).astype(F32)
    return rstd[:, None] * acc - (rstd * mean)[:, None] * colsum[None, :] + bb[None, :]


def _sigma_batch(HW, C, G, dt, seed):
    """One sample per entry of SIGMAS (scale 1.5, as the suite's family), the sample mean at that many standard deviations."""
    x = R.randn(len(SIGMAS), HW, C, seed=seed) + torch.tensor(SIGMAS)[:, None, None]
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 1))
    return R.q16(x * 1.5, dt), gamma, 0.2 * R.randn(C, seed=seed + 2)


def _gn_pre(got32, x, G, gamma, beta, eps, silu, one_pass, dt):
    ref, bound, tiny = R.gn_ref(x, G, gamma, beta, eps, silu, one_pass)
    return R.fp32_ratio(got32, ref, bound, tiny, R.k_of(dt, silu), dt)


def _per_sigma(fn):
    return [fn(i) for i in range(len(SIGMAS))]


def _report(path, dt, ratios, pre):
    """ratios: the rounded output against the full tolerance (<= 1: the storage rounding alone reaches u |ref|); pre: the fp32 result
    BEFORE that rounding against the tolerance WITHOUT the u |ref| term - the part C32_* govern (<= 0.5 by their choice, asserted <= 0.7)."""
    sig = "/".join(str(int(s)) for s in SIGMAS)
    print(f"[emu] {path} {_name(dt)}: fp32 part at {sig} sigma: " + " ".join(f"{r:.3f}" for r in pre)
          + " | rounded output: " + " ".join(f"{r:.3f}" for r in ratios))
    assert max(pre) <= 0.7 and max(ratios) <= 1.0, (path, _name(dt), pre, ratios)


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("HW,C,G,silu,eps", [(1089, 320, 32, 1, 1e-5), (4225, 64, 32, 0, 1e-6), (16641, 32, 8, 1, 1e-6), (289, 2560, 32, 0, 1e-5)])
def test_one_pass_groupnorm_emulation_meets_the_bound(HW, C, G, silu, eps, dt):
    x, gamma, beta = _sigma_batch(HW, C, G, dt, seed=HW)
    got32 = torch.from_numpy(emu_gn_one_pass(x.numpy(), G, gamma.numpy(), beta.numpy(), eps, silu))
    got = R.q16(got32, dt)
    _report(f"one-pass GroupNorm {HW}x{C} G{G} silu{silu}", dt,
            _per_sigma(lambda i: R.gn_check(f"emu one-pass {SIGMAS[i]} sigma", got[i:i + 1], x[i:i + 1], G, gamma, beta, eps, silu, True, dt)),
            _per_sigma(lambda i: _gn_pre(got32[i:i + 1], x[i:i + 1], G, gamma, beta, eps, silu, True, dt)))


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("HW,C,G,silu", [(256, 128, 32, 1), (64, 1280, 32, 0), (81, 2080, 8, 1)])
def test_two_pass_groupnorm_emulation_meets_the_bound(HW, C, G, silu, dt):
    x, gamma, beta = _sigma_batch(HW, C, G, dt, seed=HW + 1)
    got32 = torch.from_numpy(emu_gn_small(x.numpy(), G, gamma.numpy(), beta.numpy(), 1e-5, silu))
    got = R.q16(got32, dt)
    _report(f"two-pass GroupNorm {HW}x{C} G{G} silu{silu}", dt,
            _per_sigma(lambda i: R.gn_check(f"emu two-pass {SIGMAS[i]} sigma", got[i:i + 1], x[i:i + 1], G, gamma, beta, 1e-5, silu, False, dt)),
            _per_sigma(lambda i: _gn_pre(got32[i:i + 1], x[i:i + 1], G, gamma, beta, 1e-5, silu, False, dt)))


def _sigma_rows(C, dt, seed, per=3):
    x = R.randn(len(SIGMAS) * per, C, seed=seed) + torch.tensor(SIGMAS).repeat_interleave(per)[:, None]
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 1))
    return R.q16(x * 1.5, dt), gamma, 0.2 * R.randn(C, seed=seed + 2), per


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("C", [64, 320, 2048])
def test_layernorm_emulation_meets_the_bound(C, dt):
    x, gamma, beta, per = _sigma_rows(C, dt, seed=C)
    got32 = torch.from_numpy(emu_two_pass(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, 64))
    got = R.q16(got32, dt)
    ref, bound, tiny = R.ln_ref(x, gamma, beta, 1e-5)
    _report(f"two-pass LayerNorm C{C}", dt, _per_sigma(lambda i: R.gpu_util.check_bound(
        f"emu layernorm {SIGMAS[i]} sigma", got[i * per:(i + 1) * per], ref[i * per:(i + 1) * per], bound[i * per:(i + 1) * per],
        k=R.k_of(dt), tiny=tiny[i * per:(i + 1) * per], hdt=dt)),
        _per_sigma(lambda i: R.fp32_ratio(got32[i * per:(i + 1) * per], ref[i * per:(i + 1) * per], bound[i * per:(i + 1) * per],
                                          tiny[i * per:(i + 1) * per], R.k_of(dt), dt)))


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("from_parts", [False, True], ids=["pass", "parts"])
@pytest.mark.parametrize("K", [320, 1280])
def test_ln_linear_emulation_meets_the_bound(K, from_parts, dt):
    x, gamma, beta, per = _sigma_rows(K, dt, seed=K + 7)
    W = R.q16(R.randn(24, K, seed=K + 8) / K ** 0.5, dt)
    bias = 0.3 * R.randn(24, seed=K + 9)
    got32 = torch.from_numpy(emu_ln_linear(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, W.numpy(), bias.numpy(), dt, from_parts))
    got = R.q16(got32, dt)
    ref, bound, tiny = R.ln_linear_ref(x, gamma, beta, 1e-5, W, bias, from_parts)
    _report(f"ln_linear K{K} {'parts' if from_parts else 'pass'}", dt, _per_sigma(lambda i: R.gpu_util.check_bound(
        f"emu ln_linear {SIGMAS[i]} sigma", got[i * per:(i + 1) * per], ref[i * per:(i + 1) * per], bound[i * per:(i + 1) * per],
        k=R.k_ln_linear(dt), tiny=tiny[i * per:(i + 1) * per], hdt=dt)),
        _per_sigma(lambda i: R.fp32_ratio(got32[i * per:(i + 1) * per], ref[i * per:(i + 1) * per], bound[i * per:(i + 1) * per],
                                          tiny[i * per:(i + 1) * per], R.k_ln_linear(dt), dt)))


# ---------------------------------------------------------------------------------------------------------------------------
# seeded mistakes
# ---------------------------------------------------------------------------------------------------------------------------
def _benign(HW, C, G, dt, seed, scale=1.5):
    x = (R.randn(2, HW, C, seed=seed) + 0.3) * scale
    gamma = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 1))
    return R.q16(x, dt), gamma, 0.2 * R.randn(C, seed=seed + 2)


def _misread_x2(x, C1):
    """The second source of a concat read with the first one's row stride (pixel * C1 + c into a [HW][C2] buffer, wrapped at its end)."""
    B, HW, C = x.shape
    C2 = C - C1
    flat = x[:, :, C1:].reshape(B, HW * C2)
    idx = (torch.arange(HW)[:, None] * C1 + torch.arange(C2)[None, :]) % (HW * C2)
    bad = x.clone()
    bad[:, :, C1:] = flat[:, idx.reshape(-1)].reshape(B, HW, C2)
    return bad


MISTAKES = ["drop_pixel", "skip_last_chunk", "cnt", "next_group", "x2_stride", "gb_shift", "eps", "unbiased", "no_silu"]


@pytest.mark.parametrize("dt", DTS, ids=_name)
@pytest.mark.parametrize("bug", MISTAKES)
def test_seeded_mistakes_exceed_the_bound(bug, dt):
    HW, C, G, eps, silu = 257, 64, 32, 1e-5, 1
    if bug == "unbiased":
        HW, C, G = 16, 128, 32                                        # HW * cpg = 64, the two-pass kernel
    if bug == "x2_stride":
        C = 96
    x, gamma, beta = _benign(HW, C, G, dt, seed=31, scale=0.01 if bug == "eps" else 1.5)
    xin, eps_run = x, eps
    if bug == "eps":
        eps, eps_run = 1e-6, 1e-5
    if bug == "x2_stride":
        xin = _misread_x2(x, 64)
    args = (xin.numpy(), G, gamma.numpy(), beta.numpy(), eps_run, silu)
    run = emu_gn_small if bug == "unbiased" else emu_gn_one_pass
    good = R.q16(torch.from_numpy((emu_gn_small if bug == "unbiased" else emu_gn_one_pass)(x.numpy(), *args[1:4], eps, silu)), dt)
    got = R.q16(torch.from_numpy(run(*args, bug=bug)), dt)
    one_pass = bug != "unbiased"
    assert R.gn_check(f"correct emulation for {bug}", good, x, G, gamma, beta, eps, silu, one_pass, dt) <= 1.0
    ratio = R.gn_check(f"seeded {bug}", got, x, G, gamma, beta, eps, silu, one_pass, dt, enforce=False)
    ref = torch.cat([R.gn_ref(x[b:b + 1], G, gamma, beta, eps, silu, one_pass)[0] for b in range(x.shape[0])])
    e = R.rel_l2(got, ref)
    print(f"[mistake] {bug} {_name(dt)}: ratio {ratio:.3g}, rel-L2 {e:.2e} ({'passes' if e <= 4e-3 else 'fails'} rel-L2 <= 4e-3)")
    assert ratio > 1.0, (bug, ratio)


def test_chunk_rule_matches_the_cases_the_gpu_tests_name():
    """33 x 33: 17-pixel chunks, the last one holds one pixel; 257 and 17 x 17: 16-pixel chunks, last one pixel.  The launch spreads
    the pixels over the chunk COUNT of gn_pick_chunks (ppc = ceil(HW / nchunks)), so 129 x 129 runs 66 chunks of 253 pixels (last
    196), not 256-pixel chunks with a one-pixel tail, and 65 x 65 exactly 65 chunks of 65."""
    for HW, ppc, last in ((1089, 17, 1), (16641, 253, 196), (4225, 65, 65), (257, 16, 1), (289, 16, 1)):
        n = pick_chunks(HW)
        p = (HW + n - 1) // n
        assert (p, HW - (n - 1) * p) == (ppc, last), (HW, n, p)


def test_small_path_query_answers_the_shapes_the_gpu_tests_rely_on():
    """tests/test_gpu_norm_fwd.py asks gyre_debug_gn_uses_small which fp32 term a case is held to; the named boundary shapes pin it
    (HW <= 256, groups of whole 4-channel vectors on both sources, at most 24 vectors per thread)."""
    from gyre_amd import _lib
    for storage in (_lib.BF16, _lib.F16):
        L = _lib.lib(storage)
        for (HW, C, C1, G), want in (((1, 128, 128, 32), 1), ((81, 2080, 2080, 8), 1), ((256, 3072, 3072, 32), 1), ((256, 384, 200, 32), 1),
                                     ((35, 384, 384, 32), 1), ((35, 320, 320, 32), 0), ((256, 3200, 3200, 32), 0), ((257, 320, 320, 32), 0),
                                     ((64, 64, 64, 32), 0), ((256, 384, 202, 32), 0), ((1089, 320, 320, 32), 0)):
            assert L.gyre_debug_gn_uses_small(HW, C, C1, G) == want, (HW, C, C1, G)
        assert L.gyre_debug_ln_linear_folds(0, 320, 320, 0) == 0
