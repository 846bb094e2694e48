"""Host self-test of the time-embedding error model (tests/temb_ref.py): a numpy fp32 emulation of the kernels' expressions and
summation order stays under HALF of every tolerance (the constants C1, C2, s and 8 ceil(K / 512) + 7 come from the derivation in
that module's docstring), and every seeded mistake exceeds it."""
import pytest
import torch

import temb_ref as R
from gpu_util import check_bound

DIMS, KS, NS = (8, 256, 320), (8, 320, 512, 520, 1280, 2056), (1, 3, 17)
ROWS = 5


def _emb_ratio(got, t, dim, flip, shift):
    ref, a = R.embedding64(t, dim, flip, shift)
    return float(((torch.as_tensor(got).double() - ref).abs() / R.embedding_tolerance(a)).max())


def test_embedding_emulation_stays_under_half_the_tolerance():
    worst = 0.0
    for dim in DIMS:
        for flip in (0, 1):
            for shift in (0.0, 1.0):
                t = R.timesteps(16)
                worst = max(worst, _emb_ratio(R.embedding_emulate_f32(t, dim, flip, shift), t, dim, flip, shift))
    print(f"[emul] embedding: worst ratio {worst:.3f} of (C1 |a| + C2) 2^-24, C1 = {R.C1}, C2 = {R.C2}")
    assert worst <= 0.5


def test_silu_emulation_stays_under_half_the_tolerance():
    x = torch.cat([torch.linspace(-80, 80, 20001), R.linear_inputs(2056, 1, ROWS, 7)[0].flatten()])
    got = torch.from_numpy(R.silu_emulate_f32(x.numpy())).double()
    ref = R.silu64(x)
    ratio = (got - ref).abs() / (R.silu_s(x) * R.U32 * ref.abs() + 2.0 ** -150)
    print(f"[emul] silu: worst ratio {float(ratio.max()):.3f} of s(x) 2^-24 |silu(x)| at x = {float(x[int(ratio.argmax())]):.3f}")
    assert float(ratio.max()) <= 1.0
    # s(x) is a sum of worst cases, and most of them are plain IEEE roundings that this emulation and every device perform alike -
    # the argument product (2 |x| sigmoid(-x), sharp: z just above a power of two, off by half an ulp), the addition and the last
    # multiply (1 each): those parts may be used up.  Where an implementation may differ from the emulation - exp2 and the
    # reciprocal, budgeted at 1 ulp = 2 units each, correctly rounded here - at most HALF of the budget may be used.
    sig = torch.sigmoid(-x.double())
    ieee = 2.0 * x.double().abs() * sig + 2.0
    impl = 2.0 * sig + 2.0
    assert float((ieee + impl - R.silu_s(x)).abs().max()) < 1e-12
    ratio = ((got - ref).abs() / (R.U32 * ref.abs() + 2.0 ** -150) - ieee).clamp_min(0.0) / impl
    print(f"[emul] silu: worst ratio {float(ratio.max()):.3f} of the exp2 / rcp budget at x = {float(x[int(ratio.argmax())]):.3f}")
    assert float(ratio.max()) <= 0.5


@pytest.mark.parametrize("wdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_linear_emulation_stays_under_half_the_tolerance(wdt):
    worst = 0.0
    for K in KS:
        for N in NS:
            x, W, bias = R.linear_inputs(K, N, ROWS, seed=K + N)
            W = W.to(wdt).float()
            for silu in (False, True):
                for bi in (None, bias):
                    fx = R.silu_emulate_f32(x.numpy()) if silu else x.numpy()
                    got = R.linear_emulate_f32(fx, W.numpy(), None if bi is None else bi.numpy())
                    ref, bound = R.linear64(x, W, bi, silu)
                    worst = max(worst, check_bound(f"emulation K{K} N{N} silu{int(silu)} bias{int(bi is not None)}", torch.from_numpy(got), ref,
                                                   bound, k=1.0, hdt=torch.float32))
    print(f"[emul] linear ({wdt}): worst ratio {worst:.3f}")
    assert worst <= 0.5


# ---- seeded mistakes ------------------------------------------------------------------------------------------------------------------
def _emb_mistake(t, dim, flip, shift, mistake):
    half = dim // 2
    i = torch.arange(dim, dtype=torch.float64)
    if mistake != "index j in the second half":
        i = torch.where(i < half, i, i - half)
    den = half if mistake == "shift ignored" else half - shift
    a = t.double()[:, None] * torch.exp(-R.LN10000 * i / den)[None, :]
    first = torch.arange(dim) < half
    is_cos = first if flip else ~first
    if mistake == "sin / cos swapped for flip = 0" and not flip:
        is_cos = ~is_cos
    return torch.where(is_cos[None, :], torch.cos(a), torch.sin(a))


@pytest.mark.parametrize("mistake", ["shift ignored", "sin / cos swapped for flip = 0", "index j in the second half"])
def test_seeded_embedding_mistakes_are_caught(mistake):
    caught, clean = [], 0.0
    for dim in DIMS:
        for flip in (0, 1):
            for shift in (0.0, 1.0):
                t = R.timesteps(5)
                clean = max(clean, _emb_ratio(_emb_mistake(t, dim, flip, shift, None), t, dim, flip, shift))
                if _emb_ratio(_emb_mistake(t, dim, flip, shift, mistake), t, dim, flip, shift) > 1.0:
                    caught.append((dim, flip, shift))
    print(f"[seeded] {mistake}: caught at (dim, flip, shift) = {caught}")
    assert clean < 1e-6 and caught


def _lin_mistake(x, W, bias, silu, mistake):
    xd, Wd = x.double(), W.double()
    K = x.shape[1]
    fx = R.silu64(xd) if silu else xd
    if mistake == "SiLU applied twice" and silu:
        fx = R.silu64(fx)
    if mistake == "SiLU missing":
        fx = xd
    if mistake == "last k chunk dropped":                # the lanes' last trip: columns from the last multiple of 512 below K on
        fx = fx.clone()
        fx[:, (K - 1) // 512 * 512:] = 0.0
    out = fx @ Wd.t()
    if bias is not None:
        b = bias.double()
        if mistake == "bias of column n0 for the whole group":
            b = b[torch.arange(len(b)) // 4 * 4]
        out = out + b[None, :]
    return out


@pytest.mark.parametrize("mistake", ["last k chunk dropped", "bias of column n0 for the whole group", "SiLU applied twice", "SiLU missing"])
def test_seeded_linear_mistakes_are_caught(mistake):
    caught = []
    for K in KS:
        for N in NS:
            x, W, bias = R.linear_inputs(K, N, ROWS, seed=K + N)
            W = W.to(torch.bfloat16).float()
            for silu in (False, True):
                ref, bound = R.linear64(x, W, bias, silu)
                assert check_bound("clean copy", _lin_mistake(x, W, bias, silu, None), ref, bound, k=1.0, hdt=torch.float32) < 1e-6
                if check_bound(mistake, _lin_mistake(x, W, bias, silu, mistake), ref, bound, k=1.0, hdt=torch.float32, enforce=False) > 1.0:
                    caught.append((K, N, int(silu)))
    print(f"[seeded] {mistake}: caught at (K, N, silu) = {caught}")
    assert caught
    if mistake == "last k chunk dropped":
        assert any(c[0] == 2056 for c in caught)         # the chunk beyond the first 2048 columns
