"""The parity algebra behind the four-parity upsampler form (tests/ups4_ref.py) against the nine-tap gather of tests/gemm_ref.py
(conv_gather(ups=1), itself checked against F.interpolate + F.conv2d in tests/test_gemm_ref_host.py), in float64.  No GPU.

Both sides compute the same sums of products in float64 in different orders: they agree to rounding noise (1e-12 of the
absolute-value sum allows ~4500 ulps on sums of <= 1152 products).  Three seeded mistakes must each be caught."""
import pytest
import torch

import gemm_ref as R
import ups4_ref as U4

F64 = torch.float64
# (B, Hi, Wi, C, N): square, non-square, odd sizes, a single row / column
SHAPES = [(2, 4, 4, 8, 8), (1, 5, 3, 8, 16), (3, 3, 7, 16, 8), (2, 1, 6, 8, 8), (1, 6, 1, 8, 8), (1, 1, 1, 8, 8)]


def operands(shape, seed=0):
    B, Hi, Wi, Cc, N = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Hi, Wi, Cc, generator=g, dtype=F64), torch.randn(N, 3, 3, Cc, generator=g, dtype=F64)


def nine_tap(x, W):
    A = R.conv_gather(x, ups=1)
    M, _, Cc = A.shape
    A, Wm = A.reshape(M, 9 * Cc), W.reshape(W.shape[0], 9 * Cc)
    return A @ Wm.T, A.abs() @ Wm.abs().T


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_four_parity_convs_equal_the_nine_tap_gather(shape):
    x, W = operands(shape)
    want, bound = nine_tap(x, W)
    got = U4.forward(x, U4.compose(W))
    err = float(((got - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"[ups4 ref] {shape}: max |diff| / sum|x||w| = {err:.3g}")
    assert got.shape == want.shape and err < 1e-12


@pytest.mark.parametrize("bug", ["a1_grouping", "hw_swapped", "replicate"])
def test_seeded_mistakes_are_caught(bug):
    caught = []
    for shape in SHAPES[:3]:
        x, W = operands(shape, seed=1)
        want, bound = nine_tap(x, W)
        got = U4.forward(x, U4.compose(W, bug=bug), bug=bug)
        caught.append(float(((got - want).abs() / bound.clamp_min(1e-300)).max()) > 1e-3)
    assert all(caught), (bug, caught)


def test_composed_weights_sum_one_two_two_or_four_taps():
    W = torch.ones(8, 3, 3, 8, dtype=F64)
    Wc = U4.compose(W)
    # parity (a, b): rows {1 | 2} taps for a = 0, {2 | 1} for a = 1; columns alike
    for a in (0, 1):
        for b in (0, 1):
            ny, nx = ((1, 2), (2, 1))[a], ((1, 2), (2, 1))[b]
            want = torch.tensor([[ny[0] * nx[0], ny[0] * nx[1]], [ny[1] * nx[0], ny[1] * nx[1]]], dtype=F64)
            assert torch.equal(Wc[2 * a + b, 0, :, :, 0], want)
    assert float(Wc.sum()) == float(W.sum()) * 4         # every nine-tap weight appears once per parity


def test_blocked_order_places_every_element():
    Wc = torch.arange(4 * 8 * 4 * 64, dtype=F64).reshape(4, 8, 2, 2, 64)
    flat = U4.blocked(Wc)
    m = Wc.reshape(32, 256)
    for r, k in [(0, 0), (7, 63), (8, 0), (9, 65), (31, 255), (17, 130)]:
        assert flat[((r >> 3) * 4 + (k >> 6)) * 512 + (r & 7) * 64 + (k & 63)] == m[r, k]
