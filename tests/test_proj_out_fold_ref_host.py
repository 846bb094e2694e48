"""Host checks of tests/proj_out_fold_ref.py (no GPU): the identity behind the proj_out fold in float64, the seeded mistakes, and
the error bounds against an fp32 emulation of the stated operation order."""
import pytest
import torch

import proj_out_fold_ref as R

F64 = torch.float64


@pytest.mark.parametrize("C", [64, 192])
def test_identity_in_float64(C):
    Wp, W2, b2, bp = R.operands(C, 1, torch.bfloat16)
    ff, h, x = R.activations(37, C, 2, torch.bfloat16)
    two = R.two_launch(ff, h, x, Wp, W2, b2, bp)
    one = R.folded_with(ff, h, x, Wp, W2, b2, bp)
    # two float64 evaluation orders of sums of <= 5 C products of O(1) values
    tol = 5 * C * 2.0 ** -52 * 64
    assert float((one - two).abs().max()) <= tol * float(two.abs().max())
    Wc, bc = R.compose(Wp, W2, b2, bp)
    assert Wc.shape == (C, 5 * C) and bc.shape == (C,)
    assert torch.equal(Wc[:, 4 * C:], Wp)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_mistake_fails_the_comparison(mistake):
    C = 64
    Wp, W2, b2, bp = R.operands(C, 3, torch.bfloat16)
    ff, h, x = R.activations(29, C, 4, torch.bfloat16)
    two = R.two_launch(ff, h, x, Wp, W2, b2, bp)
    bad = R.folded_with(ff, h, x, Wp, W2, b2, bp, mistake)
    rel = float((bad - two).norm() / two.norm())
    good = float((R.folded_with(ff, h, x, Wp, W2, b2, bp) - two).norm() / two.norm())
    assert good < 1e-12
    assert rel > 1e-2, (mistake, rel)          # far above the 3e-2 / 1e-3 scale of the model gates' resolution on one layer


@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [64, 192])
def test_fp32_emulation_meets_the_bounds_and_mistakes_do_not(C, hdt):
    Wp, W2, b2, bp = R.operands(C, 5, hdt)
    Wc, bc = R.compose(Wp, W2, b2, bp)
    got_w, got_b = R.emulate_fp32(Wp, W2, b2, bp, hdt)
    tw, tb = R.wc_bound(Wp, W2, hdt), R.bc_bound(Wp, b2, bp)
    assert bool(((got_w.to(F64) - Wc).abs() <= tw).all())
    assert bool(((got_b.to(F64) - bc).abs() <= tb).all())
    # the bound is of the size of a storage rounding, far below the weights themselves: every seeded composition mistake breaks it
    assert float(tw[:, :4 * C].max()) < 2.0 ** -6 * float(Wc.abs().max())
    for m in ("wp_missing_on_h", "w2_transposed"):
        bad_w, _ = R.compose(Wp, W2, b2, bp, m)
        assert not bool(((bad_w - Wc).abs() <= tw).all()), m
    _, bad_b = R.compose(Wp, W2, b2, bp, "b2_not_through_wp")
    assert not bool(((bad_b - bc).abs() <= tb).all())
