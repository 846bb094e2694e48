"""Self-test of the line-art references (tests/lineart_ref.py), on the host: the storage-emulation distance of the whole net - the number
the GPU model gates are twice of - is measured, printed and re-checked per case and storage type; the sub-pixel form of the transposed
convolution is the layer; every seeded mistake exceeds the GPU gate that can see it; the fp32 emulation of each kernel meets its
derived element bound.

Which gate sees which mistake.  Seven of the nine move the net's output far beyond the model gate (2 x EMULATION) on every
MODEL_CASES entry.  eps = 1e-3 can only touch a plane whose variance is of eps' own order: the "quiet" entry (first-layer weights at a
tenth of their scale, plane variances 4e-4 .. 1.1e-3) is there for it - every channel is rescaled by its own factor, the next
convolution mixes them, and the output moves by 2.4e-2 against a gate of 1.0e-2; on the other entries (variances about 1) it moves
6.0e-4 .. 7.9e-3 and no gate can see it.  The same entry holds the eps the graph itself passes to the statistics kernel.  The
unbiased variance rescales a whole plane by sqrt((n - 1) / n), the same factor for every channel, which the NEXT instance
normalisation removes again whatever the weights are; what reaches the output is the residual sum's mixing ratio and the last plane's
scale, 6.7e-5 .. 3.8e-3 against gates of 1.1e-3 .. 3.7e-2.  It is held by the statistics kernel's own bounds instead
(tests/test_gpu_lineart_kernels.py asserts rstd and the normalised values on every plane; below: on the residual-level plane of every
MODEL_CASES entry the mistake breaks them).  The GPU kernel list also runs a "quiet" input family, on which eps = 1e-3 breaks the
element bound (below)."""
import pytest
import torch

import lineart_ref as R

SDTS = [torch.bfloat16, torch.float16]
# rel-L2 of net(store=dt) against net() on MODEL_CASES, as printed by test_storage_emulation_distance: the table
# tests/test_gpu_lineart_model.py imports.  The assertion keeps it honest (a changed net must re-measure).
EMULATION = {("tiny", torch.bfloat16): 1.854e-02, ("tiny", torch.float16): 2.193e-03,
             ("shipped", torch.bfloat16): 4.307e-03, ("shipped", torch.float16): 5.410e-04,
             ("odd", torch.bfloat16): 1.704e-02, ("odd", torch.float16): 1.850e-03,
             ("deep", torch.bfloat16): 8.510e-03, ("deep", torch.float16): 9.275e-04,
             ("quiet", torch.bfloat16): 5.147e-03, ("quiet", torch.float16): 6.369e-04}
MODEL_MISTAKES = [m for m in R.MISTAKES if m != "unbiased_variance"]
# the MODEL_CASES entries a mistake can touch: all of them, except that a wrong eps needs a plane whose variance is of eps' order
TOUCHES = {m: (("quiet",) if m == "eps_1e-3" else tuple(R.MODEL_CASES)) for m in MODEL_MISTAKES}
_NET = {}


def _net(name):
    if name not in _NET:
        cfg, sd, x = R.model_case(name)
        _NET[name] = (cfg, sd, x, R.net(sd, cfg, x))
    return _NET[name]


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_storage_emulation_distance(name, sdt):
    cfg, sd, x, ref = _net(name)
    assert tuple(ref.shape) == (x.shape[0], 1, R.out_size(x.shape[2]), R.out_size(x.shape[3]))
    d = R.rel_l2(R.net(sd, cfg, x, store=sdt), ref)
    print(f'[lineart] ("{name}", {sdt}): {d:.3e}')
    assert abs(d - EMULATION[(name, sdt)]) <= 0.02 * EMULATION[(name, sdt)]


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_subpixel_form_is_the_transposed_convolution(name):
    cfg, sd, x, ref = _net(name)
    d = R.rel_l2(R.net(sd, cfg, x, mistake="tconv_none"), ref)        # (any name starting with "tconv" takes the sub-pixel path)
    print(f"[lineart] {name}: sub-pixel form against F.conv_transpose2d {d:.3e}")
    assert d <= 1e-5


@pytest.mark.parametrize("mistake", MODEL_MISTAKES)
def test_seeded_mistake_exceeds_the_model_gate_on_every_case(mistake):
    for name in TOUCHES[mistake]:
        cfg, sd, x, ref = _net(name)
        d = R.rel_l2(R.net(sd, cfg, x, mistake=mistake), ref)
        gate = 2 * max(EMULATION[(name, dt)] for dt in SDTS)
        print(f"[lineart] {mistake} on {name}: {d:.3e} (widest gate {gate:.3e})")
        assert d > gate


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("shape", R.INORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", R.INORM_FAMILIES)
def test_inorm_emulation_meets_the_bound(family, shape, sdt):
    x = R.inorm_input(sdt, *shape, family=family)
    m, rstd, y, t = R.inorm_ref(x)
    _, _, got = R.inorm_emulate(x)
    worst = R.verdict(got.to(sdt), y, R.stored_bound(y, t, sdt))
    print(f"[lineart] inorm emulate {family} {shape} {sdt}: worst ratio {worst:.3f}")
    assert worst <= 1.0
    if family == "constant":
        assert float(got[0, :, :, 0].abs().max()) == 0.0 and float(got[-1].abs().max()) == 0.0


def _residual_plane(name):
    _, _, shape = R.MODEL_CASES[name]
    return R.out_size(shape[2]) // 4, R.out_size(shape[3]) // 4


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_unbiased_variance_breaks_the_kernel_bound_on_every_case(name, sdt):
    h, w = _residual_plane(name)
    x = R.inorm_input(sdt, 1, h, w, 256)
    _, _, y, t = R.inorm_ref(x)
    n = h * w
    wrong = y * ((n - 1) / n) ** 0.5
    worst = R.verdict(wrong.float().to(sdt), y, R.stored_bound(y, t, sdt))
    _, rstd, _, _, _, drstd = R.inorm_stats_ref(x)
    stat = float((rstd * (1 - ((n - 1) / n) ** 0.5) / drstd).min())
    print(f"[lineart] unbiased variance on the {h} x {w} plane of {name} {sdt}: worst ratio {worst:.2f}, rstd off by {stat:.0f} x its bound")
    assert worst > 1.0 and stat > 1.0


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("shape", R.INORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eps_1e_3_breaks_the_kernel_bound_on_the_quiet_family(shape, sdt):
    x = R.inorm_input(sdt, *shape, family="quiet")
    m, _, y, t = R.inorm_ref(x)
    wrong = R.inorm_ref(x, eps=1e-3)[2]
    worst = R.verdict(wrong.float().to(sdt), y, R.stored_bound(y, t, sdt))
    print(f"[lineart] eps 1e-3 on planes of variance {float(x.double().var((1, 2)).mean()):.2e} {shape} {sdt}: worst ratio {worst:.1f}")
    assert worst > 1.0


@pytest.mark.parametrize("sdt", SDTS)
def test_conv7_bounds_hold_for_fp32_and_see_the_mistakes(sdt):
    B, H, W = R.CONV7_SHAPES[0]
    x, w, b = R.conv7_in_case(sdt, B, H, W)
    ref, t = R.conv7_in_ref(x, w, b)
    fp32 = torch.nn.functional.conv2d(torch.nn.functional.pad(x.float(), (3,) * 4, "reflect"), w.float(), b).permute(0, 2, 3, 1)
    assert R.verdict(fp32.to(sdt), ref, R.stored_bound(ref, t, sdt)) <= 1.0
    assert R.verdict(R.conv7_in_ref(x, w, b, "zero_padding")[0].float().to(sdt), ref, R.stored_bound(ref, t, sdt)) > 1.0
    xp, w, b = R.conv7_out_case(sdt, B, H, W)
    for sig in (0, 1):
        ref, t = R.conv7_out_ref(xp, w, b, sig)
        bound = R.stored_bound(ref, t, torch.float32)
        v = torch.nn.functional.conv2d(xp.float().permute(0, 3, 1, 2), w.float(), b)
        assert R.verdict(torch.sigmoid(v) if sig else v, ref, bound) <= 1.0
        assert R.verdict(R.conv7_out_ref(xp, w, b, sig, "final_bias_dropped")[0].float(), ref, bound) > 1.0


@pytest.mark.parametrize("widths", R.TCONV_WIDTHS)
def test_composed_weights_and_patch_rows_are_the_layer(widths):
    cin, cout = widths
    x, w, b = R.tconv_case(torch.float16, 2, 2, 3, cin, cout)
    ref, t = R.tconv_ref(x, w, b)
    wc = R.compose_tconv(w.double())
    blocks = wc.reshape(4, cout, 4, cin).abs().amax((1, 3))
    assert int((blocks == 0).sum()) == 7                              # the seven absent blocks
    got = R.unshuffle_rows(torch.nn.functional.linear(R.patch_rows(x.double()), wc, b.double().repeat(4)), cout)
    assert float((got - ref).abs().max()) <= 1e-12
    bound = R.stored_bound(ref, t, torch.float16)
    for mistake in ("tconv_parities_swapped", "tconv_kernel_not_flipped", "tconv_edge_wrapped"):
        wrong = R.tconv_subpixel(x.double().permute(0, 3, 1, 2), w.double(), b.double(), mistake).permute(0, 2, 3, 1)
        assert R.verdict(wrong.float().to(torch.float16), ref, bound) > 1.0, mistake
