"""Self-test of the SwinIR references (tests/swinir_ref.py), on the host: the fp32 emulation of the window-attention kernel meets
the element-wise bound on every case of the GPU list, every seeded mistake breaks it, the closed-form region mask is the reference's
calculate_mask, and the storage-emulation distance of the whole net - the number the GPU model gates are twice of - is measured and
printed per configuration and storage type."""
import pytest
import torch

import swinir_ref as R

SDTS = [torch.bfloat16, torch.float16]
# rel-L2 of net(store=dt) against net() on MODEL_CASES, as printed by test_storage_emulation_distance: the constants of
# tests/test_gpu_swinir_model.py.  The assertion keeps the two files honest (a changed net must re-measure).
EMULATION = {("tiny", torch.bfloat16): 3.928e-03, ("tiny", torch.float16): 5.073e-04,
             ("tiny3", torch.bfloat16): 3.939e-03, ("tiny3", torch.float16): 4.876e-04,
             ("w180", torch.bfloat16): 3.520e-03, ("w180", torch.float16): 4.663e-04,
             ("w240", torch.bfloat16): 3.192e-03, ("w240", torch.float16): 3.770e-04}


@pytest.mark.parametrize("sdt", SDTS)
def test_emulation_meets_the_bound_on_every_gpu_case(sdt):
    for B, H, W, heads, s in R.CASES:
        L = R.case(sdt, B, H, W, heads, s)
        worst, rest = R.verdict(L, R.emulate(L))
        print(f"[swin] emulate {sdt} {(B, H, W, heads, s)}: worst ratio {worst:.3f}")
        assert worst <= 1.0 and rest


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_seeded_mistake_breaks_the_bound(mistake, sdt):
    broke = []
    for B, H, W, heads, s in R.CASES:
        L = R.case(sdt, B, H, W, heads, s)
        worst, _ = R.verdict(L, R.emulate(L, mistake))
        broke.append(worst > 1.0)
    print(f"[swin] {mistake} {sdt}: breaks the bound on cases {[i for i, b in enumerate(broke) if b]}")
    assert any(broke)


@pytest.mark.parametrize("hw", [(16, 24), (8, 8), (24, 16), (16, 16), (32, 40)])
def test_closed_form_mask_is_calculate_mask(hw):
    assert torch.equal(R.region_mask(*hw, 4), R.calculate_mask(*hw, 4))


def test_expanded_bias_indexing():
    table = torch.arange(225 * 2, dtype=torch.float32).view(225, 2)
    b = R.expanded_bias(table)
    for a, c in ((0, 0), (0, 63), (63, 0), (9, 18), (17, 40)):
        di, dj = (a >> 3) - (c >> 3) + 7, (a & 7) - (c & 7) + 7
        assert b[1, a, c] == table[di * 15 + dj, 1]


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_storage_emulation_distance(name):
    cfg, sd, x = R.model_case(name)
    ref = R.net(sd, cfg, x)
    assert ref.shape == (x.shape[0], 3, x.shape[2] * cfg["upscale"], x.shape[3] * cfg["upscale"]) and bool(torch.isfinite(ref).all())
    got = {sdt: R.rel_l2(R.net(sd, cfg, x, store=sdt), ref) for sdt in SDTS}
    for sdt, d in got.items():
        print(f"[swinir] {name} {sdt}: storage-emulation rel-L2 against the fp32 net {d:.3e}")
    for sdt, d in got.items():
        want = EMULATION[(name, sdt)]
        assert want is not None and abs(d - want) <= 0.02 * want, f"re-measure: {d:.3e}"


def test_net_pads_and_crops_like_check_image_size():
    cfg, sd, x = R.model_case("tiny")
    x = x[:1, :, :13, :21]
    full = R.net(sd, cfg, torch.nn.functional.pad(x, (0, 3, 0, 3), "reflect"))
    assert torch.equal(R.net(sd, cfg, x), full[:, :, :52, :84])
