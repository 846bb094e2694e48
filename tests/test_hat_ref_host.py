"""Self-test of the HAT references (tests/hat_ref.py), on the host: the fp32 emulation of the attention kernel meets the element-wise
bound on every case of the GPU list in both modes, every seeded mistake breaks it, the closed-form mask and indices are the reference's
formulas (the modulo-1521 wrap of the overlapping index included), the channel-attention passes likewise, and the storage-emulation
distance of the whole net - the number the GPU model gates are twice of - is measured and printed per configuration and storage type."""
import pytest
import torch

import hat_ref as R

SDTS = [torch.bfloat16, torch.float16]
# rel-L2 of net(store=dt) against net() on MODEL_CASES, as printed by test_storage_emulation_distance: the table
# tests/test_gpu_hat_model.py imports.  The assertion keeps it honest (a changed net must re-measure).
EMULATION = {("tiny", torch.bfloat16): 7.322e-03, ("tiny", torch.float16): 9.661e-04,
             ("tiny2", torch.bfloat16): 6.570e-03, ("tiny2", torch.float16): 8.421e-04,
             ("w180", torch.bfloat16): 7.669e-03, ("w180", torch.float16): 9.553e-04}
_NET = {}


def _net(name):
    if name not in _NET:
        cfg, sd, x = R.model_case(name)
        _NET[name] = (cfg, sd, x, R.net(sd, cfg, x))
    return _NET[name]


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("case", R.CASES, ids=["-".join(map(str, c)) for c in R.CASES])
def test_emulation_meets_the_bound_on_every_gpu_case(case, sdt):
    L = R.case(sdt, *case)
    worst, rest = R.verdict(L, R.emulate(L))
    print(f"[hat] emulate {sdt} {case}: worst ratio {worst:.3f}")
    assert worst <= 1.0 and rest


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("mode,mistake", [(m, k) for m in ("sa", "oca") for k in R.MISTAKES[m]])
def test_every_seeded_attention_mistake_breaks_the_bound(mode, mistake, sdt):
    broke = []
    for case in (c for c in R.CASES if c[0] == mode):
        L = R.case(sdt, *case)
        worst, _ = R.verdict(L, R.emulate(L, mistake))
        broke.append(worst > 1.0)
    print(f"[hat] {mode} {mistake} {sdt}: breaks the bound on cases {[i for i, b in enumerate(broke) if b]}")
    assert any(broke)


@pytest.mark.parametrize("sdt", SDTS)
def test_cab_emulation_meets_the_bound_and_every_mistake_breaks_it(sdt):
    broke = {m: [] for m in R.MISTAKES["cab"]}
    for case in R.CAB_CASES:
        L = R.cab_case(sdt, *case)
        worst = R.cab_verdict(L, R.cab_emulate(L))
        print(f"[hat] cab emulate {sdt} {case}: worst ratio {worst:.3f}")
        assert worst <= 1.0
        for m in broke:
            broke[m].append(R.cab_verdict(L, R.cab_emulate(L, m)) > 1.0)
    assert all(any(v) for v in broke.values()), broke


@pytest.mark.parametrize("hw", [(16, 16), (16, 32), (32, 48), (48, 32)])
def test_closed_form_mask_is_calculate_mask(hw):
    assert torch.equal(R.region_mask(*hw), R.calculate_mask(*hw))


def test_mask_share_per_window():
    assert float((R.calculate_mask(16, 16) != 0).float().mean()) == 0.75
    share = (R.calculate_mask(32, 48) != 0).float().mean((1, 2)).tolist()
    assert share == [0.0, 0.0, 0.5, 0.5, 0.5, 0.75]


def test_closed_form_indices_are_the_reference_formulas():
    assert torch.equal(R.sa_index_closed(), R.rpi_sa())
    raw = R.rpi_oca()
    assert int(raw.min()) == -880 and int(raw.max()) == 640 and abs(float((raw < 0).float().mean()) - 0.63) < 0.01
    wrapped = R.oca_index_closed()
    assert torch.equal(wrapped, raw % 1521) and int(wrapped.min()) == 0 and int(wrapped.max()) == 1520
    table = torch.arange(1521.0)
    assert torch.equal(table[raw.view(-1)], table[wrapped.view(-1)])            # torch's negative indexing is that wrap
    assert len(torch.unique(wrapped)) == 1521                                   # onto the whole table


def test_pixel_shuffle_nhwc_is_pixel_shuffle():
    x = torch.randn(2, 3, 5, 16)
    want = torch.nn.functional.pixel_shuffle(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(R.pixel_shuffle_nhwc(x), want)


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_storage_emulation_distance(name):
    cfg, sd, x, ref = _net(name)
    assert ref.shape == (x.shape[0], 3, x.shape[2] * cfg["upscale"], x.shape[3] * cfg["upscale"]) and bool(torch.isfinite(ref).all())
    got = {sdt: R.rel_l2(R.net(sd, cfg, x, store=sdt), ref) for sdt in SDTS}
    for sdt, d in got.items():
        print(f"[hat] {name} {sdt}: storage-emulation rel-L2 against the fp32 net {d:.3e}")
    for sdt, d in got.items():
        want = EMULATION[(name, sdt)]
        assert want is not None and abs(d - want) <= 0.02 * want, f"re-measure: {d:.3e}"
