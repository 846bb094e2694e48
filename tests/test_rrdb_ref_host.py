"""The reference side of the RRDBNet tests holds itself to its own bound (CPU only): the fp32 host emulation of the dense-block
convolution stays inside the derived element-wise bound for every epilogue form, seeded mistakes leave it, the exact-lattice data is
exact, and the storage-rounding emulation of the whole net - the yardstick of the GPU model gates - is measured here."""
import pytest
import torch

import rrdb_ref as R
from gyre_amd import config as gcfg, weights

SDTS = [torch.bfloat16, torch.float16]
# the rel-L2 of the storage-rounding emulation against the fp32 net that tests/test_gpu_rrdb_model.py gates at twice of
# (measured by test_storage_emulation_distance on [2, 3, 24, 20], seed 0; keep the two files in step)
MODEL_CASES = [dict(scale=4), dict(scale=2), dict(scale=1), dict(scale=4, plus=True)]


def _launch(sdt, form, **kw):
    a = dict(B=1, H=9, W=11, Cin=96, NT=32, live=32, ldx=192, ldo=192, c0=96, form=form)
    if form in ("block", "rrdb", "body"):
        a.update(Cin=192 if form != "body" else 64, NT=64, live=64, c0=0)
    a.update(kw)
    return R.launch(sdt, **a)


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("form", R.FORMS)
def test_emulation_meets_the_bound(sdt, form):
    for ups in (0, 1):
        L = _launch(sdt, form, ups=ups)
        worst, rest = R.verdict(L, R.emulate(L))
        print(f"[rrdb-ref] {form} ups={ups} {sdt}: host emulation worst err / bound {worst:.3f}")
        assert worst <= 1.0 and rest


@pytest.mark.parametrize("sdt", SDTS)
def test_live_mask_and_source_poison(sdt):
    L = R.launch(sdt, 2, 5, 7, 64, 32, 3, 64, 8, 0, form="plain")            # conv_last: 3 live channels of 8
    got = R.emulate(L)
    worst, rest = R.verdict(L, got)
    assert worst <= 1.0 and rest and bool(torch.isnan(got[..., 3:]).all()) and not bool(torch.isnan(got[..., :3]).any())
    L = _launch(sdt, "act", Cin=32)                                           # NaN from channel 32 on must never be read
    assert not bool(torch.isnan(R.emulate(L)[..., 96:128]).any())


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("mistake,form", [("dropped_tap", "act"), ("wrong_slice", "act"), ("act_after_residual", "plus"),
                                          ("beta2_dropped", "rrdb"), ("rounded_before_residual", "body")])
def test_seeded_mistakes_leave_the_bound(sdt, mistake, form):
    L = _launch(sdt, form)
    if mistake == "rounded_before_residual":
        # an early rounding costs u |v| where the bound allows u |E|: visible where the residual cancels most of v and the
        # accumulation allowance (proportional to K and to sum |w x|) is small - few non-zero weights, short K, values off the lattice
        L = _launch(sdt, "body", Cin=32, lattice=True)
        L["x"] = (L["x"].float() * 1.37).to(sdt)
    worst, rest = R.verdict(L, R.emulate(L, mistake))
    print(f"[rrdb-ref] {mistake} on {form} {sdt}: worst err / bound {worst:.3g}, outside intact {rest}")
    assert worst > 1.0 or not rest
    if mistake == "wrong_slice":
        assert not rest


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("form", R.FORMS)
def test_lattice_is_exact(sdt, form):
    """fp32 emulation == one rounding of the float64 value, bit for bit: nothing in the lattice data depends on summation order"""
    for ups in (0, 1):
        L = _launch(sdt, form, ups=ups, lattice=True)
        v, _, _ = R.value64(L)
        s = slice(L["c0"], L["c0"] + L["live"])
        assert float(v.abs().max()) < 256
        assert torch.equal(R.bits(R.emulate(L)[..., s]), R.bits(R.lattice_expected(L)))
        if L["act"] and L["r1"] is None:                         # leaky relu alone: still ONE rounding of the float64 value
            assert torch.equal(R.bits(R.emulate(L)[..., s]), R.bits(v.to(sdt)))
            assert bool((v < 0).any()) and bool((v > 0).any())
        elif L["act"]:                                           # ... with a residual the fp32 chain defines the bits ...
            assert float((R.emulate(L)[..., s].double() - v).abs().max()) <= 2.0 ** -7 * float(v.abs().max())    # ... next to float64
            assert bool((v < 0).any()) and bool((v > 0).any())
        else:
            assert torch.equal(v, v.round())                     # integers: representable in both storage types
            assert torch.equal(R.bits(R.emulate(L)[..., s]), R.bits(v.to(sdt)))


def test_epilogue_and_unshuffle_helpers():
    g = torch.Generator().manual_seed(3)
    buf = torch.randn((2, 3, 5, 64), generator=g).to(torch.bfloat16)
    r1 = torch.randn((2, 3, 5, 32), generator=g).to(torch.bfloat16)
    out = R.epilogue_inplace(buf, 32, 32, None, 0.2, 1, r1, 1.0, None, 0.0)
    assert torch.equal(R.bits(out[..., :32]), R.bits(buf[..., :32]))
    want = torch.nn.functional.leaky_relu(0.2 * buf[..., 32:].double(), R.f32(0.2)) + r1.double()
    assert float((out[..., 32:].double() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()) + 1e-6
    x = torch.randn((2, 3, 8, 12), generator=g)
    for r in (1, 2, 4):
        y = R.unshuffle(x, r, torch.float16)
        assert y.shape == (2, 8 // r, 12 // r, 32 if r < 4 else 64)
        assert torch.equal(y[..., :3 * r * r].permute(0, 3, 1, 2).float(), torch.nn.functional.pixel_unshuffle(x, r).half().float() if r > 1 else x.half().float())
        assert bool((y[..., 3 * r * r:] == 0).all())


def _independent_net(sd, cfg, x):
    """the same graph built from nn.Modules with BasicSR's layout, loaded by name - a second formulation of R.net"""
    from torch import nn

    class RDB(nn.Module):
        def __init__(self, plus):
            super().__init__()
            for k in range(5):
                setattr(self, f"conv{k + 1}", nn.Conv2d(64 + 32 * k, 64 if k == 4 else 32, 3, 1, 1))
            if plus:
                self.conv1x1 = nn.Conv2d(64, 32, 1, bias=False)

        def forward(self, x):
            a = nn.functional.leaky_relu
            x1 = a(self.conv1(x), 0.2)
            x2 = a(self.conv2(torch.cat((x, x1), 1)), 0.2)
            if hasattr(self, "conv1x1"):
                x2 = x2 + self.conv1x1(x)
            x3 = a(self.conv3(torch.cat((x, x1, x2), 1)), 0.2)
            x4 = a(self.conv4(torch.cat((x, x1, x2, x3), 1)), 0.2)
            return self.conv5(torch.cat((x, x1, x2, x3, x4), 1)) * 0.2 + x

    class RRDB(nn.Module):
        def __init__(self, plus):
            super().__init__()
            self.rdb1, self.rdb2, self.rdb3 = RDB(plus), RDB(plus), RDB(plus)

        def forward(self, x):
            return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            r = {4: 1, 2: 2, 1: 4}[cfg["scale"]]
            self.r = r
            self.conv_first = nn.Conv2d(cfg["num_in_ch"] * r * r, 64, 3, 1, 1)
            self.body = nn.Sequential(*[RRDB(cfg.get("plus", False)) for _ in range(cfg["num_block"])])
            for n in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
                setattr(self, n, nn.Conv2d(64, 64, 3, 1, 1))
            self.conv_last = nn.Conv2d(64, cfg["num_out_ch"], 3, 1, 1)

        def forward(self, x):
            a, up = nn.functional.leaky_relu, lambda t: nn.functional.interpolate(t, scale_factor=2, mode="nearest")
            f = self.conv_first(nn.functional.pixel_unshuffle(x, self.r) if self.r > 1 else x)
            f = f + self.conv_body(self.body(f))
            f = a(self.conv_up1(up(f)), 0.2)
            f = a(self.conv_up2(up(f)), 0.2)
            return self.conv_last(a(self.conv_hr(f), 0.2))

    m = Net()
    m.load_state_dict(sd)
    with torch.no_grad():
        return m(x)


@pytest.mark.parametrize("kw", MODEL_CASES)
def test_net_matches_a_module_formulation(kw):
    cfg = gcfg.tiny_rrdb(**kw)
    sd = weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))
    x = torch.rand((2, 3, 24, 20), generator=torch.Generator().manual_seed(0))
    a, b = R.net(sd, cfg, x), _independent_net(sd, cfg, x)
    r = {4: 1, 2: 2, 1: 4}[cfg.scale]
    assert a.shape == (2, 3, 24 // r * 4, 20 // r * 4)
    assert R.rel_l2(a, b) < 1e-5


@pytest.mark.parametrize("kw", MODEL_CASES)
def test_storage_emulation_distance(kw):
    cfg = gcfg.tiny_rrdb(**kw)
    sd = weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))
    x = torch.rand((2, 3, 24, 20), generator=torch.Generator().manual_seed(0))
    ref = R.net(sd, cfg, x)
    for sdt in SDTS:
        d = R.rel_l2(R.net(sd, cfg, x, store=sdt), ref)
        print(f"[rrdb-ref] storage emulation {kw} {sdt}: rel-L2 against the fp32 net {d:.3e}")
        assert d < (2e-2 if sdt == torch.bfloat16 else 3e-3)          # a few units of 2^-8 / 2^-11: sanity only, the gates use the value


def test_gate_tables_equal_the_measured_emulation():
    """The GPU gates are twice the EMULATION tables of tests/test_gpu_rrdb_model.py and tests/test_gpu_upscaler.py: every entry must be
    the value this machine measures (within 1 %: ATen may sum a convolution in another order on another CPU), so a table cannot drift."""
    import test_gpu_rrdb_model as M
    import test_gpu_upscaler as P
    for name, kw in M.CASES.items():
        cfg, sd, x, ref = M._setup(name)
        for sdt in SDTS:
            d = R.rel_l2(R.net(sd, cfg, x, store=sdt), ref)
            assert abs(d - M.EMULATION[(name, sdt)]) <= 0.01 * d, (name, sdt, d, M.EMULATION[(name, sdt)])
    for sdt in SDTS:
        d = P._emulation_distance(sdt)
        assert abs(d - P.EMULATION[sdt]) <= 0.01 * d, (sdt, d, P.EMULATION[sdt])
