"""Self-test of the MLSD references (tests/mlsd_ref.py), on the host: the restated net equals the stored outputs of the reference's own
module; the seeded weights put 1 % to 50 % of all ReLU6 outputs at 6 on every case (a ReLU in place of ReLU6 must not pass); the
storage-emulation distance of the whole net - the numbers the GPU model gate is twice of - is measured per (case, flavour), printed
and re-checked; every seeded mistake lands outside twice that distance on every case, in max-abs AND in rel-L2; the fp32 emulations of
the kernels meet their derived element bounds and the kernel-level mistakes break them."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlsd_ref as R

SDTS = [torch.bfloat16, torch.float16]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlsd_vectors.npz")
# (max-abs, rel-L2) of net(store=dt, compute=fp64) against the fp64 net on MODEL_CASES, as printed by test_storage_emulation_distance:
# the table tests/test_gpu_mlsd_model.py imports.  The assertion keeps it honest (a changed net or recipe must re-measure).  Each entry is
# the WORST of DRAWS input draws (mlsd_ref.model_input(name, seed=0 .. DRAWS - 1)); the GPU tests run draw 0.  One draw is too few at
# 16x16: its output has 576 values and whether the largest error lands near a half step is luck.
DRAWS = 4
EMULATION = {
    ("16x16", torch.bfloat16): (3.344e-03, 6.970e-03),
    ("16x16", torch.float16): (4.274e-04, 8.236e-04),
    ("17x49", torch.bfloat16): (6.369e-03, 7.491e-03),
    ("17x49", torch.float16): (6.331e-04, 9.326e-04),
    ("64x32", torch.bfloat16): (1.006e-02, 8.417e-03),
    ("64x32", torch.float16): (1.049e-03, 9.744e-04),
    ("96x160", torch.bfloat16): (1.511e-02, 9.434e-03),
    ("96x160", torch.float16): (2.066e-03, 1.283e-03),
}


def test_net_equals_the_stored_reference_outputs():
    stored = np.load(GOLDEN)
    sd = R.model_weights()
    from gyre_amd import weights
    assert stored["keys"].tolist() == list(weights.mlsd_param_shapes()) == list(sd) and len(sd) == 362
    for name in ("16x16", "17x49"):
        x = torch.from_numpy(stored["x_" + name])
        assert torch.equal(x, R.model_input(name))                   # the recipe still draws the stored input
        got, want = R.net(sd, x), torch.from_numpy(stored["y_" + name])
        print(f"[mlsd] stored reference output {name}: largest difference {R.max_abs(got, want):.3e}")
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_relu6_saturates_on_every_case(name):
    sd, x = R.model_case(name)
    st = {}
    out = R.net(sd, x, compute=torch.float64, stats=st)
    share = st["relu6_at_6"] / st["relu6_total"]
    print(f"[mlsd] {name}: {share:.3%} of {st['relu6_total']} ReLU6 outputs sit at 6; output rms {float(out.pow(2).mean().sqrt()):.3f}")
    assert 0.01 <= share <= 0.5
    assert torch.equal(out, R.model_ref64(name))


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_storage_emulation_distance(name):
    sd = R.model_weights()
    for dt in SDTS:
        ma = rl = 0.0
        for s in range(DRAWS):
            x = R.model_input(name, seed=s)
            ref, emu = R.net(sd, x, compute=torch.float64), R.net(sd, x, store=dt, compute=torch.float64)
            ma, rl = max(ma, R.max_abs(emu, ref)), max(rl, R.rel_l2(emu, ref))
        print(f'    ("{name}", torch.{str(dt).split(".")[1]}): ({ma:.3e}, {rl:.3e}),')
        want = EMULATION[(name, dt)]
        assert abs(ma - want[0]) <= 2e-3 * want[0] + 1e-9 and abs(rl - want[1]) <= 2e-3 * want[1] + 1e-9, (name, dt, ma, rl)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_seeded_mistake_lands_outside_the_gate_on_every_case(mistake):
    sd = R.model_weights()
    for name in R.MODEL_CASES:
        x, ref = R.model_input(name), R.model_ref64(name)
        for dt in SDTS:
            bad = R.net(sd, x, store=dt, compute=torch.float64, mistake=mistake)
            ma, rl = EMULATION[(name, dt)]
            assert bad.shape == ref.shape
            ra, rr = R.max_abs(bad, ref) / (2 * ma), R.rel_l2(bad, ref) / (2 * rl)
            print(f"[mlsd] {mistake} {name} {dt}: {ra:.1f} x the max-abs gate, {rr:.1f} x the rel-L2 gate")
            assert ra > 1 and rr > 1, (mistake, name, dt)


@pytest.mark.parametrize("sdt", SDTS)
def test_kernel_references_hold_their_fp32_emulation_and_see_the_kernel_mistakes(sdt):
    # depthwise: fp32 ATen on the storage operands meets the bound; symmetric padding at stride 2 and a missing input ReLU6 break it
    for (B, H, W, C), stride, rin in (((2, 3, 5, 32), 2, True), ((1, 4, 4, 32), 1, False), ((1, 2, 2, 32), 2, True)):
        x, w, b = R.dw_case(sdt, B, H, W, C)
        ref, t = R.dw_ref(x, w, b, stride, rin)
        xc = x.float().permute(0, 3, 1, 2)
        xc = F.relu6(xc) if rin else xc
        emu = F.conv2d(F.pad(xc, (0, 1, 0, 1)), w.float(), b, stride=2, groups=C) if stride == 2 else F.conv2d(xc, w.float(), b, padding=1, groups=C)
        emu = F.relu6(emu).permute(0, 2, 3, 1).to(sdt)
        assert R.verdict(emu, ref, R.stored_bound(ref, t, sdt)) <= 1.0
        if stride == 2:
            bad = F.relu6(F.conv2d(xc, w.float(), b, stride=2, padding=1, groups=C))[:, :, :H // 2, :W // 2].permute(0, 2, 3, 1).to(sdt)
            assert R.verdict(bad, ref, R.stored_bound(ref, t, sdt)) > 1.0
        if rin:
            assert R.verdict(R.dw_ref(x, w, b, stride, False)[0].to(sdt), ref, R.stored_bound(ref, t, sdt)) > 1.0
    # upsample: fp32 ATen meets the bound at the test sizes; align_corners=False breaks it
    for B, H, W in ((1, 1, 1), (2, 3, 5)):
        x = R.up2_case(sdt, B, H, W)
        ref, t = R.up2_ref(x, True)
        emu = R.upsample2_ac(F.relu(x.float().permute(0, 3, 1, 2))).permute(0, 2, 3, 1).to(sdt)
        assert ref.shape == (B, 2 * H, 2 * W, 64) and R.verdict(emu, ref, R.stored_bound(ref, t, sdt)) <= 1.0
        if H > 1:
            assert R.verdict(R.up2_ref(x, True, align_corners=False)[0].to(sdt), ref, R.stored_bound(ref, t, sdt)) > 1.0
    # dilated convolution: dilation 1 breaks it; on 4x4 only the centre tap is inside the image
    for B, H, W in ((1, 4, 4), (2, 11, 13)):
        x, w, b = R.dconv_case(sdt, B, H, W)
        ref, t = R.dconv_ref(x, w, b)
        emu = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, padding=5, dilation=5)).permute(0, 2, 3, 1).to(sdt)
        assert R.verdict(emu, ref, R.stored_bound(ref, t, sdt)) <= 1.0
        assert R.verdict(R.dconv_ref(x, w, b, dilation=1)[0].to(sdt), ref, R.stored_bound(ref, t, sdt)) > 1.0
        if H == 4:
            centre = F.relu(torch.einsum("bhwc,oc->bhwo", x.double(), w.double()[:, :, 1, 1]) + b.double())
            assert torch.allclose(centre, ref, rtol=0, atol=1e-12)
    # entry: symmetric padding breaks it
    for H, W in ((16, 16), (17, 49)):
        x, w, b = R.entry_case(sdt, torch.float32, 2, H, W)
        ref, t = R.entry_ref(x, w, b)
        emu = F.relu6(F.conv2d(F.pad(x, (0, 1, 0, 1)), w.float(), b, stride=2)).permute(0, 2, 3, 1).to(sdt)
        assert ref.shape == (2, H // 2, W // 2, 32) and R.verdict(emu, ref, R.stored_bound(ref, t, sdt)) <= 1.0
        bad = F.relu6(F.conv2d(x, w.float(), b, stride=2, padding=1))[:, :, :H // 2, :W // 2].permute(0, 2, 3, 1).to(sdt)
        assert R.verdict(bad, ref, R.stored_bound(ref, t, sdt)) > 1.0
