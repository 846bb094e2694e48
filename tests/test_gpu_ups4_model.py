"""The four-parity upsampler form inside the model runtime (Exec::conv3, csrc/model_impl.h), on a small UNet (-m gpu).

Model: channels (64, 128), 16x16 latents, batch 3: one upsampler, 8x8 -> 16x16 over 128 channels (Mp = 192 source pixels per parity:
a ragged tile).  Its shape is far below the planner's tile-count rule, so tuning bit 30 of gyre_debug_gemm_ablation takes the form
(config 24 for that conv alone); bit 29 on top keeps nine taps: the same-handle A/B.

What one extra weight rounding does to THIS model, emulated on the oracle (tests/ups4_ref.py oracle_with_rounded_upsamplers: the
upsampler's weight rounded to storage, against the four-parity form on composed weights rounded once more; measured on the CPU).
The device keeps activations in 16 bits, so the emulation rounds the output of every convolution, linear layer and GroupNorm to the
storage type in both runs: a perturbation d that meets a rounding step of spacing u leaves it as 0 or u (rms ~ sqrt(d u) > d), which
an oracle with fp32 activations does not show (it gives 1.02e-3 / 1.28e-4, the size of the perturbation where it enters).
    bf16 storage   rel-L2 of eps = 5.18e-3        fp16 storage   rel-L2 of eps = 6.38e-4
The device's two paths may differ by twice that.  Measured on MI355X: 6.5e-3 (bf16), 8.2e-4 (fp16).
This assertion has little power on its own: 1.04e-2 (bf16) is not far below what two fully decorrelated 16-bit runs would show
(about 1.4e-2 from 9.65e-3 against the oracle each).  It catches a wrong tap or a wrong row, not a subtle one; the bit-exact lattice
and the element-wise bound of tests/test_gpu_ups4_conv.py are what pin the form.
"""
import ctypes as C

import pytest
import torch

import ups4_ref as U4
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV, HDT, randn, rel_l2, report, st
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
NO_UPS4, UPS4_ALL = 1 << 29, 1 << 30
NO_POUT_FOLD = 1 << 28             # proj_out stays its own launch
EMULATED = {torch.bfloat16: 5.18e-3, torch.float16: 6.38e-4}        # (docstring) - asserted against the oracle below


def small_cfg():
    return gcfg.UNetConfig(block_out_channels=(64, 128), attn_levels=(True, True), num_heads=(2, 4), transformer_depth=(1, 2),
                           cross_attention_dim=64, sample_size=16)


@pytest.fixture(scope="module")
def small():
    cfg = small_cfg()
    sd = weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 0)
    inp = (randn(3, 4, 16, 16, seed=61), torch.tensor([640, 640, 640]), randn(3, 77, cfg.cross_attention_dim, seed=62))
    return cfg, sd, inp, M.unet_forward(sd, cfg, *inp)


def make_net(cfg, sd):
    net = GyreHipUNet(cfg)
    net.load_state_dict(sd)
    return net.to(DEV)


def fwd(net, inp):
    x, t, ctx = inp
    return net(x.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV)).sample.clone()


class Bits:
    def __init__(self, L, bits):
        self.L, self.bits = L, bits

    def __enter__(self):
        self.old = self.L.gyre_debug_gemm_ablation(self.bits)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.L.gyre_debug_gemm_ablation(self.old)
        return False


def test_the_form_is_taken_for_the_small_model_under_bit_30():
    L = _lib.lib()
    q = (C.c_int32 * 4)()
    for bits, want in ((0, 0), (UPS4_ALL, 1), (UPS4_ALL | NO_UPS4, 0)):
        old = L.gyre_debug_gemm_ablation(bits)
        try:
            _lib.check(L.gyre_debug_ups4_plan(3, 8, 8, 128, 128, 0, 0, 0, 2, q))
        finally:
            L.gyre_debug_gemm_ablation(old)
        assert q[0] == want, (bits, tuple(q))


def test_emulated_extra_rounding_is_the_stated_figure(small):
    cfg, sd, inp, _ = small
    a = U4.oracle_with_rounded_upsamplers(M, sd, cfg, inp, HDT, composed=False, store=True)
    b = U4.oracle_with_rounded_upsamplers(M, sd, cfg, inp, HDT, composed=True, store=True)
    e = rel_l2(b, a)
    print(f"[ups4 model] emulated extra weight rounding on the oracle ({HDT}): rel-L2 {e:.3e}, stated {EMULATED[HDT]:.3e}")
    assert 0.9 * EMULATED[HDT] <= e <= 1.1 * EMULATED[HDT]


def test_parity_form_against_the_oracle_and_against_nine_taps(small):
    cfg, sd, inp, ref = small
    net = make_net(cfg, sd)
    L = net._L()
    outs, launches = {}, {}
    for bits in (UPS4_ALL | NO_UPS4, UPS4_ALL):
        with Bits(L, bits):
            fwd(net, inp)                                   # first call: the per-handle weight copies (composed weights included)
            outs[bits] = fwd(net, inp).float().cpu()
            launches[bits] = L.gyre_last_launch_count()
            assert torch.equal(outs[bits], fwd(net, inp).float().cpu())            # deterministic
    nine, four = outs[UPS4_ALL | NO_UPS4], outs[UPS4_ALL]
    assert not torch.equal(nine, four), "bit 30 did not change a bit: the four-parity form did not run"
    assert launches[UPS4_ALL] == launches[UPS4_ALL | NO_UPS4], launches          # one launch either way, the compose kernel ran in the warm-up
    report("small UNet, upsampler in the four-parity form", four, ref, 3e-2)
    report("small UNet, upsampler on nine taps", nine, ref, 3e-2)
    d = rel_l2(four, nine)
    print(f"[ups4 model] four-parity vs nine taps on the same handle: rel-L2 {d:.3e} (emulated extra rounding {EMULATED[HDT]:.3e}, "
          f"allowed {2 * EMULATED[HDT]:.3e}); vs oracle: four {rel_l2(four, ref):.3e} nine {rel_l2(nine, ref):.3e}")
    assert d <= 2 * EMULATED[HDT], (d, EMULATED[HDT])


def test_activation_keeping_pass_and_vjp(small):
    cfg, sd, inp, ref = small
    net = make_net(cfg, sd)
    L = net._L()
    x, t, ctx = inp
    cot = randn(3, cfg.out_channels, 16, 16, seed=63)
    xr = x.clone().requires_grad_()
    (gref,) = torch.autograd.grad(M.unet_forward(sd, cfg, xr, t, ctx), xr, cot)
    # The activation-keeping pass never folds proj_out into FF2 (it keeps the FF2 output for the reverse sweep); at this model's sizes
    # the inference call does (C x HW >= 8192, tests/test_gpu_proj_out_fold.py), which alone changes bits.  Bit 28 takes that
    # difference out of both calls, so that what is compared is the upsampler: bit 30 set in both.
    with Bits(L, UPS4_ALL | NO_POUT_FOLD):
        with torch.no_grad():
            plain = fwd(net, inp)
        xd = x.to(DEV).requires_grad_()
        eps = net(xd, t.to(DEV), encoder_hidden_states=ctx.to(DEV)).sample
        (got,) = torch.autograd.grad(eps, xd, cot.to(DEV))
        torch.cuda.synchronize()
    assert torch.equal(plain, eps.detach()), "the activation-keeping pass and the inference call differ"
    with Bits(L, UPS4_ALL | NO_UPS4 | NO_POUT_FOLD):
        with torch.no_grad():
            nine = fwd(net, inp)
    assert not torch.equal(nine, plain), "the four-parity form did not run"
    report("small UNet eps (kept pass, four-parity upsampler)", eps.detach().float().cpu(), ref, 3e-2)
    report("small UNet vjp d_x with the four-parity upsampler in the forward", got.float().cpu(), gref, 5e-2)


def test_composed_weights_follow_a_weight_update(small):
    cfg, sd, inp, _ = small
    net = make_net(cfg, sd)
    L = net._L()
    key = "up_blocks.0.upsamplers.0.conv.weight"
    with Bits(L, UPS4_ALL):
        base = fwd(net, inp)                                # the composed weights exist from here on
        cur = {k: v.clone() for k, v in sd.items()}
        cur[key] = (sd[key].float() * -0.75 + randn(*sd[key].shape, seed=81) * 0.02).to(sd[key].dtype)
        t = cur[key].to(DEV).contiguous()
        shape = (C.c_int64 * t.ndim)(*t.shape)
        _lib.check(L.gyre_unet_set_weight(C.c_void_p(net._handle), key.encode(), C.c_void_p(t.data_ptr()), _lib.dtype_code(t), shape, t.ndim,
                                          st()), L)
        _lib.check(L.gyre_unet_finalize(C.c_void_p(net._handle), st()), L)
        torch.cuda.synchronize()
        net._ctx_slots = []
        got = fwd(net, inp)
        twin = make_net(cfg, cur)
        fresh = fwd(twin, inp)
    assert not torch.equal(got, base), "the update did not change the output"
    assert torch.equal(got, fresh), "stale composed weights after gyre_unet_set_weight"
