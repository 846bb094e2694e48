"""The native ControlNet (-m gpu; model_ctrl.hip behind gyre_amd.controlnet.GyreHipControlNet) against the fp32 restatement
tests/ctrl_ref.py, in bfloat16 and float16, and chained into the native UNet.

Gates: rel-L2 per residual <= 3e-2 (bf16) and <= 5e-3 (fp16) - those of tests/test_gpu_models.py and tests/test_gpu_f16_flavour.py
for the tiny UNet, whose encoder half this model is."""
import functools

import pytest
import torch

import ctrl_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
GATE = {torch.bfloat16: 3e-2, torch.float16: 5e-3}
DTYPES = [torch.bfloat16, torch.float16]


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@functools.lru_cache(maxsize=None)
def state(name, seed):
    cfg = gcfg.tiny_controlnet() if name == "tiny" else gcfg.sd15_controlnet()
    return cfg, weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), seed)


@functools.lru_cache(maxsize=None)
def model(name, dtype, seed=1):
    cfg, sd = state(name, seed)
    net = GyreHipControlNet(cfg)
    net.load_state_dict(sd)
    return net.to(dtype).to(DEV), {k: v.to(dtype).float() for k, v in sd.items()}


def inputs(cfg, B, h, w, S, dtype, seed=0, image_batch=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).to(dtype)
    ctx = torch.randn(B, S, cfg.cross_attention_dim, generator=g).to(dtype)
    img = torch.rand(image_batch or B, 3, 8 * h, 8 * w, generator=g).to(dtype)
    return x, ctx, img


def check(label, got, ref, dtype):
    errs = [rel_l2(g, r) for g, r in zip(got, ref)]
    print(f"[ctrl] {label} {dtype}: rel-L2 per residual " + " ".join(f"{e:.1e}" for e in errs))
    assert len(got) == len(ref) and [tuple(g.shape) for g in got] == [tuple(r.shape) for r in ref]
    assert all(float(g.float().norm()) > 0 for g in got)
    assert max(errs) <= GATE[dtype], (label, dtype, errs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 16, 24, 77, [981, 17]), (3, 16, 16, 5, 500)])
def test_tiny_controlnet_matches_the_restatement(dtype, case):
    B, h, w, S, t = case
    net, sd = model("tiny", dtype)
    cfg = net.config
    x, ctx, img = inputs(cfg, B, h, w, S, dtype, seed=B)
    tt = torch.tensor(t) if isinstance(t, list) else torch.tensor(t)
    ref = R.ctrl_forward(sd, cfg, x.float(), tt, ctx.float(), img.float())
    net.bind(img.to(DEV), ctx.to(DEV))
    got = [o.clone() for o in net(x.to(DEV), tt if isinstance(t, list) else t)]
    assert len(got) == 13 and all(o.dtype == dtype for o in got)
    check(f"tiny B={B} {h}x{w} S={S}", got, ref, dtype)
    again = net(x.to(DEV), tt if isinstance(t, list) else t)
    assert all(torch.equal(a, b) for a, b in zip(got, again))          # two calls are bit-equal


@pytest.mark.parametrize("dtype", DTYPES)
def test_sd15_widths_match_the_restatement(dtype):
    """latents 8 x 8 is the smallest size that still reaches every level: the 96-wide stride-2 convolution, the 768-wide context and
    the planner's real tiles"""
    net, sd = model("sd15", dtype)
    cfg = net.config
    x, ctx, img = inputs(cfg, 2, 8, 8, 77, dtype, seed=9)
    t = torch.tensor([700, 30])
    ref = R.ctrl_forward(sd, cfg, x.float(), t, ctx.float(), img.float())
    net.bind(img.to(DEV), ctx.to(DEV))
    check("sd15 B=2 8x8 S=77", net(x.to(DEV), t), ref, dtype)


def test_bind_semantics():
    dtype = torch.bfloat16
    net, sd = model("tiny", dtype)
    cfg = net.config
    x, ctx, img = inputs(cfg, 2, 16, 16, 7, dtype, seed=3, image_batch=1)
    fresh = GyreHipControlNet(cfg)
    fresh.load_state_dict(state("tiny", 1)[1])
    fresh = fresh.to(dtype).to(DEV)
    with pytest.raises(ValueError):
        fresh(x.to(DEV), 10)                                           # forward before bind
    net.bind(img.to(DEV), ctx.to(DEV))
    one = [o.clone() for o in net(x.to(DEV), 400)]
    net.bind(img.expand(2, -1, -1, -1).contiguous().to(DEV), ctx.to(DEV))
    rep = [o.clone() for o in net(x.to(DEV), 400)]
    assert all(torch.equal(a, b) for a, b in zip(one, rep))            # a batch-1 image = the image repeated, bit for bit
    for t in (400, 23):                                                # one bind, two steps
        ref = R.ctrl_forward(sd, cfg, x.float(), torch.tensor(t), ctx.float(), img.float())
        check(f"one bind, t={t}", net(x.to(DEV), t), ref, dtype)
    other = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(77)).to(dtype)
    net.bind(other.to(DEV), ctx.to(DEV))
    moved = net(x.to(DEV), 400)
    assert all(not torch.equal(a, b) for a, b in zip(one, moved))      # another image, other residuals
    with pytest.raises(ValueError):
        net(torch.randn(2, 4, 16, 24).to(dtype).to(DEV), 400)          # latents that do not match the bound image
    with pytest.raises(ValueError):
        net(torch.randn(3, 4, 16, 16).to(dtype).to(DEV), 400)          # nor the bound batch


def test_placement_and_sum_of_two_models():
    dtype = torch.bfloat16
    a, sda = model("tiny", dtype, 1)
    b, sdb = model("tiny", dtype, 2)
    cfg = a.config
    B = 2
    x, ctx, img = inputs(cfg, B, 16, 16, 9, dtype, seed=5)
    a.bind(img.to(DEV), ctx.to(DEV))
    b.bind(img.to(DEV), ctx.to(DEV))
    plain = [o.clone() for o in a(x.to(DEV), 321)]
    bufs = a.new_outputs(2 * B, 16, 16, DEV)
    for o in bufs:
        o.fill_(float("nan"))
    a(x.to(DEV), 321, out=bufs, out_batch=2 * B, out_offset=B)
    assert all(bool((o[:B] == 0).all()) and torch.equal(o[B:], p) for o, p in zip(bufs, plain))
    sa, sb = R.hint_scales(0.8, True, 13), R.hint_scales(1.3, False, 13)
    outs = a.new_outputs(B, 16, 16, DEV)
    a(x.to(DEV), 321, scales=sa, out=outs)
    b(x.to(DEV), 321, scales=sb, out=outs, accumulate=True)
    t = torch.tensor(321)
    ra = R.ctrl_forward(sda, cfg, x.float(), t, ctx.float(), img.float())
    rb = R.ctrl_forward(sdb, cfg, x.float(), t, ctx.float(), img.float())
    check("sum of two models", outs, [p * u + q * v for p, u, q, v in zip(ra, sa, rb, sb)], dtype)


def test_controlnet_into_unet_chain():
    dtype = torch.bfloat16
    net, sd = model("tiny", dtype)
    cfg = net.config
    ucfg = gcfg.tiny_unet()
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg))
    unet = GyreHipUNet(ucfg)
    unet.load_state_dict(usd)
    unet = unet.to(dtype).to(DEV)
    usd_r = {k: v.to(dtype).float() for k, v in usd.items()}
    x, ctx, img = inputs(cfg, 2, 16, 16, 77, dtype, seed=11)
    t = torch.tensor([600, 40])
    res = R.ctrl_forward(sd, cfg, x.float(), t, ctx.float(), img.float())
    ref = M.unet_forward(usd_r, ucfg, x.float(), t, ctx.float(), down_res=res[:-1], mid_res=res[-1])
    ref_plain = M.unet_forward(usd_r, ucfg, x.float(), t, ctx.float())
    net.bind(img.to(DEV), ctx.to(DEV))
    got_res = net(x.to(DEV), t)
    cd = ctx.to(DEV)
    got = unet(x.to(DEV), t.to(DEV), encoder_hidden_states=cd, down_block_additional_residuals=got_res[:-1],
               mid_block_additional_residual=got_res[-1]).sample
    plain = unet(x.to(DEV), t.to(DEV), encoder_hidden_states=cd).sample
    e, moved = rel_l2(got, ref), rel_l2(plain, ref)
    print(f"[ctrl] controlnet -> unet chain: rel-L2 {e:.2e} vs oracle; {moved:.2e} without the residuals; oracle's own {rel_l2(ref_plain, ref):.2e}")
    assert e <= 3e-2
    assert moved > 0.05                                                # the residuals matter
