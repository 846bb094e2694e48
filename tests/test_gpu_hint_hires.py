"""ControlNet hints under hires fix, with an alpha mask and next to a grafted 9-channel inpaint pair, end to end on the native models
(-m gpu): GyrePipeline over the tiny UNet, the tiny VAE and the tiny ControlNet, 3 steps of a k-sampler with CFG.

  (a) a 96 x 96 request on a UNet whose natural size is 64 px (tiny_unet at sample_size 8) runs: hires fix is engaged, the natural leaf
      binds image_to_natural of the hint, the full leaf the hint with soft injection.  Before there were bind slots this raised.
  (b) the result is bit-identical to the same request with the slots switched off (hints.REBIND_EVERY_CALL: every call binds slot 0
      again).  Equal-shaped calls are bit-deterministic here, so any difference is a slot bug.
  (c) an RGBA hint whose alpha is zero on the left half: the ControlNet residual buffers of the full-size leaf are exactly zero
      wherever the resized mask is zero, which is a strip on the left of every residual that is wide enough.
  (d) a grafted 9-channel pair with a ControlNet hint runs, and what the control model is given there is latents x mask channel.

(c) and (d) run at a natural size of 256 px (sample_size 32; (c) at 384 x 384): the reference's mask resize is a lanczos3 with
antialiasing over reflect padding, whose reach of 3 x the reduction factor must stay inside the mask, so the smallest residual of a
masked hint - 1/64 of the hint image - needs at least 4 pixels, in the reference as here."""
import dataclasses

import pytest
import torch

from gyre_amd import config as gcfg, hints as HN, schedulers as S, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.hints import ControlNetHint
from gyre_amd.modules import GyreHipUNet, GyreHipVAE
from gyre_amd.pipeline import GyrePipeline, mask_to_latent_mask, round_mask
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def native(cls, cfg, shapes, seed):
    m = cls(cfg)
    m.load_state_dict(weights.synthetic_state_dict(shapes(cfg), seed))
    return m.to(DEV)


@pytest.fixture(scope="module")
def rig():
    vae = native(GyreHipVAE, gcfg.tiny_vae(), weights.vae_param_shapes, 2)
    ctrl = native(GyreHipControlNet, gcfg.tiny_controlnet(), weights.controlnet_param_shapes, 1)
    unets = {}

    def unet(in_channels, sample_size):
        key = (in_channels, sample_size)
        if key not in unets:
            cfg = dataclasses.replace(gcfg.tiny_unet(in_channels), sample_size=sample_size)
            unets[key] = native(GyreHipUNet, cfg, weights.unet_param_shapes, in_channels)
        return unets[key]

    g = torch.Generator().manual_seed(5)
    text = torch.randn(2, 77, 64, generator=g).to(DEV)
    unc = torch.randn(1, 77, 64, generator=g).expand(2, -1, -1).contiguous().to(DEV)
    kw = dict(seeds=[11, 12], text_embeddings=text, uncond_embeddings=unc, num_inference_steps=3, sampler="euler", output_type="latent")
    return dict(vae=vae, ctrl=ctrl, unet=unet, kw=kw)


def image(c, n, seed):
    return torch.rand(1, c, n, n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_hires_request_with_a_controlnet_hint_runs_and_slots_change_nothing(rig):
    pipe = GyrePipeline(rig["unet"](4, 8), rig["vae"], device=DEV)
    img = image(3, 96, 1)
    run = lambda **kw: pipe(height=96, width=96, **{**rig["kw"], **kw})
    got = run(controlnet_hints=[ControlNetHint(rig["ctrl"], img, weight=0.8)])                       # (a)
    assert got.shape == (2, 4, 12, 12) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, run())                                                               # the hint matters
    assert torch.equal(got, run(controlnet_hints=[ControlNetHint(rig["ctrl"], img, weight=0.8)]))    # and the run is deterministic
    HN.REBIND_EVERY_CALL = True
    try:
        rebound = run(controlnet_hints=[ControlNetHint(rig["ctrl"], img, weight=0.8)])               # (b)
    finally:
        HN.REBIND_EVERY_CALL = False
    assert torch.equal(got, rebound)
    seq = run(controlnet_hints=[ControlNetHint(rig["ctrl"], img, weight=0.8)], cfg_execution="sequential")      # four slots
    HN.REBIND_EVERY_CALL = True
    try:
        assert torch.equal(seq, run(controlnet_hints=[ControlNetHint(rig["ctrl"], img, weight=0.8)], cfg_execution="sequential"))
    finally:
        HN.REBIND_EVERY_CALL = False


def test_alpha_mask_zeroes_the_residuals_of_the_full_leaf(rig, monkeypatch):
    pipe = GyrePipeline(rig["unet"](4, 32), rig["vae"], device=DEV)
    rgba = image(4, 384, 2)
    rgba[:, 3, :, :192] = 0.0                                                                        # alpha: zero on the left half
    rgba[:, 3, :, 192:] = 1.0
    seen = []
    inner = S.UNetWithControlnet.__call__

    def spy(self, latents, t, **kw):
        out = inner(self, latents, t, **kw)
        if latents.shape[-1] == 48:                                                                  # the full-size leaf
            seen.append([b.clone() for b in self._bufs[1]])
        return out

    monkeypatch.setattr(S.UNetWithControlnet, "__call__", spy)
    hint = ControlNetHint(rig["ctrl"], rgba, weight=0.8)
    assert hint.image.shape[1] == 3 and hint.mask is not None
    got = pipe(height=384, width=384, controlnet_hints=[hint], **rig["kw"])
    assert bool(torch.isfinite(got).all()) and len(seen) == 3
    shapes = rig["ctrl"].residual_shapes(48, 48)
    pyramid = [HN.resized_mask((rh, rw), rgba[:, [3]]) for _, rh, rw in shapes]
    checked = 0
    for bufs in seen:
        assert len(bufs) == 13 and bufs[0].shape[0] == 4                                             # the CFG pair of two images
        for b, m, (_, rh, rw) in zip(bufs, pyramid, shapes):
            zero = (m == 0).expand_as(b)
            strip = rw // 2 - 3                                                                      # columns the kernel's reach keeps clear
            if strip > 0:
                assert bool((m[..., :strip] == 0).all())
                checked += 1
            assert bool((b[zero] == 0).all()) and float(b[~zero].abs().max()) > 0
    assert checked == 3 * 9                                                                          # every residual but the four 6 x 6 ones


def test_grafted_nine_channel_pair_feeds_the_control_model_masked_latents(rig, monkeypatch):
    ctrl = rig["ctrl"]
    pipe = GyrePipeline(rig["unet"](4, 32), rig["vae"], device=DEV, inpaint_unet=rig["unet"](9, 32), grafted_inpaint=True)
    img, init = image(3, 256, 3), image(3, 256, 4)
    mask = torch.zeros(1, 1, 256, 256, device=DEV)
    mask[:, :, 64:192, :128] = 1.0                                                                   # 1 = repaint
    calls = []
    inner = GyreHipControlNet.forward

    def spy(self, latents, t, **kw):
        calls.append((latents.clone(), t, dict(kw)))
        return inner(self, latents, t, **kw)

    monkeypatch.setattr(GyreHipControlNet, "forward", spy)
    got = pipe(height=256, width=256, controlnet_hints=[ControlNetHint(ctrl, img, weight=0.8)], image=init, mask_image=mask, strength=1.0,
               **{**rig["kw"], "num_inference_steps": 10})
    monkeypatch.setattr(GyreHipControlNet, "forward", inner)
    assert got.shape == (2, 4, 32, 32) and bool(torch.isfinite(got).all())
    nine = [c for c in calls if c[2].get("x_mask") is not None]
    four = [c for c in calls if c[2].get("x_mask") is None]
    assert nine and four and len({c[2].get("slot", 0) for c in calls}) == 2                          # both leaves ran, each on its slot
    keep = mask_to_latent_mask(GyrePipeline.preprocess_mask(mask))
    want = (1 - round_mask(keep, 0.001)[:, [0]]).expand(4, -1, -1, -1)                               # the mask channel, over the CFG pair
    x, t, kw = nine[0]
    assert x.shape[1] == 4 and torch.equal(kw["x_mask"], want) and 0 < float(want.mean()) < 1
    # the same step again, on the slot the request left bound: with the mask, and with the latents multiplied on the host
    scales, slot = kw["scales"], kw.get("slot", 0)
    with_mask = [o.clone() for o in ctrl(x, t, scales=scales, slot=slot, x_mask=kw["x_mask"])]
    pre = [o.clone() for o in ctrl((x * want).contiguous(), t, scales=scales, slot=slot)]
    assert all(torch.equal(a, b) for a, b in zip(with_mask, pre))
    assert not all(torch.equal(a, b) for a, b in zip(with_mask, ctrl(x, t, scales=scales, slot=slot)))


def test_engine_serves_an_inpaint_request_with_a_controlnet_hint(rig):
    """the engine class, the public interface: hint_images routed to the control model together with mask_image, on the 9-channel inpaint
    UNet alone and on the grafted pair - both were NotImplementedError"""
    from types import SimpleNamespace
    from gyre_amd.engine import GyreUnifiedPipeline
    from test_gpu_engine import generators, tokenizer, wrapper_kwargs
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(0)
    te = CLIPTextModel(CLIPTextConfig(vocab_size=49408, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      max_position_embeddings=77, bos_token_id=49406, eos_token_id=49407, pad_token_id=49407)).eval().to(DEV)
    table = {"canny": {"canny": rig["ctrl"]}}
    manager = SimpleNamespace(for_type=lambda t, default=None: table.get(t, default))
    eng = GyreUnifiedPipeline(vae=rig["vae"], text_encoder=te, tokenizer=tokenizer, unet=rig["unet"](4, 32), inpaint_unet=rig["unet"](9, 32),
                              hintset_manager=manager)
    eng.scheduler = "euler"
    init, mask = image(3, 256, 4).cpu(), torch.zeros(1, 1, 256, 256)
    mask[:, :, 64:192, :128] = 1.0
    hint = SimpleNamespace(image=image(3, 256, 3).cpu(), hint_type="canny", weight=0.8, priority="prompt", clip_layer=None)

    def call(hints):
        args = wrapper_kwargs(prompt=["a lighthouse", "a cat"], negative_prompt=None, generator=generators([7, 8]), width=256, height=256,
                              num_inference_steps=4, image=init, mask_image=mask, strength=1.0, hint_images=hints)
        images, nsfw = eng(**args)
        assert images.shape == (2, 3, 256, 256) and bool(torch.isfinite(images).all())
        return images

    plain, hinted = call([]), call([hint])
    assert not torch.equal(plain, hinted) and torch.equal(hinted, call([hint]))
    eng._grafted_inpaint = True
    grafted = call([hint])
    assert not torch.equal(grafted, call([]))
