"""ControlNet hints in a mode tree (hires fix, grafted inpaint), host side: GyrePipeline on the CPU over stub UNet and ControlNet shells
that record what every leaf binds and calls - which hint image and mask each leaf's copy of a hint carries, which scales, which bind
slot of the control model, and how often a bind happens over a multi-step run (reference unified_pipeline.py:1080-1097, 2071-2181).
The tiny UNet config is taken at a natural size of 64 px (sample_size 8), so a 96 x 96 request is above the hires threshold.  Where a
mask is resized the natural size is 256 px (sample_size 32) and the request 384 x 384: the reference's mask resize is a lanczos3 with
antialiasing over REFLECT padding, whose reach (3 x the reduction factor on each side) must stay inside the mask, so the smallest
residual of a masked hint (1/64 of the hint image) needs at least 4 pixels - in the reference as here."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

import ctrl_ref as R
from gyre_amd import config as gcfg, hints as HN, hires as H, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.hints import ControlNetHint
from gyre_amd.pipeline import GyrePipeline


class StubControlNet:
    """the surface ControlNetHint uses of GyreHipControlNet, slots and masks included; residual k of a call is the constant k + 1"""
    SLOTS = GyreHipControlNet.SLOTS

    def __init__(self):
        self.config = gcfg.tiny_controlnet()
        self._bound, self.binds, self.calls = {}, [], []

    residual_shapes = GyreHipControlNet.residual_shapes

    def bind(self, image, ctx, *, slot=0, masks=None):
        self._bound[slot] = (image, ctx)
        self.binds.append(SimpleNamespace(slot=slot, image=image.clone(), ctx=ctx, masks=None if masks is None else [m.clone() for m in masks]))

    def new_outputs(self, B, H_, W_, device, dtype=None):
        return [torch.zeros((B, ch, h, w)) for ch, h, w in self.residual_shapes(H_, W_)]

    def __call__(self, x, t, *, scales, out, accumulate=False, out_batch=None, out_offset=0, slot=0, x_mask=None):
        image, _ = self._bound[slot]
        assert tuple(image.shape[-2:]) == (8 * x.shape[-2], 8 * x.shape[-1])          # the slot's own geometry
        self.calls.append(SimpleNamespace(slot=slot, x=x.clone(), scales=list(scales), x_mask=x_mask, accumulate=accumulate))
        for k, (o, s) in enumerate(zip(out, scales)):
            if not accumulate:
                o.zero_()
            o[out_offset:out_offset + x.shape[0]] += (k + 1) * s
        return out


class StubUNet:
    def __init__(self, in_channels=4, sample_size=8):
        self.config = dataclasses.replace(gcfg.tiny_unet(in_channels), sample_size=sample_size)
        self.calls = []

    def __call__(self, latents, t, **kw):
        self.calls.append(SimpleNamespace(shape=tuple(latents.shape), kw=kw))
        return SimpleNamespace(sample=torch.zeros_like(latents[:, :4]))


TEXT = torch.zeros(2, 5, 64)
KW = dict(seeds=[1, 2], text_embeddings=TEXT, uncond_embeddings=TEXT + 1, num_inference_steps=4, sampler="euler", output_type="latent")


def _vae():
    from test_host_pipeline import OracleVAE
    vcfg = gcfg.tiny_vae()
    return OracleVAE(weights.synthetic_state_dict(weights.vae_param_shapes(vcfg)), vcfg)


def _image(c, n, seed=0):
    return torch.rand(1, c, n, n, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("cfg_execution", ["parallel", "sequential"])
def test_hires_gives_each_leaf_its_own_hint_and_slot(cfg_execution):
    ctrl = StubControlNet()
    image, mask = _image(3, 384), (_image(1, 384, 1) > 0.5).float()
    hint = ControlNetHint(ctrl, image, mask=mask, weight=0.8)
    pipe = GyrePipeline(StubUNet(sample_size=32), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu")
    out = pipe(height=384, width=384, controlnet_hints=[hint], cfg_execution=cfg_execution, **KW)
    assert out.shape == (2, 4, 48, 48)
    sides = 2 if cfg_execution == "sequential" else 1
    # one bind per (hint, side, leaf) over the four steps, every one on a slot of its own
    assert len(ctrl.binds) == 2 * sides and sorted(b.slot for b in ctrl.binds) == list(range(2 * sides))
    nat = [b for b in ctrl.binds if b.image.shape[-1] == 256]
    full = [b for b in ctrl.binds if b.image.shape[-1] == 384]
    assert len(nat) == sides and len(full) == sides
    oos = pipe.hires_oos_fraction
    for b in nat:                                              # the natural leaf: image_to_natural of the image and of the mask
        assert torch.equal(b.image, H.image_to_natural(256, image, oos))
        want = [HN.resized_mask((rh, rw), H.image_to_natural(256, mask, oos)) for _, rh, rw in ctrl.residual_shapes(32, 32)]
        assert len(b.masks) == 13 and all(torch.equal(p, q) for p, q in zip(b.masks, want))
    for b in full:                                             # the full-size leaf: the image and the mask as they came
        assert torch.equal(b.image, image) and torch.equal(b.masks[0], HN.resized_mask((48, 48), mask))
    by_slot = {b.slot: b for b in ctrl.binds}
    soft, plain = R.hint_scales(0.8, True, 13), R.hint_scales(0.8, False, 13)
    assert soft != plain
    seen = set()
    for c in ctrl.calls:
        is_full = by_slot[c.slot].image.shape[-1] == 384
        assert c.x.shape[-1] == (48 if is_full else 32)
        assert c.scales == (soft if is_full else plain)        # hint.extend(soft_injection=True) on the full-size leaf only
        assert c.x_mask is None
        seen.add(c.slot)
    assert seen == set(by_slot) and len(ctrl.calls) > len(ctrl.binds)
    assert hint.soft_injection is False and hint._slots == {}  # the request's own hint object is left as it was


def test_rebind_switch_binds_slot_zero_on_every_call():
    ctrl = StubControlNet()
    hint = ControlNetHint(ctrl, _image(3, 96), weight=0.8)
    pipe = GyrePipeline(StubUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu")
    HN.REBIND_EVERY_CALL = True
    try:
        pipe(height=96, width=96, controlnet_hints=[hint], **KW)
    finally:
        HN.REBIND_EVERY_CALL = False
    assert len(ctrl.binds) == len(ctrl.calls) > 4 and {b.slot for b in ctrl.binds} == {0} and {c.slot for c in ctrl.calls} == {0}


def test_single_leaf_request_keeps_the_old_calls():
    """no tree: the request's own hint object on slot 0, bound once, through bind(image, ctx) / model(...) without the new arguments"""
    ctrl = StubControlNet()
    hint = ControlNetHint(ctrl, _image(3, 64), weight=0.8)
    pipe = GyrePipeline(StubUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu")
    pipe(height=64, width=64, controlnet_hints=[hint], **KW)
    assert len(ctrl.binds) == 1 and ctrl.binds[0].slot == 0 and ctrl.binds[0].masks is None and len(ctrl.calls) == 4
    assert hint._slots == {}


def test_grafted_inpaint_pair_both_leaves_see_the_hint():
    ctrl = StubControlNet()
    image = _image(3, 256)
    hint = ControlNetHint(ctrl, image, weight=0.8)
    u4, u9 = StubUNet(sample_size=32), StubUNet(9, sample_size=32)
    pipe = GyrePipeline(u4, _vae(), device="cpu", inpaint_unet=u9, grafted_inpaint=True)
    init = _image(3, 256, 3)
    mask = torch.zeros(1, 1, 256, 256)
    mask[:, :, :, :128] = 1.0                                   # repaint the left half
    pipe(height=256, width=256, controlnet_hints=[hint], image=init, mask_image=mask, strength=1.0, **{**KW, "num_inference_steps": 10})
    assert u4.calls and u9.calls and all(c.shape[1] == 9 for c in u9.calls)
    assert len(ctrl.binds) == 2 and sorted(b.slot for b in ctrl.binds) == [0, 1]
    nine = [b for b in ctrl.binds if b.masks is not None]
    four = [b for b in ctrl.binds if b.masks is None]
    assert len(nine) == 1 and len(four) == 1 and torch.equal(four[0].image, image)
    calls9 = [c for c in ctrl.calls if c.slot == nine[0].slot]
    calls4 = [c for c in ctrl.calls if c.slot == four[0].slot]
    assert calls9 and calls4 and all(c.x_mask is None for c in calls4)
    # the 9-channel leaf: x_mask is the mask channel of its extra channels (repeated over the CFG pair), the bound image the hint
    # image times that mask at image resolution, the residual masks that mask at every residual's resolution
    kw9 = u9.calls[0].kw
    assert "down_block_additional_residuals" in kw9 and "down_block_additional_residuals" in u4.calls[0].kw
    m = calls9[0].x_mask
    assert m is not None and m.shape == (4, 1, 32, 32) and all(c.x_mask is m for c in calls9)          # computed once, not per step
    assert set(m.unique().tolist()) <= {0.0, 1.0} and bool((m[:, :, :, :16] == 1).all()) and bool((m[:, :, :, 16:] == 0).all())
    big = HN.resized_mask((256, 256), m)
    assert torch.equal(nine[0].image, image * big)
    assert all(torch.equal(p, HN.resized_mask((rh, rw), big)) for p, (_, rh, rw) in zip(nine[0].masks, ctrl.residual_shapes(32, 32)))
    assert all(c.x.shape[1] == 4 for c in ctrl.calls)


def test_a_fifth_slot_raises():
    ctrl = StubControlNet()
    hints = [ControlNetHint(ctrl, _image(3, 96, s)) for s in range(3)]                 # 2 leaves x 3 hints on one model
    pipe = GyrePipeline(StubUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu")
    with pytest.raises(NotImplementedError, match="GYRE_CTRL_SLOTS = 4"):
        pipe(height=96, width=96, controlnet_hints=hints, **KW)
    assert not ctrl.binds
    other = StubControlNet()                                                           # two models: two slots each
    pipe(height=96, width=96, controlnet_hints=[ControlNetHint(ctrl, _image(3, 96)), ControlNetHint(other, _image(3, 96))], **KW)
    assert sorted(b.slot for b in ctrl.binds) == [0, 1] and sorted(b.slot for b in other.binds) == [0, 1]


def test_extend_is_the_references():
    ctrl = StubControlNet()
    hint = ControlNetHint(ctrl, _image(4, 16), weight=0.7, cfg_only=True)              # the alpha plane is the mask
    twin = hint.extend()
    assert twin is not hint and twin._token is not hint._token and twin.model is ctrl
    assert torch.equal(twin.image, hint.image) and torch.equal(twin.mask, hint.mask) and (twin.weight, twin.cfg_only) == (0.7, True)
    soft = hint.extend(soft_injection=True)
    assert soft.soft_injection and not hint.soft_injection
    seen = {}
    half = hint.extend(lambda image, mask, **rest: seen.update(rest) or {"image": image * 0.5, "mask": None}, weight=0.3)
    assert set(seen) == {"model", "weight", "soft_injection", "cfg_only"} and seen["weight"] == 0.3
    assert torch.equal(half.image, hint.image * 0.5) and half.mask is None and half.weight == 0.3
    pooled = ControlNetHint(SimpleNamespace(config=gcfg.tiny_controlnet(global_pool_conditions=True)), _image(3, 16))
    assert pooled.extend(soft_injection=True).soft_injection is False                  # the constructor's own rules apply again
    with pytest.raises(ValueError, match="whole multiple"):
        HN.resized_mask((5, 8), torch.ones(1, 1, 16, 16))


def test_extend_on_the_t2i_hint_classes():
    """extend on T2IHint, CoAdapterHint and StyleHint: the stored constructor arguments round-trip, an image already cut to the adapter's
    cin // 64 channels included, and the copy is a new object of the same class"""
    sketch = SimpleNamespace(config=gcfg.T2IConfig(cin=64), _coadapter_type=False)
    h = HN.T2IHint(sketch, _image(3, 16), weight=0.6, cfg_only=True)
    assert h.image.shape == (1, 1, 16, 16)
    e = h.extend(soft_injection=True)
    assert type(e) is HN.T2IHint and e is not h and e.model is sketch and torch.equal(e.image, h.image)     # one channel stays one channel
    assert (e.weight, e.soft_injection, e.cfg_only, e.mask) == (0.6, True, True, None) and not h.soft_injection
    half = h.extend(lambda image, **_: {"image": image[..., ::2, ::2]})
    assert half.image.shape == (1, 1, 8, 8)
    co = SimpleNamespace(config={}, _coadapter_type="sketch")
    fuser = object()
    c = HN.CoAdapterHint(co, _image(3, 16), fuser, weight=0.4)
    ce = c.extend(weight=0.9)
    assert type(ce) is HN.CoAdapterHint and ce.fuser is fuser and ce.weight == 0.9 and ce.coadapter_type() == "sketch"
    fe = SimpleNamespace(image_mean=[0.5] * 3, image_std=[0.5] * 3, size={"shortest_edge": 32})
    clip = object()
    s = HN.StyleHint(SimpleNamespace(_coadapter_type=False), _image(3, 16), clip, fe, weight=0.3, cfg_only=True, clip_layer="penultimate")
    se = s.extend(weight=0.5)
    assert type(se) is HN.StyleHint and se.clip_model is clip and se.feature_extractor is fe and se.clip_layer == "penultimate"
    assert (se.weight, se.cfg_only, se.soft_injection) == (0.5, True, False) and torch.equal(se.image, s.image)


def test_a_mask_too_small_for_the_resize_says_so():
    with pytest.raises(ValueError, match="at least 4"):
        HN.resized_mask((1, 1), torch.ones(1, 1, 64, 64))
    assert HN.resized_mask((4, 4), torch.ones(1, 1, 256, 256)).shape == (1, 1, 4, 4)
    hint = ControlNetHint(StubControlNet(), _image(4, 64))                     # a 64 px RGBA hint: its smallest residual is 1 x 1
    with pytest.raises(ValueError, match="at least 256 pixels"):
        hint.run("g", torch.zeros(2, 4, 8, 8), 5, torch.zeros(2, 5, 64), None, False)
