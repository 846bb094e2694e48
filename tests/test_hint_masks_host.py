"""Masked ControlNet hints, host side, against what the reference computed (tests/golden/hint_mask_vectors.npz, recorded by
tests/golden/make_hint_mask_golden.py from UnifiedPipelineHint_Controlnet over a fake control model): an explicit mask, the alpha
plane of an RGBA hint, an all-ones mask, soft_injection x cfg_only on the CFG sides g / u / f, 4- and 9-channel latents, extend, and a
mask of a size that cannot be resized.

The fake control model here has the surface of GyreHipControlNet and does what the device does: residual k leaves as
fl(fl(scale_k r_k) m_k) in float32, with m_k the mask bound for residual k and the latents multiplied by x_mask on the way in.  Its
unweighted residuals are the generator's ramps plus average pools of the bound image and of the latents it was given, so the recorded
residuals also pin those two.

Bound: the reference multiplies r by weight, by the layer weight and by the mask - three float32 roundings; the native path rounds the
scale once (weight x layer weight, formed in double), then the two device products - three as well.  Mask, image and latents are the
same float32 tensors on both sides (the same resize, the same products).  So |got - ref| <= (3 + 3) 2^-24 |ref|, plus 2^-149 for a
denormal step."""
import json
import os

import numpy as np
import pytest
import torch

from golden import make_hint_mask_golden as G
from gyre_amd import hints as HN
from gyre_amd.hints import ControlNetHint

GOLD = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hint_mask_vectors.npz")))
CASES = [tuple(c) for c in json.loads(str(GOLD["cases"]))]
WEIGHT = float(GOLD["weight"])
N = 13


class FakeNativeControlNet:
    SLOTS = 4
    config = type("Cfg", (dict,), {"n_residuals": N - 1})()

    def __init__(self):
        self._bound, self.binds = {}, 0

    def residual_shapes(self, H, W):
        assert (H, W) == (G.LAT, G.LAT)
        return [(1, h, w) for h, w in G.residual_hw(H, W)]

    def bind(self, image, ctx, *, slot=0, masks=None):
        assert masks is None or (len(masks) == N and all(m.dtype == torch.float32 for m in masks))
        self._bound[slot] = (image, ctx, masks)
        self.binds += 1

    def __call__(self, x, t, *, scales, out, accumulate=False, out_batch=None, out_offset=0, slot=0, x_mask=None):
        image, ctx, masks = self._bound[slot]
        assert ctx.shape[0] == x.shape[0] and x.shape[1] == 4 and not accumulate
        if x_mask is not None:
            assert x_mask.shape == (x.shape[0], 1, G.LAT, G.LAT)
            x = x * x_mask
        res = G.fake_residuals(image, x)
        for k, (o, r, s) in enumerate(zip(out, res, scales)):
            v = torch.tensor(s, dtype=torch.float32) * r
            if masks is not None:
                v = v * masks[k]
            o.zero_()
            o[out_offset:out_offset + x.shape[0]] = v
        return out


def native(name, kind, soft, cfg_only, side, channels):
    image, mask, latents, ctx = G.inputs(name, kind, side, channels)
    model = FakeNativeControlNet()
    hint = ControlNetHint(model, image, mask=mask, weight=WEIGHT, soft_injection=soft, cfg_only=cfg_only)
    out = [torch.full((latents.shape[0], 1, h, w), float("nan")) for h, w in G.residual_hw(G.LAT, G.LAT)]
    extra = latents[:G.B, 4:].clone() if channels == 9 else None           # what the leaf keeps for the whole request
    wrote = [hint.run(side, latents, torch.full((latents.shape[0],), 500), ctx, out, False, extra=extra) for _ in range(3)]
    return hint, model, out, wrote


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_masked_hint_matches_the_reference(case):
    name, kind, soft, cfg_only, side, channels = case
    hint, model, out, wrote = native(*case)
    assert (hint.mask is not None) == bool(GOLD[f"{name}.has_mask"])         # an all-ones mask is discarded, an alpha plane kept
    if f"{name}.zeros" in GOLD:                                             # cfg_only on the unconditional side: nothing runs
        assert wrote == [False] * 3 and model.binds == 0
        return
    assert wrote == [True] * 3 and model.binds == 1                         # three steps, one bind: nothing is rebuilt per step
    worst = 0.0
    for k, o in enumerate(out):
        ref = torch.from_numpy(GOLD[f"{name}.r{k}"])
        assert o.shape == ref.shape
        bound = 6 * 2.0 ** -24 * ref.double().abs() + 2.0 ** -149
        worst = max(worst, float(((o.double() - ref.double()).abs() / bound).max()))
    print(f"[hint masks] {name}: worst |got - ref| / bound {worst:.3f}")
    assert worst <= 1.0
    if kind in ("explicit", "rgba"):                                         # the mask bites: zero on the left, beyond the kernel's reach
        assert bool((out[0][..., : G.LAT // 2 - 3] == 0).all()) and float(out[0].abs().max()) > 0


def test_inpaint_state_is_keyed_on_the_extra_channels():
    name, kind, soft, cfg_only, side, channels = CASES[7]                   # explicit_soft_f9
    image, mask, latents, ctx = G.inputs(name, kind, side, channels)
    model = FakeNativeControlNet()
    hint = ControlNetHint(model, image, mask=mask, weight=WEIGHT, soft_injection=soft)
    out = [torch.zeros((latents.shape[0], 1, h, w)) for h, w in G.residual_hw(G.LAT, G.LAT)]
    extra, t = latents[:G.B, 4:].clone(), torch.full((latents.shape[0],), 500)
    hint.run(side, latents, t, ctx, out, False, extra=extra)
    kept = hint._inpaint[side]
    hint.run(side, latents, t, ctx, out, False, extra=extra)
    assert hint._inpaint[side] is kept and model.binds == 1
    hint.run(side, latents, t, ctx, out, False, extra=extra.clone())        # another request's tensor: made again, bound again
    assert hint._inpaint[side] is not kept and model.binds == 2
    with pytest.raises(ValueError, match="9-channel"):
        hint.run(side, latents, t, ctx, out, False)


def test_extend_and_the_mask_that_cannot_be_resized():
    image, mask, _, _ = G.inputs("explicit_g4", "explicit", "g", 4)
    hint = ControlNetHint(FakeNativeControlNet(), image, mask=mask, weight=WEIGHT, cfg_only=True)
    soft = hint.extend(lambda image, mask, **_: {"soft_injection": True})
    assert [soft.soft_injection, soft.cfg_only, soft.weight == WEIGHT, soft.mask is not None, soft is not hint] == GOLD["extend.soft"].tolist()
    half = hint.extend(lambda image, mask, **_: {"image": image[..., ::2, ::2], "mask": mask[..., ::2, ::2] if mask is not None else mask})
    assert [list(half.image.shape), list(half.mask.shape)] == GOLD["extend.half_shapes"].tolist()
    assert bool(GOLD["non_divisible_raises"])                               # the reference asserts; here it is a ValueError
    with pytest.raises(ValueError, match="whole multiple"):
        HN.resized_mask((5, 8), torch.ones(1, 1, 16, 16))
    bad = ControlNetHint(FakeNativeControlNet(), image, mask=torch.rand(1, 1, 250, 250), weight=WEIGHT)
    out = [torch.zeros((G.B, 1, h, w)) for h, w in G.residual_hw(G.LAT, G.LAT)]
    with pytest.raises(ValueError, match="whole multiple"):
        bad.run("g", torch.zeros(G.B, 4, G.LAT, G.LAT), 500, torch.zeros(G.B, 3, 8), out, False)
