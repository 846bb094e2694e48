"""Build-container script: EXECUTES the reference's masked ControlNet-hint code and records what it computed in hint_mask_vectors.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hint_mask_golden.py

  * unified_pipeline.py ``UnifiedPipelineHint_Controlnet`` - its constructor (an explicit mask, the alpha plane of an RGBA image, an
    all-ones mask that is discarded), ``__call__`` on the CFG sides g / u / f with soft_injection x cfg_only over 4- and 9-channel
    latents, and ``extend`` - over a fake control model whose residuals are known ramps plus average pools of what it was given
    (the conditioning image and the latents), so that the recorded residuals also pin those two inputs.

``gyre.images.resize`` is routed to ``gyre_amd.images.resize`` (as tests/test_reference_upscaler.py routes the blur): ResizeRight is
not installed where this runs.  That leaves ResizeRight itself unpinned here, as it already is - gyre_amd/resize.py restates it and
is held against recorded vectors of its own.  Everything else - which mask goes where, in which order the factors are multiplied -
is the reference's own arithmetic.

The file holds seeds, case descriptions and the weighted residuals only; inputs are regenerated from the seeds
(tests/test_hint_masks_host.py).  Third-party packages the reference imports but this path never runs are stubbed
(make_golden._install).  Nothing here ships."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

B, LAT = 2, 32                      # images per request; latents 32 x 32 (hint image 256 x 256): the smallest residual is 4 x 4
WEIGHT = 0.7
# (name, mask kind, soft_injection, cfg_only, CFG side, latent channels)
CASES = [
    ("explicit_g4", "explicit", False, False, "g", 4),
    ("explicit_soft_f4", "explicit", True, False, "f", 4),
    ("explicit_soft_cfgonly_f4", "explicit", True, True, "f", 4),
    ("explicit_cfgonly_u4", "explicit", False, True, "u", 4),
    ("rgba_soft_g4", "rgba", True, False, "g", 4),
    ("ones_f4", "ones", False, False, "f", 4),
    ("none_g9", "none", False, False, "g", 9),
    ("explicit_soft_f9", "explicit", True, False, "f", 9),
    ("rgba_cfgonly_g9", "rgba", False, True, "g", 9),
    ("explicit_soft_cfgonly_u9", "explicit", True, True, "u", 9),
    ("ones_soft_u9", "ones", True, False, "u", 9),
]


def residual_hw(h, w, n_levels=4, layers=2):
    out = [(h, w)]
    for i in range(n_levels):
        out += [(h, w)] * layers
        if i < n_levels - 1:
            h, w = (h + 1) // 2, (w + 1) // 2
            out.append((h, w))
    return out + [(h, w)]


def ramps(batch):
    """residual k of sample b before the pools: a ramp over the pixels, offset by k and b"""
    out = []
    for k, (h, w) in enumerate(residual_hw(LAT, LAT)):
        r = torch.linspace(-1.0, 1.0, h * w, dtype=torch.float32).reshape(1, 1, h, w) * (1 + 0.25 * k)
        out.append(torch.cat([r + 0.125 * (k + 1) + 0.5 * b for b in range(batch)]))
    return out


def fake_residuals(cond, latents):
    """the ramps plus average pools of the conditioning image and of the latents, at every residual's size"""
    batch = latents.shape[0]
    c, x = cond.mean(1, keepdim=True), latents.mean(1, keepdim=True)
    if c.shape[0] != batch:
        c = c.expand(batch, -1, -1, -1)
    return [r + F.adaptive_avg_pool2d(c, r.shape[-2:]) + F.adaptive_avg_pool2d(x, r.shape[-2:]) for r in ramps(batch)]


def inputs(name, kind, side, channels):
    """(image [1, 3 or 4, 256, 256], explicit mask or None, latents [B or 2B, channels, 32, 32], context) from the case's seed"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    image = torch.rand(1, 3, 8 * LAT, 8 * LAT, generator=g)
    soft_edge = torch.rand(1, 1, 8 * LAT, 8 * LAT, generator=g)
    soft_edge[:, :, :, : 4 * LAT] = 0.0                                   # zero on the left half, noise on the right
    mask = None
    if kind == "explicit":
        mask = soft_edge
    elif kind == "rgba":
        image = torch.cat([image, soft_edge], dim=1)
    elif kind == "ones":
        mask = torch.ones(1, 1, 8 * LAT, 8 * LAT)
    batch = 2 * B if side == "f" else B
    latents = torch.randn(batch, 4, LAT, LAT, generator=g)
    if channels == 9:
        hole = (torch.rand(B, 1, LAT, LAT, generator=g) > 0.5).float()   # the inpaint UNet's mask channel
        extra = torch.cat([hole, torch.randn(B, 4, LAT, LAT, generator=g)], dim=1)
        latents = torch.cat([latents, extra.repeat(batch // B, 1, 1, 1)], dim=1)
    ctx = torch.randn(batch, 3, 8, generator=g)
    return image, mask, latents, ctx


def main():
    import make_golden as mg
    mg._install()
    from types import SimpleNamespace
    from gyre.pipeline import unified_pipeline as UP
    from gyre_amd import images as native_images
    UP.images.resize = native_images.resize

    class FakeControlNet:
        config = {}

        def __call__(self, latents, t, encoder_hidden_states=None, controlnet_cond=None, **_):
            res = fake_residuals(controlnet_cond, latents)
            return SimpleNamespace(down_block_res_samples=res[:-1], mid_block_res_sample=res[-1])

    out = {"cases": np.array(json.dumps(CASES)), "weight": np.array(WEIGHT)}
    for name, kind, soft, cfg_only, side, channels in CASES:
        image, mask, latents, ctx = inputs(name, kind, side, channels)
        hint = UP.UnifiedPipelineHint_Controlnet(FakeControlNet(), image, mask, WEIGHT, soft, cfg_only, B)
        out[f"{name}.has_mask"] = np.array(hint.mask is not None)
        t = torch.full((latents.shape[0],), 500)
        with torch.no_grad():
            res = hint(latents, t, ctx, side)
        down, mid = res.down_block_res_samples, res.mid_block_res_sample
        if side == "u" and cfg_only:                                       # "Just return zeros": nothing is recorded
            assert all(float(d) == 0 for d in down) and float(mid) == 0
            out[f"{name}.zeros"] = np.array(True)
            continue
        for k, r in enumerate(list(down) + [mid]):
            out[f"{name}.r{k}"] = r.numpy()
    # extend: the callbacks of the hires-fix tree (unified_pipeline.py:2148-2168) on a masked hint
    image, mask, _, _ = inputs("explicit_g4", "explicit", "g", 4)
    hint = UP.UnifiedPipelineHint_Controlnet(FakeControlNet(), image, mask, WEIGHT, False, True, B)
    soft = hint.extend(lambda image, mask, **_: {"soft_injection": True})
    half = hint.extend(lambda image, mask, **_: {"image": image[..., ::2, ::2], "mask": mask[..., ::2, ::2] if mask is not None else mask})
    out["extend.soft"] = np.array([soft.soft_injection, soft.cfg_only, soft.weight == WEIGHT, soft.mask is not None, soft is not hint])
    out["extend.half_shapes"] = np.array([list(half.image.shape), list(half.mask.shape)])
    # a mask whose size is no whole multiple / divisor of the state's: the reference's asserts
    try:
        hint.resized_mask(torch.zeros(1, 1, 5, 8), torch.ones(1, 1, 16, 16))
        raised = False
    except AssertionError:
        raised = True
    out["non_divisible_raises"] = np.array(raised)
    path = os.path.join(HERE, "hint_mask_vectors.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
