"""Post-decode image helpers (host/device PyTorch): the outmask composite of the reference's pipeline tail.

reference: gyre/pipeline/unified_pipeline.py:2493-2510 (composite), gyre/images.py:667-672 + :49-82 (8-bit round
trip), gyre/match_histograms.py:12-36,84-92 (per-channel CDF matching, statistics taken over the whole batch - this
step couples the images of a batch in the reference, too).
"""
from __future__ import annotations

import numpy as np
import torch

Tensor = torch.Tensor


def _lut_from_counts(src_counts: np.ndarray, tmpl_counts: np.ndarray) -> np.ndarray:
    """256-entry map value -> matched value for one channel (unsigned-integer branch of _match_cumulative_cdf)."""
    tmpl_values = np.nonzero(tmpl_counts)[0]
    tmpl_nz = tmpl_counts[tmpl_values]
    src_q = np.cumsum(src_counts) / src_counts.sum()
    tmpl_q = np.cumsum(tmpl_nz) / tmpl_counts.sum()
    return np.interp(src_q, tmpl_q, tmpl_values)


def match_histograms_u8(image: Tensor, reference: Tensor) -> Tensor:
    """image, reference: uint8 [B,H,W,C] on any device -> uint8 matched image (float results truncated, as numpy's
    assignment into the uint8 output array does).  Only the 256-bin counts and the LUT cross the PCIe bus."""
    if image.ndim != reference.ndim:
        raise ValueError("Image and reference must have the same number of channels.")
    if image.shape[-1] != reference.shape[-1]:
        raise ValueError("Number of channels in the input image and reference image must match!")
    out = torch.empty_like(image)
    for c in range(image.shape[-1]):
        src = image[..., c].reshape(-1).to(torch.int64)
        sc = torch.bincount(src, minlength=256).cpu().numpy()
        tc = torch.bincount(reference[..., c].reshape(-1).to(torch.int64), minlength=256).cpu().numpy()
        lut = torch.from_numpy(_lut_from_counts(sc, tc).astype(np.uint8)).to(image.device)
        out[..., c] = lut[src].reshape(image.shape[:-1])
    return out


def match_histograms(image: Tensor, reference: Tensor) -> Tensor:
    """float BCHW in [0,1] -> float BCHW, through the same 8-bit quantisation the reference applies (toCV / fromCV;
    the channel reordering there is its own inverse and the matching is per channel, so it is skipped)."""
    to_u8 = lambda t: (t.to(torch.float32) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    m = match_histograms_u8(to_u8(image), to_u8(reference))
    return (m.permute(0, 3, 1, 2).to(torch.float32) / 255.0).to(image)


def outmask_composite(result: Tensor, source: Tensor, outmask: Tensor) -> Tensor:
    """result [B,3,H,W] in [0,1]; source / outmask [1 or B, >=3, H, W].  The generated pixels are tone-matched to the
    source-with-result composite, then pasted over the source where outmask is 1."""
    B = result.shape[0]
    rep = lambda t: (torch.cat([t] * B) if t.shape[0] == 1 else t)[:, [0, 1, 2]].to(result)
    outmask, source = rep(outmask), rep(source)
    reference = source * (1 - outmask) + result * outmask
    matched = match_histograms(result, reference)
    return source * (1 - outmask) + matched * outmask


# ---- the helpers of the upscaler path (reference gyre/images.py:290-408) -----------------------------------------------------------
def gaussianblur(tensor: Tensor, sigma) -> Tensor:
    """Separable Gaussian with a kernel of ceil(6 sigma) made odd and reflect padding (gyre/images.py:290-295; resize.gaussian_blur)."""
    from .resize import gaussian_blur
    return gaussian_blur(tensor, sigma)


def scale_shape(shape, scale: float):
    """`shape` with its two spatial (last) entries multiplied by `scale` and rounded to the nearest integer"""
    *lead, h, w = shape
    return (*lead, round(h * scale), round(w * scale))


def _per_axis(value):
    """a number, or a sequence of one or two numbers -> (vertical, horizontal)"""
    seq = tuple(value) if isinstance(value, (tuple, list)) else (value,)
    if len(seq) not in (1, 2):
        raise ValueError(f"expected one factor or a (vertical, horizontal) pair, got {value!r}")
    return seq[0], seq[-1]


def resize(tensor: Tensor, factors, sharpness: int = 1) -> Tensor:
    """Resample the two spatial axes by `factors` with lanczos3 over reflect padding, clamped to [0, 1]: with the kernel stretched
    against aliasing for sharpness 1, unstretched for 2 - what the reference's ``images.resize`` asks ResizeRight for.  Its
    sharpness 0 (area downscaling through kornia) is not built."""
    from .resize import resize_right
    if sharpness <= 0:
        raise NotImplementedError("images.resize: sharpness 0 (area downscaling) is outside the native path")
    return resize_right(tensor, scale_factors=_per_axis(factors), interp_method="lanczos3", antialiasing=sharpness == 1,
                        pad_mode="reflect").clamp(0, 1)


def _fit_axis(have: int, want: int):
    """How a side of `have` pixels is brought to `want`: (first pixel kept, padding in front, padding behind).  The difference is
    halved rounding DOWN, so an odd surplus is cut one pixel deeper in front and an odd shortfall padded one pixel more behind.
    As in the reference, a shortfall of exactly one pixel halves to nothing and is left as it is."""
    half = (want - have) // 2
    if half < 0:
        return -half, 0, 0
    if half > 0:
        return 0, half, want - have - half
    return 0, 0, 0


def rescale(tensor: Tensor, height: int, width=None, fit: str = "cover", pad_mode: str = "constant", sharpness: int = 1) -> Tensor:
    """Bring an image to height x width (square when width is None).  fit "cover": one factor for both axes, the larger of the two
    ratios, and the overhang cut off around the centre; "contain": the smaller ratio, and the gap padded (pad_mode) around the centre;
    anything else ("strict"): each axis by its own ratio.  Resampling: resize()."""
    target = (height, height if width is None else width)
    ratios = [want / have for want, have in zip(target, tensor.shape[-2:])]
    if fit == "cover":
        ratios = [max(ratios)] * 2
    elif fit == "contain":
        ratios = [min(ratios)] * 2
    out = resize(tensor, ratios, sharpness=sharpness)
    (top, above, below), (left, before, after) = (_fit_axis(have, want) for have, want in zip(out.shape[-2:], target))
    out = out[..., top:top + target[0], left:left + target[1]]
    return torch.nn.functional.pad(out, [before, after, above, below], pad_mode)


def from_pil(image) -> Tensor:
    """A PIL image -> float [1, C, H, W] in [0, 1] (8-bit channels divided by 255; a greyscale image gets one channel)"""
    arr = torch.from_numpy(np.array(image, copy=True))
    if arr.ndim == 2:
        arr = arr[..., None]
    return (arr.to(torch.float32) / 255.0).permute(2, 0, 1)[None].contiguous()
