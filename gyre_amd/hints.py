"""Host side of hint-image conditioning with T2I adapters.

  T2IHint              UnifiedPipelineHint_T2i, standard path       unified_pipeline.py:746-786, 906-919
  combine_t2i_states   UNetWithT2I.__init__, standard branch        unet/core.py:128-206 (with AdapterStateList, :67-93)

The adapter itself runs natively (gyre_amd/t2i.py); what is here is the per-level weighting of its states and the sums the CFG
wrappers receive.  Style adapters, co-adapters with their fuser, and masked hints (the mask resize is an unpinned lanczos3) raise
NotImplementedError.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor


def normalise_tensor(t: Tensor, channels: int) -> Tensor:
    """reference images.normalise_tensor for 1 and 3 channels: batch axis added, grey replicated / colour cut to the count."""
    if t.ndim == 3:
        t = t[None]
    if channels == 1:
        return t[:, [0]]
    if channels == 3:
        return t[:, [0, 1, 2]] if t.shape[1] >= 3 else t[:, [0, 0, 0]]
    raise ValueError(f"Unknown number of channels {channels}")


class T2IHint:
    """One hint image bound to its adapter.  Calling it runs the adapter and returns the weighted per-level states."""

    def __init__(self, model, image: Tensor, mask: Optional[Tensor] = None, weight: float = 1.0, soft_injection: bool = False,
                 cfg_only: bool = False):
        if getattr(model, "_coadapter_type", False):
            raise NotImplementedError("T2I co-adapters (fuser) are outside the native path")
        if image.ndim == 3:
            image = image[None]
        if mask is None and image.shape[1] == 4:
            mask = image[:, [3]]
        if mask is not None:
            mask = normalise_tensor(mask, 1)
            if mask.mean() == 1.0 and mask.std() == 0.0:      # pure ones: the reference discards it
                mask = None
        if mask is not None:
            raise NotImplementedError("masked T2I hints (the reference resizes the mask with an unpinned lanczos3)")
        channels = model.config.cin // 64 if "cin" in model.config else 3
        self.model, self.image = model, normalise_tensor(normalise_tensor(image, 3), channels)
        self.weight, self.soft_injection, self.cfg_only = weight, soft_injection, cfg_only

    def layer_weights(self):
        if not self.soft_injection:
            return (1.0, 1.0, 1.0, 1.0)
        lw = torch.logspace(-0.25, 0, 4)
        if self.cfg_only:
            lw[0] = 0.25
        return lw

    def coadapter_type(self):
        return False

    def to(self, device=None, dtype=None):
        self.image = self.image.to(device, dtype)
        return self

    def __call__(self) -> List[Tensor]:
        states = self.model(self.image)
        return [s * self.weight * lw for s, lw in zip(states, self.layer_weights())]      # (lw: a float or a 0-dim host tensor)


def combine_t2i_states(hints: Sequence) -> Optional[Dict[str, List[Tensor]]]:
    """{"g": sum over all hints, "u": the same with cfg_only hints replaced by zeros, "f": cat[u, g] along the batch} per level -
    what the conditional side, the unconditional side and the CFG-parallel call receive.  None without hints."""
    if not hints:
        return None
    gs, us = [], []
    for hint in hints:
        if hint.coadapter_type():
            raise NotImplementedError("T2I co-adapters (fuser) are outside the native path")
        state = hint()
        if not isinstance(state, list):
            raise NotImplementedError("T2I style adapter states")
        gs.append(state)
        us.append([torch.zeros_like(s) for s in state] if hint.cfg_only else state)
    out = {"u": [sum(i) for i in zip(*us)], "g": [sum(i) for i in zip(*gs)]}
    out["f"] = [torch.cat([u, g], dim=0) for u, g in zip(out["u"], out["g"])]
    return out
