"""Host side of hint-image conditioning with T2I adapters and ControlNets.

  T2IHint              UnifiedPipelineHint_T2i, standard path       unified_pipeline.py:746-786, 906-919
  combine_t2i_states   UNetWithT2I.__init__, standard branch        unet/core.py:128-206 (with AdapterStateList, :67-93)
  ControlNetHint       UnifiedPipelineHint_Controlnet               unified_pipeline.py:957-1058 (run per step by
                                                                    schedulers.UNetWithControlnet, unet/core.py:40-64)

The adapter itself runs natively (gyre_amd/t2i.py); what is here is the per-level weighting of its states and the sums the CFG
wrappers receive.  T2IHint and combine_t2i_states refuse style adapters and co-adapters; those enter through StyleHint, CoAdapterHint
and build_t2i_conditioning at the end of this file (gyre_amd/pipeline.py calls them once per request, engine._hints builds them).  Masked hints
(the mask resize is an unpinned lanczos3) raise NotImplementedError.  The ControlNet itself runs natively too (gyre_amd/controlnet.py): its hint only decides the per-residual scales,
which half of a CFG call the model sees and where in the shared residual buffers its outputs land; masked ControlNet hints raise for
the same reason.
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
        self._bind(model, image, mask, weight, soft_injection, cfg_only)

    def _bind(self, model, image, mask, weight, soft_injection, cfg_only):
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


class ControlNetHint:
    """One hint image bound to its ControlNet.  ``run`` is called once per UNet evaluation by schedulers.UNetWithControlnet with the
    CFG side of the calling stack: "g" (guided), "u" (unconditional) or "f" (one call over cat[unconditional, guided])."""

    def __init__(self, model, image: Tensor, mask: Optional[Tensor] = None, weight: float = 1.0, soft_injection: bool = False,
                 cfg_only: bool = False):
        if image.ndim == 3:
            image = image[None]
        if model.config.get("global_pool_conditions", False):
            cfg_only, soft_injection, mask = True, False, None        # (the reference ignores a mask here; the alpha plane below too)
            image = image[:, :3] if image.shape[1] == 4 else image
        if mask is None and image.shape[1] == 4:
            mask = image[:, [3]]
        if mask is not None:
            mask = normalise_tensor(mask, 1)
            if mask.mean() == 1.0 and mask.std() == 0.0:              # pure ones: the reference discards it
                mask = None
        if mask is not None:
            raise NotImplementedError("masked ControlNet hints (the reference resizes the mask with an unpinned lanczos3)")
        self.model, self.image = model, normalise_tensor(image, model.config.get("conditioning_channels", 3))
        self.weight, self.soft_injection, self.cfg_only = weight, soft_injection, cfg_only
        self._token = object()                                        # who bound the model last: (token, side)
        self._ctx = {}                                                # side -> (the stack's context, the context the model sees)

    def scales(self):
        """weight x logspace(-1, 0, N + 1)[k] for down residual k and the last point for the mid residual; the weight alone without
        soft injection (N + 1 = 13 for SD)."""
        n = self.model.config.n_residuals + 1
        if not self.soft_injection:
            return [float(self.weight)] * n
        return [float(self.weight) * float(lw) for lw in torch.logspace(-1, 0, n)]

    def to(self, device=None, dtype=None):
        self.image = self.image.to(device, dtype)
        return self

    def _bind(self, side, ctx):
        """The embedding of the image and the projected context live in the model, one request at a time: bind again only when
        another hint, another side (sequential CFG alternates two contexts on one model) or another request used it last."""
        kept = self._ctx.get(side)
        if kept is None or kept[0] is not ctx:
            seen = ctx.chunk(2)[-1].contiguous() if (self.cfg_only and side == "f") else ctx
            kept = self._ctx[side] = (ctx, seen)
        owner = getattr(self.model, "_bind_owner", None)
        if owner is None or owner[0] is not self._token or owner[1] != side or owner[2] is not kept[1] or self.model._bound is None:
            self.model.bind(self.image, kept[1])
            self.model._bind_owner = (self._token, side, kept[1])

    def run(self, side: str, latents: Tensor, t, encoder_hidden_states: Tensor, out, accumulate: bool):
        """Adds (accumulate) or assigns this hint's residuals for one UNet call into ``out`` (N + 1 NCHW buffers at the batch of
        ``latents``).  False when the hint contributes nothing on this side (cfg_only on "u")."""
        if latents.shape[1] == 9:
            raise NotImplementedError("ControlNet hints with a 9-channel inpaint UNet (the reference resizes its mask with an unpinned lanczos)")
        x, B = latents[:, 0:4], latents.shape[0]
        if self.cfg_only and side == "u":
            return False
        self._bind(side, encoder_hidden_states)
        if self.cfg_only and side == "f":                             # the guided half only, into the upper half; the lower half is zero
            x = x.chunk(2)[-1]
            t = t.chunk(2)[-1] if isinstance(t, torch.Tensor) and t.ndim > 0 and t.numel() > 1 else t
            self.model(x, t, scales=self.scales(), out=out, accumulate=accumulate, out_batch=B, out_offset=B - x.shape[0])
        else:
            self.model(x, t, scales=self.scales(), out=out, accumulate=accumulate)
        return True


# ---- style adapters and co-adapters ---------------------------------------------------------------------------------------
# The host side of the two token-sequence T2I networks (gyre_amd/t2i.py GyreHipT2IStyleAdapter / GyreHipT2IFuser):
#   StyleHint                UnifiedPipelineHint_T2i, style path          unified_pipeline.py:843-854, 921-948
#   CoAdapterHint            a spatial hint whose adapter is a co-adapter  unified_pipeline.py:886-892, 953-954
#   build_t2i_conditioning   UNetWithT2I.__init__                          unet/core.py:103-211
#   extend_style_context     UNetWithT2I.__call__, the context extension   unet/core.py:220-237
# T2IHint and combine_t2i_states above keep refusing co-adapters and style states: these are the names the new capability enters by.
def normalise_clip_layer(clip_layer, default=None):
    """reference prompt_types.normalise_clip_layer: "final" | "penultimate" | n (the n-th hidden state from the end, n >= 3)"""
    if clip_layer is None:
        clip_layer = default
    if isinstance(clip_layer, int):
        clip_layer = abs(clip_layer)
    if clip_layer == 0 or clip_layer == 1 or clip_layer == "final":
        return "final"
    if clip_layer == 2 or clip_layer == "penultimate":
        return "penultimate"
    return clip_layer


class CoAdapterHint(T2IHint):
    """A spatial hint whose adapter was loaded as a co-adapter (``model._coadapter_type`` names its condition): the weighted states go
    through ``fuser`` together with the request's other co-adapters (build_t2i_conditioning)."""

    def __init__(self, model, image: Tensor, fuser, mask: Optional[Tensor] = None, weight: float = 1.0, soft_injection: bool = False,
                 cfg_only: bool = False):
        cotype = getattr(model, "_coadapter_type", False)
        if not cotype:
            raise ValueError("CoAdapterHint needs an adapter loaded with coadapter=<condition name>")
        if fuser is None:
            raise ValueError("T2i Coadapter model needs a fuser model")
        self._bind(model, image, mask, weight, soft_injection, cfg_only)      # (T2IHint's own constructor keeps refusing co-adapters)
        self.fuser = fuser

    def coadapter_type(self):
        return getattr(self.model, "_coadapter_type", False)


class StyleHint:
    """One style image bound to its style adapter, the host CLIP model and its feature extractor.  Calling it returns the weighted
    style tokens [N, num_token, context_dim].  With a model loaded as a co-adapter it needs the ``fuser`` as well."""

    def __init__(self, model, image: Tensor, clip_model, feature_extractor, fuser=None, mask: Optional[Tensor] = None, weight: float = 1.0,
                 soft_injection: bool = False, cfg_only: bool = False, clip_layer=None):
        import warnings
        if mask is not None:
            warnings.warn("Style T2iAdapters don't make sense with masks - ignoring")
        if soft_injection:
            warnings.warn("Style T2iAdapters don't make sense with soft_injection - ignoring")
        if clip_model is None or feature_extractor is None:
            raise ValueError("T2i Style model needs a clip model and feature extractor")
        if image.ndim == 3:
            image = image[None]
        self.model, self.image = model, normalise_tensor(image, 3)          # (an alpha plane would be the ignored mask)
        self.weight, self.soft_injection, self.cfg_only = weight, False, cfg_only
        self.clip_model, self.feature_extractor, self.fuser, self.clip_layer = clip_model, feature_extractor, fuser, clip_layer
        if self.coadapter_type() and fuser is None:
            raise ValueError("T2i Coadapter model needs a fuser model")
        self.mean, self.std = list(feature_extractor.image_mean), list(feature_extractor.image_std)
        size = feature_extractor.size
        self.clip_size = size["shortest_edge"] if isinstance(size, dict) else size

    def coadapter_type(self):
        return getattr(self.model, "_coadapter_type", False)

    def to(self, device=None, dtype=None):
        self.image = self.image.to(device, dtype)
        return self

    def preprocess(self, image: Tensor) -> Tensor:
        """rescale(image, clip_size, clip_size, "cover") and torchvision's Normalize(image_mean, image_std)"""
        from .images import rescale
        image = rescale(image, self.clip_size, self.clip_size, "cover")
        mean = torch.as_tensor(self.mean, dtype=image.dtype, device=image.device).view(1, -1, 1, 1)
        std = torch.as_tensor(self.std, dtype=image.dtype, device=image.device).view(1, -1, 1, 1)
        return (image - mean) / std

    def __call__(self) -> Tensor:
        layer = normalise_clip_layer(self.clip_layer, "final")
        image = self.preprocess(self.image)
        vision = self.clip_model.vision_model
        first = next(iter(vision.parameters()), None) if hasattr(vision, "parameters") else None
        if first is not None:                              # the CLIP vision tower is a host (PyTorch) model, wherever it lives
            image = image.to(first.device, first.dtype)
        embeds = vision(image, output_hidden_states=(layer != "final"), return_dict=True)
        if layer == "final":
            hidden = embeds.last_hidden_state
        elif layer == "penultimate":
            hidden = embeds.hidden_states[-2]
        else:
            hidden = embeds.hidden_states[-layer]
        result = self.model(hidden.to(device=getattr(self.model, "device", hidden.device), dtype=self.model.dtype)).to(image.dtype)
        return result * self.weight


def _fuse(fuser, coadapters, side):
    """UNetWithT2I._fuse: the states of each condition summed (spatial) or concatenated (style tokens), then the fuser.  side "all":
    every hint as it is; "either": cfg_only hints replaced by zeros."""
    if fuser is None:
        raise ValueError("fuser is missing")
    summed = {}
    for cotype, items in coadapters.items():
        states = [(torch.zeros_like(s) if isinstance(s, Tensor) else [torch.zeros_like(t) for t in s]) if (cfg_only and side == "either") else s
                  for s, cfg_only in items]
        summed[cotype] = [sum(i) for i in zip(*states)] if isinstance(states[0], list) else torch.cat(states, dim=1)
    if not summed:
        return None, None
    return fuser(summed)


def build_t2i_conditioning(hints: Sequence):
    """(states, style): states = {"u", "g", "f"} per-level sums as combine_t2i_states returns them (None without spatial states), style
    = the style tokens [N, T, context_dim] concatenated along the sequence (None without a style hint) - the whole of
    UNetWithT2I.__init__ over standard hints, style hints and co-adapters with their fuser."""
    gs, us, styles, coadapters, spatial_cfg_only, fuser = [], [], [], {}, set(), None
    for hint in hints:
        state, cfg_only = hint(), hint.cfg_only
        cotype = hint.coadapter_type()
        if cotype:
            if isinstance(state, list):
                spatial_cfg_only.add(bool(cfg_only))
                coadapters.setdefault(cotype, []).append((state, bool(cfg_only)))
            else:
                coadapters.setdefault(cotype, []).append((state, False))      # (style tokens are never zeroed, core.py:145)
            fuser = hint.fuser
        elif isinstance(state, list):
            gs.append(state)
            us.append([torch.zeros_like(s) for s in state] if cfg_only else state)
        else:
            styles.append(state)
    if coadapters:
        if len(spatial_cfg_only) <= 1:
            cfg_only = spatial_cfg_only.pop() if spatial_cfg_only else False
            maps, tokens = _fuse(fuser, coadapters, "all")
            if maps is not None:
                gs.append(maps)
                us.append([torch.zeros_like(t) for t in maps] if cfg_only else maps)
            if tokens is not None:
                styles.append(tokens)
        else:                                             # the co-adapters disagree on cfg_only: one fuse per side (core.py:177-191)
            for guided in (True, False):
                maps, tokens = _fuse(fuser, coadapters, "all" if guided else "either")
                if maps is not None:
                    (gs if guided else us).append(maps)
                if not guided and tokens is not None:
                    styles.append(tokens)
    states = None
    if gs:
        assert len(us) == len(gs)
        states = {"u": [sum(i) for i in zip(*us)], "g": [sum(i) for i in zip(*gs)]}
        states["f"] = [torch.cat([u, g], dim=0) for u, g in zip(states["u"], states["g"])]
    return states, (torch.cat(styles, dim=1) if styles else None)


def extend_style_context(encoder_hidden_states: Tensor, style: Optional[Tensor], side: str) -> Tensor:
    """UNetWithT2I.__call__'s context extension: the guided context gets the style tokens appended, the unconditional one its own last
    T rows again; side "f" is cat[unconditional, guided] along the batch."""
    if style is None:
        return encoder_hidden_states
    T = style.shape[1]
    if side == "f":
        uncond, cond = encoder_hidden_states.chunk(2)
    elif side == "u":
        uncond, cond = encoder_hidden_states, None
    else:
        uncond, cond = None, encoder_hidden_states
    res = []
    if uncond is not None:
        res.append(torch.cat([uncond, uncond[:, -T:, :]], dim=1))
    if cond is not None:
        res.append(torch.cat([cond, style.to(cond.dtype)], dim=1))
    return torch.cat(res, dim=0)
