"""Host side of hint-image conditioning with T2I adapters and ControlNets.

  T2IHint              UnifiedPipelineHint_T2i, standard path       unified_pipeline.py:746-786, 906-919
  combine_t2i_states   UNetWithT2I.__init__, standard branch        unet/core.py:128-206 (with AdapterStateList, :67-93)
  ControlNetHint       UnifiedPipelineHint_Controlnet               unified_pipeline.py:957-1058 (run per step by
                                                                    schedulers.UNetWithControlnet, unet/core.py:40-64)

The adapter itself runs natively (gyre_amd/t2i.py); what is here is the per-level weighting of its states and the sums the CFG
wrappers receive.  T2IHint and combine_t2i_states refuse style adapters and co-adapters; those enter through StyleHint, CoAdapterHint
and build_t2i_conditioning at the end of this file (gyre_amd/pipeline.py calls them once per request, engine._hints builds them).  Masked T2I
hints raise NotImplementedError.  The ControlNet itself runs natively too (gyre_amd/controlnet.py): its hint decides the per-residual
scales, which half of a CFG call the model sees, where in the shared residual buffers its outputs land and which of the model's bind
slots it runs on (the leaves of a hires-fix or graft tree alternate on one model every step, each leaf with its own copy of the hint).
A ControlNet hint may carry a mask - explicit, or the alpha plane of an RGBA image: ``resized_mask`` (UnifiedPipelineHint.resized_mask,
unified_pipeline.py:810-828, over gyre_amd.images.resize) brings it to every residual's resolution once per bind and the model
multiplies it in on the device.  Next to a 9-channel inpaint UNet the control model sees latents x mask channel and the hint image x
that mask at image resolution (unified_pipeline.py:1016-1024), computed once per leaf.  ``extend`` on every hint class is
UnifiedPipelineHint.extend (:799-808): a new hint from the stored constructor arguments, updated.
"""
from __future__ import annotations

import inspect
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


def resized_mask(state_shape, mask: Tensor) -> Tensor:
    """UnifiedPipelineHint.resized_mask for a mask that is there: images.resize(mask, (h_state / h_mask, w_state / w_mask)), lanczos3
    with antialiasing, clamped to [0, 1].  state_shape: anything whose last two entries are the state's height and width.  The size of
    one must be a whole multiple of the other's (the reference's two asserts)."""
    from .images import resize
    hs, ws = int(state_shape[-2]), int(state_shape[-1])
    hm, wm = int(mask.shape[-2]), int(mask.shape[-1])
    if max(hm, hs) % min(hm, hs) or max(wm, ws) % min(wm, ws):
        raise ValueError(f"a hint mask of {hm} x {wm} cannot be resized to a state of {hs} x {ws}: one size must be a whole multiple of the other")
    for have, want in ((hm, hs), (wm, ws)):
        if want < have and 3 * (have // want) > have - 1:                 # the stretched lanczos3 reaches 3 x the factor past each edge
            raise ValueError(f"a hint mask of {hm} x {wm} cannot be resized to a state of {hs} x {ws}: lanczos3 over reflect padding needs "
                             "the smaller size to be at least 4 (a hint image of at least 256 pixels a side for an SD control model)")
    return resize(mask, (hs / hm, ws / wm))


class _Extendable:
    def extend(self, callback=None, **kwargs):
        """UnifiedPipelineHint.extend: a new hint of the same class from the constructor arguments this one holds, updated with
        ``kwargs`` and then with what ``callback(**arguments)`` returns.  The new hint shares nothing per-request with this one."""
        keys = [k for k in inspect.signature(self.__init__).parameters if k != "self"]
        cargs = {k: getattr(self, k) for k in keys}
        cargs.update(kwargs)
        if callback is not None:
            cargs.update(callback(**cargs))
        return self.__class__(**cargs)


class T2IHint(_Extendable):
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
            raise NotImplementedError("masked T2I hints (the per-state multiply by the resized mask is not built)")
        channels = model.config.cin // 64 if "cin" in model.config else 3
        self.model, self.image, self.mask = model, normalise_tensor(normalise_tensor(image, 3), channels), None
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


REBIND_EVERY_CALL = False      # private switch for tests and timing: no bind slots, every call binds slot 0 again


def has_bind_slots(model) -> bool:
    """Does this control-model shell keep bind slots, residual masks and a latent mask (GyreHipControlNet: ``SLOTS`` binds,
    ``bind(..., slot=, masks=)``, ``forward(..., slot=, x_mask=)``)?  A shell with the older surface - ``bind(image, ctx)`` alone - can
    serve neither a masked hint nor the leaves of a hires-fix / graft tree, and keeps raising NotImplementedError for them."""
    return int(getattr(model, "SLOTS", 0) or 0) > 0


def _is_bound(model, slot: int) -> bool:
    bound = getattr(model, "_bound", None)
    return slot in bound if isinstance(bound, dict) else bound is not None


class ControlNetHint(_Extendable):
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
        if mask is not None and not has_bind_slots(model):
            raise NotImplementedError("masked ControlNet hints need a control model that takes residual masks (bind(..., masks=))")
        self.model, self.image = model, normalise_tensor(image, model.config.get("conditioning_channels", 3))
        self.mask = mask
        self.weight, self.soft_injection, self.cfg_only = weight, soft_injection, cfg_only
        self._token = object()                                        # who bound a slot of the model last: (token, side, ...)
        self._ctx = {}                                                # side -> (the stack's context, the context the model sees)
        self._slots = {}                                              # side -> bind slot of the model (reserve); 0 where not reserved
        self._pyramid = None                                          # the mask at every residual's resolution, built at the first bind
        self._inpaint = {}                                            # side -> what a 9-channel leaf binds (_inpaint_state)

    def scales(self):
        """weight x logspace(-1, 0, N + 1)[k] for down residual k and the last point for the mid residual; the weight alone without
        soft injection (N + 1 = 13 for SD)."""
        n = self.model.config.n_residuals + 1
        if not self.soft_injection:
            return [float(self.weight)] * n
        return [float(self.weight) * float(lw) for lw in torch.logspace(-1, 0, n)]

    def to(self, device=None, dtype=None):
        self.image = self.image.to(device, dtype)
        if self.mask is not None:
            self.mask = self.mask.to(device, dtype)
        self._pyramid, self._inpaint = None, {}
        return self

    def sides(self, cfg: bool, sequential: bool):
        """the CFG sides this hint runs on in a request"""
        if not cfg:
            return ("g",)
        if not sequential:
            return ("f",)
        return ("g",) if self.cfg_only else ("g", "u")

    def reserve(self, plan: dict, sides: Sequence[str]) -> None:
        """Take one bind slot of the model per side, from ``plan`` ({id(model): slots taken so far}, one plan per request)."""
        limit = getattr(self.model, "SLOTS", 4)
        for side in sides:
            n = plan.get(id(self.model), 0)
            if n >= limit:
                raise NotImplementedError(f"more than {limit} binds on one control model (GYRE_CTRL_SLOTS = {limit}: one per hint, leaf of "
                                          "the hires-fix / graft tree and sequential CFG side)")
            plan[id(self.model)] = n + 1
            self._slots[side] = n

    def mask_pyramid(self, mask: Tensor) -> List[Tensor]:
        """``mask`` (image resolution) at the resolution of each of the N + 1 residuals"""
        H, W = self.image.shape[-2:]
        return [resized_mask((rh, rw), mask) for _, rh, rw in self.model.residual_shapes(H // 8, W // 8)]

    def _inpaint_state(self, side, extra: Tensor, batch: int):
        """What a 9-channel inpaint leaf binds and runs with (unified_pipeline.py:1016-1024): the latent mask the control model's latents
        are multiplied by, the hint image times that mask at image resolution (times the hint's own mask) and the residual masks made
        from the combined mask.  The mask channel is constant over a request: computed once per side, keyed on the identity of the leaf's
        extra-channels tensor."""
        kept = self._inpaint.get(side)
        if kept is None or kept[0] is not extra or kept[1] != batch:
            m = extra[:, [0]].to(self.image.device, torch.float32)
            if m.shape[0] != batch:
                m = m.repeat(batch // m.shape[0], 1, 1, 1)
            combined = resized_mask(self.image.shape, m).to(self.image.dtype)
            if self.mask is not None:
                combined = combined * self.mask
            kept = self._inpaint[side] = (extra, batch, m.contiguous(), (self.image * combined).contiguous(), self.mask_pyramid(combined))
        return kept[2:]

    def _bind(self, side, ctx, image=None, masks=None):
        """The embedding of the image and the projected context live in a bind slot of the model, one request at a time: bind again
        only when another hint, another side (without reserved slots sequential CFG alternates two contexts on slot 0) or another
        request used the slot last."""
        kept = self._ctx.get(side)
        if kept is None or kept[0] is not ctx:
            seen = ctx.chunk(2)[-1].contiguous() if (self.cfg_only and side == "f") else ctx
            kept = self._ctx[side] = (ctx, seen)
        if image is None:
            image = self.image
            if self.mask is not None:
                if self._pyramid is None:
                    self._pyramid = self.mask_pyramid(self.mask)
                masks = self._pyramid
        slot = 0 if REBIND_EVERY_CALL else self._slots.get(side, 0)
        owners = self.model.__dict__.setdefault("_bind_owners", {})
        owner = owners.get(slot)
        if (REBIND_EVERY_CALL or owner is None or owner[0] is not self._token or owner[1] != side or owner[2] is not kept[1]
                or owner[3] is not image or not _is_bound(self.model, slot)):
            kw = {}
            if slot:
                kw["slot"] = slot
            if masks is not None:
                kw["masks"] = masks
            self.model.bind(image, kept[1], **kw)
            owners[slot] = (self._token, side, kept[1], image)
        return slot

    def run(self, side: str, latents: Tensor, t, encoder_hidden_states: Tensor, out, accumulate: bool, extra: Optional[Tensor] = None):
        """Adds (accumulate) or assigns this hint's residuals for one UNet call into ``out`` (N + 1 NCHW buffers at the batch of
        ``latents``).  False when the hint contributes nothing on this side (cfg_only on "u").  extra: the extra channels of a
        9-channel inpaint leaf (mask, masked-image latents), the tensor the leaf keeps for the whole request."""
        x, B = latents[:, 0:4], latents.shape[0]
        if self.cfg_only and side == "u":
            return False
        half = self.cfg_only and side == "f"                          # the guided half only, into the upper half; the lower half is zero
        if half:
            x = x.chunk(2)[-1]
            t = t.chunk(2)[-1] if isinstance(t, torch.Tensor) and t.ndim > 0 and t.numel() > 1 else t
        kw = {}
        if latents.shape[1] == 9:
            if not has_bind_slots(self.model):
                raise NotImplementedError("ControlNet hints with a 9-channel inpaint UNet need a control model that takes a latent mask "
                                          "(forward(..., x_mask=))")
            if extra is None:
                raise ValueError("a ControlNet hint next to a 9-channel inpaint UNet needs the leaf's extra channels (extra=...)")
            x_mask, image, masks = self._inpaint_state(side, extra, x.shape[0])
            slot = self._bind(side, encoder_hidden_states, image, masks)
            kw["x_mask"] = x_mask
        else:
            slot = self._bind(side, encoder_hidden_states)
        if slot:
            kw["slot"] = slot
        if half:
            kw.update(out_batch=B, out_offset=B - x.shape[0])
        self.model(x, t, scales=self.scales(), out=out, accumulate=accumulate, **kw)
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


class StyleHint(_Extendable):
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
        self.weight, self.soft_injection, self.cfg_only, self.mask = weight, False, cfg_only, None
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
