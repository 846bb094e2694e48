"""nn.Module shell over the native ControlNet (hint image + latents + timestep + text context -> the UNet's residual inputs).

The reference wraps diffusers-style ``ControlNetModel`` instances (gyre/pipeline/controlnet/models.py) and calls them once per
denoising step from ``UNetWithControlnet`` (unet/core.py:40-64); ``UnifiedPipelineHint_Controlnet`` (unified_pipeline.py:957-1058)
touches this surface only:

  ``model(latents, t, encoder_hidden_states=..., controlnet_cond=image, return_dict=False)``    -> (down residuals, mid residual)
  ``model.config.get("global_pool_conditions", False)``
  ``model.dtype`` / ``model.device``

The native model splits that call in two.  ``bind(image, encoder_hidden_states)`` runs once per request: the conditioning embedding
of the hint image and the cross-attention K / V of the text context do not depend on the step.  ``forward(latents, t, scales=...)``
runs once per step and writes the N + 1 scaled residuals straight into NCHW buffers that are allocated once per request - into a batch
window of them (``out_batch`` / ``out_offset``: the guided half of a CFG-parallel call) and on top of what another control model left
there (``accumulate``).  Parameters carry the diffusers state-dict names, so checkpoints load with ``load_state_dict``.  All compute
happens in the HIP library (gyre_ctrl_bind / gyre_ctrl_forward); there is no PyTorch fallback.

A model keeps ``SLOTS`` independent binds (gyre_ctrl_bind_slot / gyre_ctrl_forward_slot): the leaves of a hires-fix or graft tree
alternate on one control model every step, each with its own hint image, size and context.  A bind may carry one mask per residual
(``masks``: the hint's mask at every residual resolution, multiplied in by the hand-off kernel), a forward a latent mask (``x_mask``:
next to a 9-channel inpaint UNet the control model sees latents * mask channel, multiplied in by the entry pass).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from .config import ControlNetConfig, sd15_controlnet
from .modules import _NativeModule, _build_tree
from .weights import controlnet_param_shapes


class GyreHipControlNet(_NativeModule):
    """Drop-in for the reference's ControlNetModel on the hint path."""

    _kind = "ctrl"

    def __init__(self, config: Optional[ControlNetConfig] = None):
        super().__init__()
        self.config = config or sd15_controlnet()
        c = self.config
        if len(c.conditioning_embedding_out_channels) != 4 or any(ch < 8 or ch % 8 for ch in c.conditioning_embedding_out_channels):
            raise NotImplementedError("the conditioning embedding has four widths, each a multiple of 8")
        if c.controlnet_conditioning_channel_order not in ("rgb", "bgr"):
            raise ValueError(f"unknown controlnet_conditioning_channel_order: {c.controlnet_conditioning_channel_order}")
        self._bound = {}              # slot -> (handle, B, image H, image W, S) of its last bind
        self._outs = None             # residual buffers of the request
        _build_tree(self, controlnet_param_shapes(c))

    def _shapes(self):
        return controlnet_param_shapes(self.config)

    @staticmethod
    def _config_from_json(j: dict) -> ControlNetConfig:
        if j.get("class_embed_type") is not None or j.get("num_class_embeds") is not None:
            raise NotImplementedError("class-conditioned ControlNets are outside the native hot path")
        boc = tuple(j.get("block_out_channels", (320, 640, 1280, 1280)))
        n = len(boc)
        down = j.get("down_block_types", ["CrossAttnDownBlock2D"] * (n - 1) + ["DownBlock2D"])
        # diffusers quirk kept by every SD config: "attention_head_dim" holds the NUMBER of heads per level
        ahd = j.get("num_attention_heads") or j.get("attention_head_dim", 8)
        heads = tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * n
        return ControlNetConfig(in_channels=j.get("in_channels", 4), block_out_channels=boc, layers_per_block=j.get("layers_per_block", 2),
                                attn_levels=tuple("CrossAttn" in d for d in down), num_heads=heads,
                                cross_attention_dim=j.get("cross_attention_dim", 768), norm_num_groups=j.get("norm_num_groups", 32),
                                use_linear_projection=bool(j.get("use_linear_projection", False)),
                                flip_sin_to_cos=j.get("flip_sin_to_cos", True), freq_shift=float(j.get("freq_shift", 0)),
                                conditioning_channels=j.get("conditioning_channels", 3),
                                conditioning_embedding_out_channels=tuple(j.get("conditioning_embedding_out_channels", (16, 32, 96, 256))),
                                controlnet_conditioning_channel_order=j.get("controlnet_conditioning_channel_order", "rgb"),
                                global_pool_conditions=bool(j.get("global_pool_conditions", False)))

    @classmethod
    def from_pretrained(cls, path: str, torch_dtype: Optional[torch.dtype] = None, variant: Optional[str] = None,
                        subfolder: Optional[str] = None, **kw):
        """A diffusers folder (config.json + *.safetensors, or a *.bin where no safetensors file exists)."""
        root = os.path.join(path, subfolder) if subfolder else path
        if any(f.endswith(".safetensors") for f in os.listdir(root)):
            return super().from_pretrained(path, torch_dtype=torch_dtype, variant=variant, subfolder=subfolder, **kw)
        import json
        bins = sorted(f for f in os.listdir(root) if f.endswith(".bin"))
        if not bins:
            raise FileNotFoundError(f"no *.safetensors or *.bin in {root}")
        cfg = None
        if os.path.exists(os.path.join(root, "config.json")):
            with open(os.path.join(root, "config.json")) as f:
                cfg = cls._config_from_json(json.load(f))
        model = cls(cfg)
        model.load_state_dict(torch.load(os.path.join(root, bins[0]), map_location="cpu", weights_only=True))
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        model._source = path
        return model.eval()

    def _c_cfg(self):
        c, cfg = self.config, _lib.CtrlCfg()
        n = len(c.block_out_channels)
        cfg.in_channels, cfg.n_levels = c.in_channels, n
        for i in range(n):
            cfg.block_out_channels[i] = c.block_out_channels[i]
            cfg.attn_levels[i] = int(c.attn_levels[i])
            cfg.num_heads[i] = c.num_heads[i]
            cfg.transformer_depth[i] = c.transformer_depth[i]
        cfg.layers_per_block = c.layers_per_block
        cfg.cross_attention_dim = c.cross_attention_dim
        cfg.norm_num_groups = c.norm_num_groups
        cfg.use_linear_projection = int(c.use_linear_projection)
        cfg.flip_sin_to_cos = int(c.flip_sin_to_cos)
        cfg.freq_shift = c.freq_shift
        cfg.cond_channels = c.conditioning_channels
        for i, ch in enumerate(c.conditioning_embedding_out_channels):
            cfg.cond_embed_channels[i] = ch
        return cfg

    def _invalidate(self):
        super()._invalidate()
        self._bound = {}              # new weights: the embeddings and the projected contexts are stale (the library drops them too)

    def residual_shapes(self, H: int, W: int) -> List[Tuple[int, int, int]]:
        """(channels, h, w) of the N down residuals and the mid residual for H x W latents (a stride-2 convolution rounds an odd size up)."""
        c = self.config
        out, h, w = [(c.block_out_channels[0], H, W)], H, W
        n = len(c.block_out_channels)
        for i, ch in enumerate(c.block_out_channels):
            out += [(ch, h, w)] * c.layers_per_block
            if i < n - 1:
                h, w = (h + 1) // 2, (w + 1) // 2
                out.append((ch, h, w))
        out.append((c.block_out_channels[-1], h, w))
        return out

    SLOTS = 4                         # include/gyre_hip.h GYRE_CTRL_SLOTS

    def _check_slot(self, slot: int) -> int:
        if not isinstance(slot, int) or slot < 0 or slot >= self.SLOTS:
            raise ValueError(f"bind slot must be in [0, {self.SLOTS}), got {slot!r}")
        return slot

    @torch.no_grad()
    def bind(self, image: torch.Tensor, encoder_hidden_states: torch.Tensor, *, slot: int = 0,
             masks: Optional[Sequence[torch.Tensor]] = None) -> None:
        """Once per request: embed the hint image [1 or B, conditioning_channels, 8h, 8w] and project the text context [B, S, D] into
        bind slot ``slot``.  masks: one [1 or B, 1, h_k, w_k] tensor per residual (residual_shapes), copied into the model; every
        residual of this slot is multiplied by its mask on the way out."""
        c = self.config
        slot = self._check_slot(slot)
        if image.ndim != 4 or image.shape[1] != c.conditioning_channels:
            raise ValueError(f"expected a hint image [B,{c.conditioning_channels},H,W], got {tuple(image.shape)}")
        ctx = encoder_hidden_states
        if ctx is None or ctx.ndim != 3 or ctx.shape[2] != c.cross_attention_dim:
            raise ValueError(f"expected encoder_hidden_states [B,S,{c.cross_attention_dim}]")
        B, S = ctx.shape[0], ctx.shape[1]
        Bi, _, H, W = image.shape
        if Bi not in (1, B):
            raise ValueError(f"the hint image needs batch 1 or {B}, got {Bi}")
        if H % 8 or W % 8 or H < 8 or W < 8:
            raise ValueError(f"hint image height and width must be multiples of 8, got {H} x {W}")
        dev = ctx.device
        h = self._sync(dev)
        if image.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            image = image.to(torch.float32)
        if c.controlnet_conditioning_channel_order == "bgr":
            image = torch.flip(image, dims=[1])
        x = image.to(dev).contiguous()
        ctx = ctx.contiguous()
        _lib.require_gpu_tensor(x, "hint image")
        _lib.require_gpu_tensor(ctx, "encoder_hidden_states")
        L = self._L()
        marr = hw = None
        n = mB = 0
        if masks is not None:
            shapes = self.residual_shapes(H // 8, W // 8)
            if len(masks) != len(shapes):
                raise ValueError(f"{len(shapes)} residual masks expected, got {len(masks)}")
            mB = masks[0].shape[0]
            for m, (_, rh, rw) in zip(masks, shapes):
                if m.ndim != 4 or tuple(m.shape) != (mB, 1, rh, rw) or mB not in (1, B):
                    raise ValueError(f"a residual mask must be [1 or {B}, 1, {rh}, {rw}], got {tuple(m.shape)}")
            masks = [m.to(dev, torch.float32).contiguous() for m in masks]
            for m in masks:
                _lib.require_gpu_tensor(m, "residual mask")
            n = len(masks)
            marr = (C.c_void_p * n)(*[m.data_ptr() for m in masks])
            hw = (C.c_int32 * (2 * n))(*[v for m in masks for v in m.shape[-2:]])
        self._bound.pop(slot, None)
        with torch.cuda.device(dev):
            need = L.gyre_ctrl_bind_slot_workspace_bytes(C.c_void_p(h), slot, Bi, H, W, B)
            if need == 0:
                _lib.check(-1, L)
            ws = self._workspace(need, dev)
            wp = (ws.data_ptr() + 255) & ~255
            if slot == 0 and masks is None:            # the entry point every request used before there were slots
                _lib.check(L.gyre_ctrl_bind(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()), _lib.dtype_code(x),
                                            Bi, H, W, C.c_void_p(ctx.data_ptr()), _lib.dtype_code(ctx), B, S, C.c_void_p(wp), need), L)
            else:
                _lib.check(L.gyre_ctrl_bind_slot(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), slot, C.c_void_p(x.data_ptr()),
                                                 _lib.dtype_code(x), Bi, H, W, C.c_void_p(ctx.data_ptr()), _lib.dtype_code(ctx), B, S, marr, hw, n,
                                                 mB, C.c_void_p(wp), need), L)
        self._bound[slot] = (h, B, H, W, S)
        self._outs = None

    def new_outputs(self, B: int, H: int, W: int, device, dtype=None) -> List[torch.Tensor]:
        """The N + 1 residual buffers for a batch of B and H x W latents."""
        return [torch.empty((B, ch, rh, rw), dtype=dtype or self.dtype, device=device) for ch, rh, rw in self.residual_shapes(H, W)]

    @torch.no_grad()
    def forward(self, latents: torch.Tensor, t, *, scales: Optional[Sequence[float]] = None, out: Optional[List[torch.Tensor]] = None,
                accumulate: bool = False, out_batch: Optional[int] = None, out_offset: int = 0, slot: int = 0,
                x_mask: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """The N + 1 residuals of one step (N down residuals, then the mid one), each times its scale, written to samples
        [out_offset, out_offset + B) of ``out`` (batch ``out_batch``; default: B, offset 0).  Without ``out`` the buffers are the
        module's own, allocated at the first step of a request and reused by every later one.  slot: the bind this step runs on.
        x_mask: [1 or B, 1, H, W]; the model sees latents * x_mask (the product in fp32, one rounding to the model's storage)."""
        c = self.config
        slot = self._check_slot(slot)
        if latents.ndim != 4 or latents.shape[1] != c.in_channels:
            raise ValueError(f"expected latents [B,{c.in_channels},H,W], got {tuple(latents.shape)}")
        B, _, H, W = latents.shape
        dev = latents.device
        h = self._sync(dev)
        bound = self._bound.get(slot)
        if bound is None or bound[0] != h:
            raise ValueError("GyreHipControlNet.forward needs a bind(image, encoder_hidden_states) call first")
        _, bB, bH, bW, S = bound
        if B != bB or H * 8 != bH or W * 8 != bW:
            raise ValueError(f"latents {B} x {H} x {W} do not match the bound request (batch {bB}, hint image {bH} x {bW})")
        shapes = self.residual_shapes(H, W)
        n = len(shapes)
        sc = [1.0] * n if scales is None else [float(s) for s in scales]
        if len(sc) != n:
            raise ValueError(f"{n} scales expected (down residuals, then mid), got {len(sc)}")
        out_batch = B if out_batch is None else int(out_batch)
        if out_offset < 0 or out_offset + B > out_batch:
            raise ValueError("the samples [out_offset, out_offset + B) must lie inside out_batch")
        if out is None:
            key = (out_batch, H, W, dev)
            if self._outs is None or self._outs[0] != key:
                if accumulate:
                    raise ValueError("accumulate needs the buffers of an earlier call")
                self._outs = (key, self.new_outputs(out_batch, H, W, dev))
            out = self._outs[1]
        if len(out) != n:
            raise ValueError(f"{n} output buffers expected, got {len(out)}")
        for o, (ch, rh, rw) in zip(out, shapes):
            if tuple(o.shape) != (out_batch, ch, rh, rw) or o.dtype != out[0].dtype or o.device != dev or not o.is_contiguous():
                raise ValueError(f"output buffer must be contiguous {(out_batch, ch, rh, rw)} on {dev}, got {tuple(o.shape)}")
        if isinstance(t, torch.Tensor):
            tt = t.to(dev).to(torch.int64).reshape(-1)
            if tt.numel() == 1:
                tt = tt.expand(B)
        else:
            tt = torch.full((B,), int(t), dtype=torch.int64, device=dev)
        if tt.numel() != B:
            raise ValueError(f"timestep must be a scalar or have {B} elements")
        tt = tt.contiguous()
        x = latents.contiguous()
        _lib.require_gpu_tensor(x, "latents")
        xm, xmB = None, 0
        if x_mask is not None:
            if x_mask.ndim != 4 or x_mask.shape[0] not in (1, B) or tuple(x_mask.shape[1:]) != (1, H, W):
                raise ValueError(f"x_mask must be [1 or {B}, 1, {H}, {W}], got {tuple(x_mask.shape)}")
            xm = x_mask.to(dev, torch.float32).contiguous()
            _lib.require_gpu_tensor(xm, "x_mask")
            xmB = xm.shape[0]
        L = self._L()
        with torch.cuda.device(dev):
            need = L.gyre_ctrl_workspace_bytes(C.c_void_p(h), B, H, W, S)
            if need == 0:
                _lib.check(-1, L)
            ws = self._workspace(need, dev)
            wp = (ws.data_ptr() + 255) & ~255
            arr = (C.c_void_p * n)(*[o.data_ptr() for o in out])
            if slot == 0 and xm is None:
                _lib.check(L.gyre_ctrl_forward(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()), _lib.dtype_code(x),
                                               C.c_void_p(tt.data_ptr()), B, H, W, C.c_void_p(wp), need, (C.c_float * n)(*sc),
                                               1 if accumulate else 0, out_batch, out_offset, arr, n, _lib.dtype_code(out[0])), L)
            else:
                _lib.check(L.gyre_ctrl_forward_slot(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), slot, C.c_void_p(x.data_ptr()),
                                                    _lib.dtype_code(x), None if xm is None else C.c_void_p(xm.data_ptr()), xmB,
                                                    C.c_void_p(tt.data_ptr()), B, H, W, C.c_void_p(wp), need, (C.c_float * n)(*sc),
                                                    1 if accumulate else 0, out_batch, out_offset, arr, n, _lib.dtype_code(out[0])), L)
        return out
