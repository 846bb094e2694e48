"""nn.Module shell over the native T2I adapter (hint image -> one feature map per UNet down level).

The reference's adapter classes (gyre/pipeline/t2i_adapter/models.py ``T2iAdapter_main`` / ``T2iAdapter_light``) wrap the
plain-torch ``Adapter`` / ``Adapter_light`` in diffusers' ModelMixin; the pipeline touches this surface only:

  ``model(image)``                       a list of NCHW states, one per level       unified_pipeline.py:906-919
  ``"cin" in model.config`` / ``.cin``   channels of the hint image = cin // 64      unified_pipeline.py:869
  ``model._coadapter_type``              False for a standard adapter                unified_pipeline.py:953-954
  ``T2iAdapter.from_state_dict(path, torch_dtype, ..., type=..., **config)``         models.py:16-77

Parameters carry the reference's state-dict names, so its ``.pth`` files load with ``load_state_dict``.  All compute happens in
the HIP library (gyre_t2i_forward); there is no PyTorch fallback.  Style adapters and the co-adapter fuser are not built.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import List, Optional

import torch

from . import _lib
from .config import T2IConfig, t2i_config
from .modules import _NativeModule, _build_tree
from .weights import t2i_param_shapes


class GyreHipT2IAdapter(_NativeModule):
    """Drop-in for the reference's T2iAdapter_main / T2iAdapter_light on the hint path."""

    _kind = "t2i"
    _coadapter_type = False

    def __init__(self, config: Optional[dict] = None, **kw):
        super().__init__()
        cfg = dict(config or {})
        cfg.update(kw)
        self.autoinvert = bool(cfg.pop("autoinvert", False))
        self.config: T2IConfig = t2i_config(cfg.pop("type", "main"), **cfg)
        if len(self.config.channels) != 4:
            raise ValueError("a T2I adapter has one width per UNet down level (4)")
        if self.config.cin % 64:
            raise ValueError("cin must be 64 x the hint image's channels")
        if self.config.type == "main" and not self.config.sk and len(set(self.config.channels)) != 1:
            # adapter.py:87-99 feeds skep the output of in_conv: the reference's own block fails on a width change without sk
            raise NotImplementedError("a main adapter with sk=False needs the same width at every level (as in the reference)")
        _build_tree(self, t2i_param_shapes(self.config))

    def _shapes(self):
        return t2i_param_shapes(self.config)

    def _c_cfg(self):
        c, cfg = self.config, _lib.T2ICfg()
        cfg.kind = 1 if c.type == "light" else 0
        cfg.cin, cfg.n_levels, cfg.nums_rb = c.cin, len(c.channels), c.nums_rb
        for i, ch in enumerate(c.channels):
            cfg.channels[i] = ch
        cfg.ksize, cfg.sk, cfg.use_conv = int(c.get("ksize", 3)), int(bool(c.get("sk", False))), int(bool(c.get("use_conv", False)))
        return cfg

    def feature_shapes(self, H: int, W: int) -> List[tuple]:
        """(channels, h, w) of every level for an H x W hint image: the stride-2 convolution rounds an odd size up, the
        average pool down (torch semantics of adapter.py's Downsample)."""
        c = self.config
        up = c.type == "main" and c.get("use_conv", False)
        out, h, w = [], H // 8, W // 8
        for i, ch in enumerate(c.channels):
            if i:
                h, w = ((h + 1) // 2, (w + 1) // 2) if up else (h // 2, w // 2)
            out.append((ch, h, w))
        return out

    @torch.no_grad()
    def forward(self, image: torch.Tensor) -> List[torch.Tensor]:
        c = self.config
        if image.ndim != 4 or image.shape[1] != c.cin // 64:
            raise ValueError(f"expected a hint image [B,{c.cin // 64},H,W], got {tuple(image.shape)}")
        B, _, H, W = image.shape
        if H % 8 or W % 8 or H < 8 or W < 8:
            raise ValueError(f"hint image height and width must be multiples of 8, got {H} x {W}")
        shapes = self.feature_shapes(H, W)
        if min(min(h, w) for _, h, w in shapes) < 1:
            raise ValueError(f"hint image {H} x {W} is too small for the adapter's four levels")
        dev = image.device
        h = self._sync(dev)
        if image.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            image = image.to(torch.float32)
        if self.autoinvert and image.mean() > 0.66:      # more than 2/3 white: assume it needs inverting (models.py:113-119)
            image = 1 - image
        x = image.contiguous()
        _lib.require_gpu_tensor(x, "hint image")
        L = self._L()
        with torch.cuda.device(dev):
            need = L.gyre_t2i_workspace_bytes(C.c_void_p(h), B, H, W)
            if need == 0:
                _lib.check(-1, L)
            ws = self._workspace(need, dev)
            wp = (ws.data_ptr() + 255) & ~255
            outs = [torch.empty((B, ch, fh, fw), dtype=self.dtype, device=dev) for ch, fh, fw in shapes]
            arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            _lib.check(L.gyre_t2i_forward(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()),
                                          _lib.dtype_code(x), B, H, W, C.c_void_p(wp), need, arr, len(outs),
                                          _lib.dtype_code(outs[0])), L)
        return outs

    @classmethod
    def from_state_dict(cls, path, torch_dtype="auto", low_cpu_mem_usage=True, allow_patterns=(), ignore_patterns=(),
                        coadapter=False, **config):
        """The reference's loader (t2i_adapter/models.py:16-77): the first ``*.pt`` / ``*.pth`` of the directory into an adapter
        of ``type`` ("main" or "light") built from that type's default configuration overlaid with ``config``."""
        t2i_type = config.pop("type", "main")
        if t2i_type in ("style", "fuser") or coadapter:
            raise NotImplementedError(f"T2I adapter type {t2i_type!r} / co-adapters are outside the native path")
        if t2i_type not in ("main", "light"):
            raise ValueError(f"Unknown T2i Adapter type {t2i_type}")
        import fnmatch
        paths = [os.path.basename(p) for pat in ("*.pt", "*.pth") for p in sorted(glob.glob(os.path.join(path, pat)))]
        if allow_patterns:
            paths = [p for p in paths if any(fnmatch.fnmatch(p, a) for a in allow_patterns)]
        if ignore_patterns:
            paths = [p for p in paths if not any(fnmatch.fnmatch(p, a) for a in ignore_patterns)]
        if not paths:
            raise RuntimeError(f"No model found for T2iAdapter at {path}")
        adapter = cls(type=t2i_type, **config)
        adapter.load_state_dict(torch.load(os.path.join(path, paths[0]), map_location="cpu", weights_only=True))
        if torch_dtype != "auto":
            adapter.to(torch_dtype)
        adapter._source = path
        return adapter.eval()
