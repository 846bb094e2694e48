"""nn.Module shell over the native T2I adapter (hint image -> one feature map per UNet down level).

The reference's adapter classes (gyre/pipeline/t2i_adapter/models.py ``T2iAdapter_main`` / ``T2iAdapter_light``) wrap the
plain-torch ``Adapter`` / ``Adapter_light`` in diffusers' ModelMixin; the pipeline touches this surface only:

  ``model(image)``                       a list of NCHW states, one per level       unified_pipeline.py:906-919
  ``"cin" in model.config`` / ``.cin``   channels of the hint image = cin // 64      unified_pipeline.py:869
  ``model._coadapter_type``              False for a standard adapter                unified_pipeline.py:953-954
  ``T2iAdapter.from_state_dict(path, torch_dtype, ..., type=..., **config)``         models.py:16-77

Parameters carry the reference's state-dict names, so its ``.pth`` files load with ``load_state_dict``.  All compute happens in
the HIP library (gyre_t2i_forward); there is no PyTorch fallback.

The reference's two token-sequence networks run natively as well: ``GyreHipT2IStyleAdapter`` (``T2iAdapter_style``: CLIP hidden states
-> style tokens) and ``GyreHipT2IFuser`` (``CoAdapterFuser``: the states / tokens of several co-adapters -> gained states / tokens),
both on the gyre_t2i_seq handle.  ``T2iAdapter.from_state_dict`` is the reference's loader over all four types.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import List, Optional

import torch

from . import _lib
from .config import EXTRA_CONDITION, T2IConfig, t2i_config, t2i_fuser_config, t2i_style_config
from .modules import _NativeModule, _build_tree
from .weights import t2i_fuser_param_shapes, t2i_param_shapes, t2i_style_param_shapes


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


def _load_first_checkpoint(path, allow_patterns, ignore_patterns):
    import fnmatch
    paths = [os.path.basename(p) for pat in ("*.pt", "*.pth") for p in sorted(glob.glob(os.path.join(path, pat)))]
    if allow_patterns:
        paths = [p for p in paths if any(fnmatch.fnmatch(p, a) for a in allow_patterns)]
    if ignore_patterns:
        paths = [p for p in paths if not any(fnmatch.fnmatch(p, a) for a in ignore_patterns)]
    if not paths:
        raise RuntimeError(f"No model found for T2iAdapter at {path}")
    return torch.load(os.path.join(path, paths[0]), map_location="cpu", weights_only=True)


class _SeqModule(_NativeModule):
    """What the two token-sequence networks share: the gyre_t2i_seq handle and its configuration struct."""

    _kind = "t2i_seq"
    _coadapter_type = False

    def _c_cfg(self):
        c, cfg = self.config, _lib.T2ISeqCfg()
        cfg.kind = 1 if c.type == "fuser" else 0
        cfg.width, cfg.num_head, cfg.n_layers = c.width, c.num_head, c.n_layes
        cfg.num_token, cfg.context_dim = int(c.get("num_token", 0)), int(c.get("context_dim", 0))
        for i, ch in enumerate(c.get("unet_channels", (0, 0, 0, 0))):
            cfg.unet_channels[i] = ch
        return cfg

    def _ws_ptr(self, need: int, dev) -> int:
        if need == 0:
            _lib.check(-1, self._L())
        return (self._workspace(need, dev).data_ptr() + 255) & ~255

    def _check_len(self, n_tokens: int) -> None:
        c = self.config
        limit = self._L().gyre_op_seq_attn_max_len(c.width // c.num_head)
        if n_tokens > limit:
            raise NotImplementedError(f"a sequence of {n_tokens} tokens exceeds the {limit} the native attention kernel holds at head "
                                      f"dim {c.width // c.num_head}")

    @staticmethod
    def _float(t: torch.Tensor) -> torch.Tensor:
        return (t if t.dtype in (torch.float32, torch.bfloat16, torch.float16) else t.to(torch.float32)).contiguous()


class GyreHipT2IStyleAdapter(_SeqModule):
    """Drop-in for the reference's T2iAdapter_style: ``model(clip_hidden_states [N, S, width]) -> [N, num_token, context_dim]``."""

    def __init__(self, config: Optional[dict] = None, **kw):
        super().__init__()
        cfg = dict(config or {})
        cfg.update(kw)
        cfg.pop("type", None)
        self.config: T2IConfig = t2i_style_config(**cfg)
        _build_tree(self, t2i_style_param_shapes(self.config))

    def _shapes(self):
        return t2i_style_param_shapes(self.config)

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        c = self.config
        if x.ndim != 3 or x.shape[2] != c.width or x.shape[1] < 1:
            raise ValueError(f"expected CLIP hidden states [N, S, {c.width}], got {tuple(x.shape)}")
        N, S, _ = x.shape
        self._check_len(S + c.num_token)
        dev = x.device
        h = self._sync(dev)
        x = self._float(x)
        _lib.require_gpu_tensor(x, "hidden states")
        L = self._L()
        with torch.cuda.device(dev):
            need = L.gyre_t2i_seq_workspace_bytes(C.c_void_p(h), N, S, 0)
            wp = self._ws_ptr(need, dev)
            out = torch.empty((N, c.num_token, c.context_dim), dtype=self.dtype, device=dev)
            _lib.check(L.gyre_t2i_style_forward(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()), _lib.dtype_code(x),
                                                N, S, C.c_void_p(wp), need, C.c_void_p(out.data_ptr()), _lib.dtype_code(out)), L)
        return out


class GyreHipT2IFuser(_SeqModule):
    """Drop-in for the reference's CoAdapterFuser: ``fuser(features)`` over an ordered mapping (or a list of pairs) condition name ->
    four spatial states (a list) or one token tensor [N, T, width]; returns (four summed gained maps | None, gained tokens | None)."""

    def __init__(self, config: Optional[dict] = None, **kw):
        super().__init__()
        cfg = dict(config or {})
        cfg.update(kw)
        cfg.pop("type", None)
        self.config: T2IConfig = t2i_fuser_config(**cfg)
        _build_tree(self, t2i_fuser_param_shapes(self.config))

    def _shapes(self):
        return t2i_fuser_param_shapes(self.config)

    @torch.no_grad()
    def forward(self, features):
        items = list(features.items()) if hasattr(features, "items") else list(features)
        if not items:
            return None, None
        c = self.config
        first = items[0][1]
        dev = (first[0] if isinstance(first, (list, tuple)) else first).device
        h = self._sync(dev)
        L = self._L()
        sdt = _lib.STORAGE_TORCH_DTYPE[self._handle_storage]
        arr = (_lib.FuserInput * len(items))()
        keep, N, tdt, n_sp, S, hw = [], None, None, 0, 0, None
        for e, (name, v) in zip(arr, items):
            if name not in EXTRA_CONDITION:
                raise ValueError(f"unknown co-adapter condition {name!r}")
            e.task = EXTRA_CONDITION[name]
            if isinstance(v, (list, tuple)):
                if len(v) != 4 or any(m.ndim != 4 or m.shape[1] != ch for m, ch in zip(v, c.unet_channels)):
                    raise ValueError(f"{name}: expected four states with {c.unet_channels} channels")
                if hw is not None and [tuple(m.shape[2:]) for m in v] != hw:
                    raise ValueError("the co-adapters' states differ in size")
                hw = [tuple(m.shape[2:]) for m in v]
                v = [m.to(sdt).contiguous() for m in v]                 # the states enter in the storage type
                for i, m in enumerate(v):
                    e.in_[i], e.h[i], e.w[i] = m.data_ptr(), m.shape[2], m.shape[3]
                n_sp += 1
                batch = v[0].shape[0]
            else:
                if v.ndim != 3 or v.shape[2] != c.width or v.shape[1] < 1:
                    raise ValueError(f"{name}: expected tokens [N, T, {c.width}], got {tuple(v.shape)}")
                v = self._float(v)
                if tdt is not None and v.dtype != tdt:
                    v = v.to(tdt)
                tdt = v.dtype
                e.tokens, e.in_[0] = v.shape[1], v.data_ptr()
                S += v.shape[1]
                batch = v.shape[0]
                v = [v]
            for m in v:
                _lib.require_gpu_tensor(m, f"{name} input")
            if N is not None and batch != N:
                raise ValueError("the co-adapters' inputs differ in batch size")
            N = batch
            keep.append(v)
        self._check_len(S + 4 * n_sp)
        with torch.cuda.device(dev):
            need = L.gyre_t2i_seq_workspace_bytes(C.c_void_p(h), N, S, n_sp)
            wp = self._ws_ptr(need, dev)
            maps = [torch.empty((N, ch, fh, fw), dtype=sdt, device=dev) for ch, (fh, fw) in zip(c.unet_channels, hw)] if n_sp else None
            seq = torch.empty((N, S, c.width), dtype=tdt, device=dev) if S else None
            mp = (C.c_void_p * 4)(*[m.data_ptr() for m in maps]) if maps else None
            _lib.check(L.gyre_t2i_fuser_forward(C.c_void_p(h), C.c_void_p(_lib.stream_ptr(dev)), arr, len(items),
                                                _lib.dtype_code(seq) if S else 0, N, C.c_void_p(wp), need, mp,
                                                C.c_void_p(seq.data_ptr()) if S else None), L)
            torch.cuda.current_stream(dev).synchronize()                # the converted inputs in `keep` may now be freed
        return maps, seq


class T2iAdapter:
    """The reference's loader surface (t2i_adapter/models.py:16-77), what ``engines.yaml``'s ``T2iAdapter/from_state_dict(...)``
    names: dispatches on ``type`` to the native main / light / style / fuser module and records ``_coadapter_type``."""

    @classmethod
    def from_state_dict(cls, path, torch_dtype="auto", low_cpu_mem_usage=True, allow_patterns=(), ignore_patterns=(),
                        coadapter=False, **config):
        t2i_type = config.pop("type", "main")
        if t2i_type in ("main", "light"):
            adapter = GyreHipT2IAdapter(type=t2i_type, **config)
        elif t2i_type == "style":
            adapter = GyreHipT2IStyleAdapter(**config)
        elif t2i_type == "fuser":
            adapter = GyreHipT2IFuser(**config)
        else:
            raise ValueError(f"Unknown T2i Adapter type {t2i_type}")
        adapter.load_state_dict(_load_first_checkpoint(path, allow_patterns, ignore_patterns))
        if torch_dtype != "auto":
            adapter.to(torch_dtype)
        adapter._source = path
        adapter._coadapter_type = coadapter
        return adapter.eval()
