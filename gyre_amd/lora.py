"""LoRA for the native UNet: merged into the weights before they are repacked for the kernels.

The reference attaches a forward hook to every targeted nn.Linear / nn.Conv2d that adds
``up(down(input)) * (alpha / r) * scale`` to the layer output (gyre/pipeline/lora.py:96-160), applied per request
(unified_pipeline.py:2207-2233) and removed at the start of the next one (:2190-2200).  The native UNet is one C call
with no per-layer Python hooks, so the same linear map is folded into the weight instead:

    Linear:  W' = W + s * up @ down                      (y = x W'^T  ==  x W^T + s * (x down^T) up^T)
    Conv2d:  W' = W + s * einsum(up[o,r,1,1], down[r,i,kh,kw])   (1x1 "up" after a kxk "down", same stride/padding)

with s = scale * alpha / r (alpha absent -> 1).  Key formats as detected by reference lora.py:58-93:
  kohya-ss   ``lora_unet_<module path with _>.lora_down.weight / .lora_up.weight / .alpha``   (lora.py:271-330)
  diffusers  ``<path>.processor.<to_q|to_k|to_v|to_out>_lora.down.weight / .up.weight``        (lora.py:232-268)
  cloneofsimo needs the un-vendored lora_diffusion submodule's module-search order -> NotImplementedError.
Text-encoder entries (``lora_te_``) are ignored here: they are gyre_amd/text_adapters.py's.

The touched base weights are kept (CPU copies) so that removing / re-scaling restores them bit-exactly.

Precision: the merge happens in fp32 and the merged fp32 tensor is what the native module uploads
(``unet._weight_overrides``, consumed by modules._NativeModule._upload_source), so base + delta is rounded to bf16 once,
inside the repack kernel.  Writing the sum back into a bf16 / fp16 master parameter first would round it against the
master's grid: a delta element below half an ulp of W (|delta| < 0.2-0.4 % of |W|, typical for LoRA) would vanish,
which the reference's activation-space hook never does.  The master parameter also receives the (rounded) merged value,
for ``state_dict()`` consumers only.

Device path (``attach_lora`` / ``set_attached_scale`` / ``detach_loras``): the same map without the host.  The factors are kept
as they come (never multiplied out), live on the module's device in their own dtype, and for each TOUCHED weight one
``gyre_unet_set_weight_delta`` call hands the untouched master parameter and the factor pairs, as LORA terms, to the fused
repack kernel (csrc/kernels_lyco.hip): base + sum_j s_j up_j down_j in fp32, rounded once.  Untouched weights are not uploaded again, and
detaching re-issues the touched keys with zero pairs, which restores the base bits.  On this path the master parameters are
NEVER written: ``state_dict()`` keeps showing the base weights while a LoRA is attached - which is what the reference's hooks do
(they leave ``module.weight`` alone).  The two paths do not stack: attaching onto a host-merged module, or merging into a module
with attached LoRAs, is a ValueError.
"""
from __future__ import annotations

import re
from typing import Dict, Mapping, Optional

import torch

Tensor = torch.Tensor

_DETECT = ((":0:up", "cloneofsimo"), (".lora_up.weight", "kohya-ss"), (".to_k_lora.up.weight", "diffusers"))
_KOHYA_FIELDS = (".lora_up.weight", ".lora_down.weight", ".alpha")


def detect_lora_type(lora: Mapping[str, Tensor]) -> str:
    kind = None
    for key in lora.keys():
        for pat, name in _DETECT:
            if key.endswith(pat):
                kind = name
                break
        if kind:
            break
    if kind is None:
        raise ValueError("Unknown LoRA format (or not a LoRA)")
    if kind == "kohya-ss":
        for key in lora.keys():
            if not key.endswith(_KOHYA_FIELDS):
                raise ValueError("LoRA contains unknown fields, probably a Lycoris")
    return kind


def lora_delta(up: Tensor, down: Tensor, alpha: Optional[Tensor] = None) -> Tensor:
    """The weight-space image of one LoRA pair, without the user scale (fp32)."""
    r = down.shape[0]
    iscale = float(alpha) / r if alpha is not None else 1.0
    up, down = up.to(torch.float32), down.to(torch.float32)
    if down.ndim == 2:
        return (up @ down) * iscale
    if down.ndim == 4:
        if up.shape[2:] != (1, 1):
            raise ValueError("conv LoRA: the up projection must be 1x1")
        return torch.einsum("or,rikl->oikl", up[:, :, 0, 0], down) * iscale
    raise ValueError(f"Can't apply LoRA of rank-{down.ndim} tensors")


def _flat_names(params) -> Dict[str, str]:
    """kohya / LyCORIS module names (the weight's module path with ``_`` for ``.``) -> weight-parameter name"""
    return {name[:-len(".weight")].replace(".", "_"): name for name in params if name.endswith(".weight")}


def _pairs(unet: torch.nn.Module, lora: Mapping[str, Tensor]):
    """The key rules of both paths: yields (weight-parameter name, up, down, alpha or None) per targeted weight."""
    params = dict(unet.named_parameters())
    kind = detect_lora_type(lora)
    if kind == "cloneofsimo":
        raise NotImplementedError("cloneofsimo LoRA files need lora_diffusion's module search order (not vendored)")
    if kind == "kohya-ss":
        flat = _flat_names(params)
        for key in lora.keys():
            if not key.endswith(".lora_down.weight"):
                continue
            if key.startswith("lora_te_"):
                continue
            if not key.startswith("lora_unet_"):
                raise ValueError(f"Unknown key in Kohya LoRA, don't know how to apply - {key}")
            mod = key[len("lora_unet_"):].split(".")[0]
            if mod not in flat:
                raise RuntimeError(f"Couldn't find model for {key} when applying LoRA")
            yield flat[mod], lora[key.replace(".lora_down.", ".lora_up.")], lora[key], \
                lora.get(key.replace(".lora_down.weight", ".alpha"))
        return
    for key in lora.keys():                                                   # diffusers attention-processor format
        if not key.endswith(".down.weight"):
            continue
        fixed = re.sub(r"processor.(.+)_lora.down.weight$",
                       lambda m: m[1] + ".0" if m[1] == "to_out" else m[1], key)
        name = fixed + ".weight"
        if name not in params:
            raise RuntimeError(f"Couldn't find model for {key} when applying LoRA")
        yield name, lora[key.replace(".down.weight", ".up.weight")], lora[key], None


def _targets(unet: torch.nn.Module, lora: Mapping[str, Tensor]) -> Dict[str, Tensor]:
    """weight-parameter name -> unscaled delta"""
    out: Dict[str, Tensor] = {}
    for name, up, down, alpha in _pairs(unet, lora):
        out[name] = lora_delta(up, down, alpha)
    return out


def _state(unet):
    st = getattr(unet, "_lora_state", None)
    if st is None:
        st = {"base": {}, "loras": {}}          # base: name -> original weight (CPU); loras: id -> (deltas, scale)
        unet._lora_state = st
    return st


@torch.no_grad()
def _rebuild(unet) -> None:
    st = _state(unet)
    params = dict(unet.named_parameters())
    for name, base in st["base"].items():
        w = base.to(torch.float32)
        for deltas, scale in st["loras"].values():
            if name in deltas and scale != 0:
                d = deltas[name]
                if d.shape != w.shape:
                    raise ValueError(f"LoRA delta for {name} has shape {tuple(d.shape)}, weight {tuple(w.shape)}")
                w = w + d * scale
        p = params[name]
        p.copy_(w.to(p.device, p.dtype))
        if st["loras"] and p.dtype != torch.float32:
            ov = getattr(unet, "_weight_overrides", None)
            if ov is None:
                ov = unet._weight_overrides = {}
            ov[name] = w                      # fp32, uploaded instead of the rounded master
        elif getattr(unet, "_weight_overrides", None):
            unet._weight_overrides.pop(name, None)
    if not st["loras"]:
        st["base"].clear()
        if getattr(unet, "_weight_overrides", None):
            unet._weight_overrides.clear()
    if hasattr(unet, "_invalidate"):
        unet._invalidate()                       # the native copy is repacked from the merged weights at next use


def _refuse_attached(unet) -> None:
    if (getattr(unet, "_lora_attached", None) or {"loras": {}})["loras"]:
        raise ValueError("this module has attached (device-path) LoRAs: the two LoRA paths do not stack - detach_loras() first")


@torch.no_grad()
def apply_lora(unet, lora: Mapping[str, Tensor], lora_id, scale: float = 1.0) -> int:
    """Merge one LoRA (a dict of tensors, e.g. safetensors.torch.load_file) under ``lora_id``.  Returns the number of
    weights touched."""
    _refuse_attached(unet)
    return _merge(unet, _targets(unet, lora), lora_id, scale)


@torch.no_grad()
def _merge(unet, deltas: Dict[str, Tensor], lora_id, scale: float) -> int:
    """Register ``deltas`` (weight-parameter name -> unscaled fp32 delta: a LoRA's, or a LyCORIS file's from lycoris.apply_lycoris)
    under ``lora_id`` and rebuild the touched weights."""
    st = _state(unet)
    params = dict(unet.named_parameters())
    for name in deltas:
        if name not in st["base"]:
            st["base"][name] = params[name].detach().to("cpu", copy=True)
    st["loras"][lora_id] = (deltas, float(scale))
    _rebuild(unet)
    return len(deltas)


def set_lora_scale(unet, lora_id, scale: float = 1.0) -> None:
    st = _state(unet)
    if lora_id not in st["loras"]:
        raise KeyError(lora_id)
    st["loras"][lora_id] = (st["loras"][lora_id][0], float(scale))
    _rebuild(unet)


def remove_lora_from_model(unet) -> None:
    st = _state(unet)
    if st["loras"]:
        st["loras"].clear()
        _rebuild(unet)


# ---- device path: factors stay factors, merged inside the repack kernel -------------------------------------------------
_FACTOR_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class Term:
    """One gyre_delta_term with its device tensors: ``kind`` (_lib.DELTA_*), ``ops`` = up to two (up, down) pairs (up None for a
    dense operand), ``w1`` (KRON: dense fp32 [O1, I1]) and the file scale.  A LoRA pair is a LORA term (lora_term); the LyCORIS
    forms are lycoris.make_term's."""

    def __init__(self, kind, ops, scale, w1=None):
        self.kind, self.ops, self.scale, self.w1 = kind, ops, scale, w1

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        return Term(self.kind, [(mv(u), mv(d)) for u, d in self.ops], self.scale, mv(self.w1))

    def tensors(self):
        return [t for pair in self.ops for t in pair if t is not None] + ([self.w1] if self.w1 is not None else [])

    def fits(self, w: Tensor) -> bool:
        """Do the operands give a delta of ``w``'s shape (the kernel trusts this)?"""
        from . import _lib
        O, I = w.shape[0], w.shape[1]
        kk = w.numel() // (O * I)
        if not all(t.is_contiguous() for t in self.tensors()):
            return False
        if self.kind == _lib.DELTA_KRON:
            if self.w1 is None or self.w1.ndim != 2 or self.w1.dtype != torch.float32:
                return False
            O1, I1 = self.w1.shape
            if O % O1 or I % I1:
                return False
            O, I = O // O1, I // I1
        for up, down in self.ops:
            if up is None:
                if down.numel() != O * I * kk or down.shape[0] != O:
                    return False
            elif up.ndim != 2 or up.shape[0] != O or up.dtype != down.dtype or down.shape[0] != up.shape[1] or up.shape[1] < 1 \
                    or down.numel() != up.shape[1] * I * kk:
                return False
        return True

    def fill(self, c, user_scale: float) -> None:
        from . import _lib
        c.kind, c.scale = self.kind, user_scale * self.scale
        for q, (up, down) in enumerate(self.ops):
            c.up[q], c.down[q] = (None if up is None else up.data_ptr()), down.data_ptr()
            c.dtype[q], c.rank[q] = _lib.dtype_code(down), (0 if up is None else up.shape[1])
        if self.w1 is not None:
            c.w1, c.O1, c.I1 = self.w1.data_ptr(), self.w1.shape[0], self.w1.shape[1]


class Factors:
    """One LoRA or LyCORIS file's terms on a device, as attach_loras keeps them: ``terms[name] = Term`` per touched weight.
    ``source`` keeps the tensors mapping they were made from referenced (an identity-keyed cache of uploads must not see its key's
    address recycled)."""

    def __init__(self, terms: Dict[str, Term], device, source=None):
        self.terms, self.device, self.source = terms, device, source

    def names(self):
        return self.terms.keys()

    def hits(self, name) -> list:
        """What hits the weight ``name``: [Term], or []."""
        return [self.terms[name]] if name in self.terms else []

    def to(self, device):
        """These factors on ``device``: this object where they already are, a NEW one otherwise (an upload may be shared between
        modules and devices - it is never changed in place)."""
        if device == self.device:
            return self
        return Factors({k: t.to(device) for k, t in self.terms.items()}, device, self.source)


def fix_factor(t: Tensor, device) -> Tensor:
    """A file tensor as the kernels read it: on ``device``, contiguous, in its own dtype where that is fp32 / bf16 / fp16."""
    return (t if t.dtype in _FACTOR_DTYPES else t.to(torch.float32)).detach().to(device).contiguous()


def lora_term(up: Tensor, down: Tensor, alpha, w: Tensor, name: str, device) -> Term:
    """The LORA term of one LoRA pair for the weight ``w`` (its shape only): up [O, r] (a conv's 1 x 1 up flattened), down
    [r, I(, KH, KW)] on ``device``, scale alpha / r (alpha absent: 1).  Each factor keeps its own dtype unless the two differ - a
    term's pair has ONE dtype, so both are then promoted to fp32.  ValueError where the pair does not give the weight's shape.
    The one constructor of a LoRA file's terms: upload_factors here and text_adapters.upload_text_factors."""
    from . import _lib
    if down.ndim not in (2, 4) or up.ndim != down.ndim:
        raise ValueError(f"Can't apply LoRA of rank-{down.ndim} tensors")
    if down.ndim == 4 and tuple(up.shape[2:]) != (1, 1):
        raise ValueError("conv LoRA: the up projection must be 1x1")
    r = down.shape[0]
    if r < 1 or up.shape[1] != r:
        raise ValueError(f"LoRA for {name}: up has rank {up.shape[1]}, down rank {r}")
    if w.ndim != down.ndim or up.shape[0] != w.shape[0] or tuple(down.shape[1:]) != tuple(w.shape[1:]):
        raise ValueError(f"LoRA for {name}: up {tuple(up.shape)} x down {tuple(down.shape)} does not give the weight's "
                         f"shape {tuple(w.shape)}")
    up, down = fix_factor(up, device).reshape(up.shape[0], r), fix_factor(down, device)
    if up.dtype != down.dtype:
        up, down = up.float(), down.float()
    return Term(_lib.DELTA_LORA, [(up, down)], float(alpha) / r if alpha is not None else 1.0)


def upload_factors(unet, lora: Mapping[str, Tensor], device=None) -> Factors:
    """Parse ``lora`` (the key rules of apply_lora) and put its factors on ``device`` (default: the module's) as LORA terms
    (lora_term); nothing is multiplied out.  Shapes are checked against the weights they target (ValueError)."""
    device = torch.device(device) if device is not None else unet.device
    params = dict(unet.named_parameters())
    return Factors({name: lora_term(up, down, alpha, params[name], name, device) for name, up, down, alpha in _pairs(unet, lora)},
                   device, lora)


def _attached(unet):
    at = getattr(unet, "_lora_attached", None)
    if at is None:
        at = {"loras": {}}                       # id -> (Factors, user scale), in attach order
        unet._lora_attached = at
    return at


def _issue(unet, names) -> None:
    """One gyre_unet_set_weight_delta call for each of ``names`` on the module's live handle: the untouched master parameter plus
    every attached term (a LoRA pair is a LORA term) that hits the key, in attach order (none: the base bits).  A module whose
    native copy is stale anyway (``_dirty``: after ``.to(...)``) is left to ``_sync``, which re-applies the attached set behind its
    full upload."""
    import ctypes as C
    from . import _lib
    names = list(names)
    if not names:
        return
    if getattr(unet, "_handle", None) is not None and not unet._dirty:
        at = _attached(unet)
        params = dict(unet.named_parameters())
        dev = unet._handle_device
        L = unet._L()
        for lid, (f, scale) in list(at["loras"].items()):       # this module's entry follows it to the handle's device
            if f.device != dev:
                at["loras"][lid] = (f.to(dev), scale)
        # everything is checked before the first call, so a refusal leaves the native copy as it was: the kernel trusts these shapes
        plan = {}
        for name in names:                       # (scale 0 contributes nothing, as in the host merge)
            w = params[name]
            plan[name] = [(term, scale) for f, scale in at["loras"].values() if scale != 0 for term in f.hits(name)]
            if len(plan[name]) > _lib.DELTA_MAX_TERMS:
                raise ValueError(f"{len(plan[name])} LoRA pairs / LyCORIS terms hit {name}: at most {_lib.DELTA_MAX_TERMS} per weight")
            for term, _ in plan[name]:
                if w.ndim not in (2, 4) or not term.fits(w):
                    raise ValueError(f"LoRA / LyCORIS term does not fit {name} {tuple(w.shape)} (factors uploaded for another model?)")
        try:
            with torch.cuda.device(dev):
                st = _lib.stream_ptr(dev)
                for name, hits in plan.items():
                    base = params[name].detach()
                    base = (base if base.device == dev else base.to(dev)).contiguous()
                    shape = (C.c_int64 * base.ndim)(*base.shape)
                    arr = (_lib.DeltaTerm * max(len(hits), 1))()
                    for j, (term, scale) in enumerate(hits):
                        term.fill(arr[j], scale)
                    _lib.check(L.gyre_unet_set_weight_delta(C.c_void_p(unet._handle), name.encode(), C.c_void_p(base.data_ptr()),
                                                            _lib.dtype_code(base), shape, base.ndim, len(hits), arr, C.c_void_p(st)), L)
        except Exception:
            # some keys may carry the new terms and others not: the native copy no longer matches any registry state, so the next
            # use uploads everything again and re-applies whatever the caller leaves attached
            unet._invalidate()
            raise
    # what the context cache, the SDXL embedding memo and the device-slot replicas compare; NOT _dirty: nothing else is re-uploaded
    unet._ctx_slots = []
    unet._weights_version = getattr(unet, "_weights_version", 0) + 1


def _reapply_attached(unet) -> None:
    """modules._NativeModule._sync, behind a full (dirty) upload: put the attached LoRAs onto the new native copy."""
    at = getattr(unet, "_lora_attached", None)
    if at and at["loras"]:
        _issue(unet, sorted({n for f, _ in at["loras"].values() for n in f.names()}))


def attach_lora(unet, tensors, lora_id, scale: float = 1.0) -> int:
    """Attach one LoRA (a dict of tensors, or the Factors upload_factors made of one) under ``lora_id`` on the device path:
    only the weights it touches are repacked, from the master parameter and the factors (module docstring).  Returns the number
    of weights touched.  The module must be on a GPU (GyreError otherwise, as for a forward)."""
    return attach_loras(unet, [(tensors, lora_id, scale)])[0]


def attach_loras(unet, specs) -> list:
    """Several LoRAs at once, ``specs = [(tensors or Factors, lora_id, scale), ...]``: all are registered first and every
    touched weight is repacked ONCE, with all the pairs that hit it.  Returns the number of weights each one touches.  An entry
    may also be the Factors of an uploaded LyCORIS file (lycoris.upload_factors; lycoris.attach_adapters routes mappings of
    either kind); a tensors mapping given here is read as a LoRA and a LyCORIS one is refused by detect_lora_type."""
    if (getattr(unet, "_lora_state", None) or {"loras": {}})["loras"]:
        raise ValueError("this module has host-merged LoRAs (apply_lora): the two LoRA paths do not stack - "
                         "remove_lora_from_model() first")
    is_factors = lambda t: isinstance(t, Factors)
    for tensors, _, _ in specs:                                # format errors come first
        if not is_factors(tensors) and detect_lora_type(tensors) == "cloneofsimo":
            raise NotImplementedError("cloneofsimo LoRA files need lora_diffusion's module search order (not vendored)")
    dev = unet.device
    unet._sync(dev)                                            # handle exists and holds the current weights (+ what is attached)
    new = [(t.to(dev) if is_factors(t) else upload_factors(unet, t, dev), lid, float(scale)) for t, lid, scale in specs]
    at = _attached(unet)
    before = dict(at["loras"])
    names = set()
    for factors, lid, scale in new:
        old = at["loras"].pop(lid, None)
        at["loras"][lid] = (factors, scale)
        names |= set(factors.names()) | (set(old[0].names()) if old else set())
    try:
        _issue(unet, sorted(names))
    except Exception:                                          # (_issue has left the native copy untouched, or marked it stale)
        at["loras"].clear()
        at["loras"].update(before)
        raise
    return [len(f.names()) for f, _, _ in new]


def set_attached_scale(unet, lora_id, scale: float = 1.0) -> None:
    at = _attached(unet)
    if lora_id not in at["loras"]:
        raise KeyError(lora_id)
    factors = at["loras"][lora_id][0]
    at["loras"][lora_id] = (factors, float(scale))
    _issue(unet, sorted(factors.names()))


def detach_loras(unet) -> None:
    """Take every attached LoRA off: the touched keys are re-issued with zero pairs, which writes the base bits."""
    at = getattr(unet, "_lora_attached", None)
    if not at or not at["loras"]:
        return
    names = sorted({n for f, _ in at["loras"].values() for n in f.names()})
    at["loras"].clear()
    _issue(unet, names)
