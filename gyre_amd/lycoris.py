"""LyCORIS (LoCon, LoHa, LoKr, full diff) for the native UNet: merged into the weights before they are repacked for the kernels.

The reference routes every ``lora=`` entry that ``detect_lora_type`` refuses to ``apply_lycoris`` (unified_pipeline.py:2210-2233,
gyre/pipeline/lycoris.py): a ``LycorisHook`` on every targeted nn.Linear / nn.Conv2d swaps ``weight + sum updown`` in for the
forward.  That is a map in weight space already, so here it joins the same two paths a LoRA takes (gyre_amd/lora.py): the host
merge (``apply_lycoris``, through lora's ``_lora_state`` registry - ``set_lora_scale`` / ``remove_lora_from_model`` cover it) and
the device path (``upload_factors`` + ``attach_lycoris`` / ``attach_adapters``), where the factors stay factors and each touched
weight is repacked once by the fused kernel of csrc/kernels_lyco.hip (``gyre_unet_set_weight_delta``).

Per module (keys grouped by the part before the first ``.``, prefix ``lora_unet_``, module path with ``_``) the delta is
``updown * file scale * user scale`` (lycoris.py:99-228 rebuild_weight, :267-285 _calc_updown), in file-tensor terms:
  LoCon  lora_up.weight, lora_down.weight [, lora_mid.weight]    up @ down  (the LoRA form), or with mid [r, r, KH, KW], up [O, r, 1, 1],
         down [r, I, 1, 1]:  D[o,i,k,l] = sum_{n,m} mid[n,m,k,l] up[o,n] down[m,i]
  LoHa   hada_w1_a/_b, hada_w2_a/_b [, hada_t1, hada_t2]           D = P1 * P2 element-wise;  P = wa [O, r] @ wb [r, I KH KW] in the
         weight's OIHW-flat order, or with t [r, r, KH, KW]:  P[o,i,k,l] = sum_{a,b} t[a,b,k,l] wa[a,o] wb[b,i]  (wa is [r, O] there)
  LoKr   lokr_w1 | lokr_w1_a/_b;  lokr_w2 | lokr_w2_a/_b | lokr_t2 + lokr_w2_a/_b
         D[o1 O2 + o2, i1 I2 + i2, k, l] = W1[o1, i1] W2[o2, i2, k, l],  W1 dense or w1a @ w1b, W2 dense, w2a @ w2b or the t form
  Full   diff                                                      D = diff
File scale: the ``scale`` key when present and non-zero, else ``alpha / dim`` when both exist, else 1; dim = down.shape[0] (LoCon),
wXb.shape[0] (LoHa, LoKr), none for Full (its alpha is ignored); a LoKr's alpha reads as absent when neither w1_a nor w2_a exists.
With two decomposed sides of different rank the reference's dim depends on the iteration order of a Python set: ValueError here.
IA3 (``weight`` / ``on_input``: the reference's own handler cannot run either, it stores ``.weight`` and reads ``.w``), DyLoRA
(``dyn_up`` / ``dyn_down``) and sparse bias (``bias_*``) are NotImplementedError at parse time.  ``lora_te_`` entries are ignored here (they are
gyre_amd/text_adapters.py's); another prefix is a ValueError, a ``lora_unet_`` key without a module a RuntimeError, as in the reference.

Deliberate deviation (the one lora.py makes): the reference adds each delta in the weight's own dtype; here base + sum of deltas
is summed in fp32 and rounded to the storage type once.

Device path: Tucker cores and a low-rank W1 are contracted once per upload with ``gyre_op_lyco_core`` (fp32), the ``wa`` of a t form
is transposed to [O, r] with a plain copy, nothing else is multiplied out.  One registry per UNet (lora._attached): a weight hit by
LoRA pairs and LyCORIS terms is repacked once with all of them in attach order, at most 8 per weight.
"""
from __future__ import annotations

import ctypes as C
from itertools import groupby
from typing import Dict, List, Mapping, Optional

import torch

from . import lora as LR
from .lora import Factors, Term

Tensor = torch.Tensor

_SCALARS = ("alpha", "scale")
_FIELDS = {"locon": ("lora_up.weight", "lora_down.weight", "lora_mid.weight"),
           "loha": ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b", "hada_t1", "hada_t2"),
           "lokr": ("lokr_w1", "lokr_w1_a", "lokr_w1_b", "lokr_w2", "lokr_w2_a", "lokr_w2_b", "lokr_t2"),
           "full": ("diff",)}
_BIAS = ("bias_indices", "bias_values", "bias_size")


def _kind(keys, where="") -> str:
    """The form of one module from its parameter keys, in the reference's order of tests (lycoris.py:477-538)."""
    keys = set(keys)
    if any(k.startswith("hada") for k in keys):
        kind = "loha"
    elif any(k.startswith("lokr") for k in keys):
        kind = "lokr"
    elif "weight" in keys:
        raise NotImplementedError(f"IA3 LyCORIS module {where}(weight / on_input): not supported (the reference cannot run it either)")
    elif "diff" in keys:
        kind = "full"
    else:
        kind = "locon"
    if keys & set(_BIAS):
        raise NotImplementedError(f"LyCORIS module {where}with a sparse bias (bias_indices / bias_values / bias_size): not supported")
    if keys & {"dyn_up", "dyn_down"}:
        raise NotImplementedError(f"DyLoRA LyCORIS module {where}(dyn_up / dyn_down): not supported")
    for k in keys:
        if k not in _FIELDS[kind] and k not in _SCALARS:
            raise ValueError(f"Don't know how to handle key {k} of the LyCORIS module {where}")
    need = {"locon": [("lora_up.weight",), ("lora_down.weight",)],
            "loha": [("hada_w1_a",), ("hada_w1_b",), ("hada_w2_a",), ("hada_w2_b",)],
            "lokr": [("lokr_w1", "lokr_w1_a"), ("lokr_w1", "lokr_w1_b"), ("lokr_w2", "lokr_w2_a"), ("lokr_w2", "lokr_w2_b")],
            "full": [("diff",)]}[kind]
    for alt in need:
        if not keys & set(alt):
            raise ValueError(f"LyCORIS module {where}({kind}) lacks {' or '.join(alt)}")
    return kind


def _modules(unet: torch.nn.Module, tensors) -> List[tuple]:
    """The key rules of apply_lycoris (lycoris.py:431-470): [(weight-parameter name, fields)] per targeted UNet weight, fields =
    {parameter key: tensor}.  ``tensors``: a dict of tensors, or a safetensors handle (keys() / get_tensor())."""
    get = tensors.get_tensor if hasattr(tensors, "get_tensor") else tensors.__getitem__
    flat = LR._flat_names(dict(unet.named_parameters()))
    out = []
    for module_key, keys in groupby(sorted(tensors.keys()), lambda key: key.split(".")[0]):
        keys = list(keys)
        if module_key.startswith("lora_te_"):
            continue
        if not module_key.startswith("lora_unet_"):
            raise ValueError(f"Unknown module key in Lycoris, don't know how to apply - {module_key}")
        mod = module_key[len("lora_unet_"):]
        if mod not in flat:
            raise RuntimeError(f"Couldn't find model for {module_key} when applying LoRA")
        if any("." not in k for k in keys):
            raise ValueError(f"Don't know how to handle key {module_key}")
        fields = {k.split(".", 1)[1]: get(k) for k in keys}
        _kind(fields, module_key + " ")
        out.append((flat[mod], fields))
    return out


def file_scale(fields: Mapping[str, Tensor]) -> float:
    """_calc_updown's scale without the user scale (module docstring)."""
    kind = _kind(fields)
    scale = fields.get("scale")
    if scale is not None and float(scale) != 0:
        return float(scale)
    alpha = fields.get("alpha")
    if kind == "locon":
        dims = [fields["lora_down.weight"].shape[0]]
    elif kind == "loha":
        dims = [fields["hada_w1_b"].shape[0], fields["hada_w2_b"].shape[0]]
    elif kind == "lokr":
        dims = [fields[k].shape[0] for k in ("lokr_w1_b", "lokr_w2_b") if k in fields]
        if "lokr_w1_a" not in fields and "lokr_w2_a" not in fields:
            alpha = None
    else:
        dims = []
    if alpha is None or not dims:
        return 1.0
    if len(set(dims)) > 1:
        raise ValueError(f"LyCORIS {kind} module with two decomposed sides of ranks {dims} and no scale key: alpha / dim is ambiguous")
    return float(alpha) / dims[0]


def _f32(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32)


def _flat2(t: Tensor) -> Tensor:
    return t.reshape(t.shape[0], -1)


def _cp(t, wa, wb):
    """make_weight_cp: P[o,i,k,l] = sum_{a,b} t[a,b,k,l] wa[a,o] wb[b,i]"""
    if t.ndim != 4 or wa.ndim != 2 or wb.ndim != 2 or wa.shape[0] != t.shape[0] or wb.shape[0] != t.shape[1]:
        raise ValueError(f"LyCORIS Tucker form: t {tuple(t.shape)}, wa {tuple(wa.shape)}, wb {tuple(wb.shape)} do not fit")
    return torch.einsum("abkl,ao,bi->oikl", t, wa, wb)


def _mm(a, b):
    a, b = _flat2(a), _flat2(b)
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"LyCORIS factors {tuple(a.shape)} x {tuple(b.shape)} do not multiply")
    return a @ b


def lyco_delta(fields: Mapping[str, Tensor], shape) -> Tensor:
    """The weight-space image of one module's tensors (``fields``: parameter key -> tensor, alpha / scale included) for a weight of
    ``shape``, with the file scale and without the user scale (fp32): the host counterpart of lora.lora_delta."""
    kind = _kind(fields)
    f = {k: _f32(v) for k, v in fields.items() if k not in _SCALARS}
    if kind == "locon":
        up, down, mid = f["lora_up.weight"], f["lora_down.weight"], f.get("lora_mid.weight")
        if mid is not None:
            up2, down2 = _flat2(up), _flat2(down)
            if mid.ndim != 4 or up2.shape[1] != mid.shape[0] or down2.shape[0] != mid.shape[1]:
                raise ValueError(f"LoCon: up {tuple(up.shape)}, mid {tuple(mid.shape)}, down {tuple(down.shape)} do not fit")
            d = torch.einsum("nmkl,in,mj->ijkl", mid, up2, down2)
        else:
            d = _mm(up, down)
    elif kind == "loha":
        def prod(wa, wb, t):
            return _cp(t, wa, wb) if t is not None else _mm(wa, wb)
        p1 = prod(f["hada_w1_a"], f["hada_w1_b"], f.get("hada_t1"))
        p2 = prod(f["hada_w2_a"], f["hada_w2_b"], f.get("hada_t2"))
        if p1.numel() != p2.numel():
            raise ValueError(f"LoHa: the two products have shapes {tuple(p1.shape)} and {tuple(p2.shape)}")
        d = p1.reshape(-1) * p2.reshape(-1)
    elif kind == "lokr":
        w1 = f["lokr_w1"] if "lokr_w1" in f else _mm(f["lokr_w1_a"], f["lokr_w1_b"])
        if "lokr_w2" in f:
            w2 = f["lokr_w2"]
        elif "lokr_t2" in f:
            w2 = _cp(f["lokr_t2"], f["lokr_w2_a"], f["lokr_w2_b"])
        else:
            w2 = _mm(f["lokr_w2_a"], f["lokr_w2_b"])
        if w1.ndim != 2:
            raise ValueError(f"LoKr: w1 must be a matrix, got {tuple(w1.shape)}")
        kk = 1
        for n in tuple(shape)[2:]:
            kk *= n
        w2 = w2.reshape(w2.shape[0], -1, kk)                              # [O2, I2, KK]: a 2-d w2 is OIHW-flat (I2 KK columns)
        d = torch.einsum("ab,cdk->acbdk", w1, w2)                         # [O1, O2, I1, I2, KK]
        if (w1.shape[0] * w2.shape[0], w1.shape[1] * w2.shape[1]) != tuple(shape)[:2]:
            raise ValueError(f"LoKr: w1 {tuple(w1.shape)} x w2 {tuple(w2.shape[:2])} does not give the weight's shape {tuple(shape)}")
    else:
        d = f["diff"]
    n = 1
    for s in shape:
        n *= s
    if d.numel() != n:
        raise ValueError(f"LyCORIS {kind} delta has {d.numel()} elements, the weight {tuple(shape)} has {n}")
    return d.reshape(tuple(shape)) * file_scale(fields)


def _targets(unet, tensors) -> Dict[str, Tensor]:
    params = dict(unet.named_parameters())
    return {name: lyco_delta(fields, params[name].shape) for name, fields in _modules(unet, tensors)}


@torch.no_grad()
def apply_lycoris(unet, tensors, lyco_id, scale: float = 1.0) -> int:
    """Host merge of one LyCORIS file under ``lyco_id`` through lora's registry (lora.set_lora_scale / remove_lora_from_model then
    cover it).  Returns the number of weights touched."""
    LR._refuse_attached(unet)
    return LR._merge(unet, _targets(unet, tensors), lyco_id, scale)


# ---- device path ---------------------------------------------------------------------------------------------------------
def _core(L, core: Tensor, right: Tensor) -> Tensor:
    """gyre_op_lyco_core: core [A, B, T...] x right [B, C] -> fp32 [A, C, T]."""
    from . import _lib
    A, B = core.shape[0], core.shape[1]
    T = core[0, 0].numel()
    if right.ndim != 2 or right.shape[0] != B:
        raise ValueError(f"LyCORIS: core {tuple(core.shape)} and factor {tuple(right.shape)} do not contract")
    out = torch.empty((A, right.shape[1], T), dtype=torch.float32, device=core.device)
    with torch.cuda.device(core.device):
        _lib.check(L.gyre_op_lyco_core(C.c_void_p(_lib.stream_ptr(core.device)), C.c_void_p(core.data_ptr()), _lib.dtype_code(core),
                                       C.c_void_p(right.data_ptr()), _lib.dtype_code(right), A, B, right.shape[1], T,
                                       C.c_void_p(out.data_ptr())), L)
    return out


def make_term(L, fields: Mapping[str, Tensor], w: Tensor, name: str, device) -> Term:
    """The Term of one module's file tensors for the weight ``w`` (its shape only), operands on ``device`` in their own dtype.
    Tucker cores and a low-rank W1 are contracted here (gyre_op_lyco_core of the library ``L``, fp32); nothing else is multiplied
    out.  ValueError where the tensors do not give the weight's shape.  Shared by upload_factors and text_adapters."""
    from . import _lib
    fix = lambda t: LR.fix_factor(t, device)

    def product(wa, wb, t):
        """(up [O', r], down [r, ...]) of one low-rank product; with a core: up = wa^T in fp32, down = core(t, wb)."""
        if t is None:
            wa, wb = fix(wa), fix(wb)
            wa = wa.reshape(wa.shape[0], -1)
            if wa.dtype != wb.dtype:
                wa, wb = wa.float(), wb.float()
            return wa.contiguous(), wb
        t, wa, wb = fix(t), fix(wa), fix(wb)
        if t.ndim != 4 or wa.ndim != 2 or wb.ndim != 2 or wa.shape[0] != t.shape[0] or wb.shape[0] != t.shape[1]:
            raise ValueError(f"LyCORIS for {name}: t {tuple(t.shape)}, wa {tuple(wa.shape)}, wb {tuple(wb.shape)} do not fit")
        return wa.float().t().contiguous(), _core(L, t, wb)

    kind, scale = _kind(fields), file_scale(fields)
    if kind == "locon":
        up, down, mid = fields["lora_up.weight"], fields["lora_down.weight"], fields.get("lora_mid.weight")
        if mid is None:
            term = Term(_lib.DELTA_LORA, [product(up, down, None)], scale)
        else:
            mid, up, down = fix(mid), fix(up), fix(down)
            up, down = up.reshape(up.shape[0], -1), down.reshape(down.shape[0], -1)
            if mid.ndim != 4 or up.shape[1] != mid.shape[0] or down.shape[0] != mid.shape[1]:
                raise ValueError(f"LoCon for {name}: up {tuple(up.shape)}, mid {tuple(mid.shape)}, down {tuple(down.shape)} do not fit")
            term = Term(_lib.DELTA_LORA, [(up.float().contiguous(), _core(L, mid, down.contiguous()))], scale)
    elif kind == "loha":
        term = Term(_lib.DELTA_HADA, [product(fields["hada_w1_a"], fields["hada_w1_b"], fields.get("hada_t1")),
                                      product(fields["hada_w2_a"], fields["hada_w2_b"], fields.get("hada_t2"))], scale)
    elif kind == "lokr":
        if "lokr_w1" in fields:
            w1 = fix(fields["lokr_w1"]).float().contiguous()
        else:
            a, b = fix(fields["lokr_w1_a"]), fix(fields["lokr_w1_b"])
            if a.ndim != 2 or b.ndim != 2:
                raise ValueError(f"LoKr for {name}: w1_a / w1_b must be matrices")
            w1 = _core(L, a, b).reshape(a.shape[0], b.shape[1])
        if "lokr_w2" in fields:
            op = (None, fix(fields["lokr_w2"]))
        else:
            op = product(fields["lokr_w2_a"], fields["lokr_w2_b"], fields.get("lokr_t2"))
        term = Term(_lib.DELTA_KRON, [op], scale, w1)
    else:
        term = Term(_lib.DELTA_FULL, [(None, fix(fields["diff"]))], scale)
    if w.ndim not in (2, 4) or not term.fits(w):
        raise ValueError(f"LyCORIS {kind} module for {name}: its tensors do not give the weight's shape {tuple(w.shape)}")
    return term


def upload_factors(unet, tensors, device=None) -> Factors:
    """Parse ``tensors`` (the key rules of apply_lycoris) and put its terms on ``device`` (default: the module's), each factor in its own
    dtype.  Tucker cores and a low-rank W1 are contracted once here (gyre_op_lyco_core, fp32); nothing else is multiplied out.
    Shapes are checked against the weights they target (ValueError)."""
    from . import _lib
    device = torch.device(device) if device is not None else unet.device
    if device.type != "cuda":
        raise _lib.GyreError("LyCORIS factors are prepared on the GPU (gyre_op_lyco_core): the native path has no CPU fallback")
    L = unet._L() if hasattr(unet, "_L") else _lib.lib()
    params = dict(unet.named_parameters())
    terms = {name: make_term(L, fields, params[name], name, device) for name, fields in _modules(unet, tensors)}
    return Factors(terms, device, tensors)


def is_lycoris(tensors) -> bool:
    """The reference's routing (unified_pipeline.py:2212-2216): what detect_lora_type refuses with a ValueError goes to the LyCORIS
    parser."""
    try:
        LR.detect_lora_type(tensors)
        return False
    except ValueError:
        return True


def factors_for(unet, tensors, device=None):
    """lora.upload_factors or this module's, by that routing."""
    if isinstance(tensors, Factors):
        return tensors
    return upload_factors(unet, tensors, device) if is_lycoris(tensors) else LR.upload_factors(unet, tensors, device)


def attach_adapters(unet, specs) -> list:
    """``specs = [(tensors | Factors, id, scale), ...]``, LoRA and LyCORIS files mixed: all are registered first
    and every touched weight is repacked ONCE with every pair / term that hits it, in attach order (lora.attach_loras)."""
    specs = list(specs)
    for t, _, _ in specs:                                           # format errors come first, before any upload
        if not isinstance(t, Factors) and not is_lycoris(t) and LR.detect_lora_type(t) == "cloneofsimo":
            raise NotImplementedError("cloneofsimo LoRA files need lora_diffusion's module search order (not vendored)")
    if specs:
        unet._sync(unet.device)                                     # raises off the GPU, before factors_for would
    return LR.attach_loras(unet, [(factors_for(unet, t, unet.device), lid, scale) for t, lid, scale in specs])


def attach_lycoris(unet, tensors, lyco_id, scale: float = 1.0) -> int:
    """Attach one LyCORIS file (a dict of tensors, a safetensors handle, or the Factors upload_factors made of one) on the
    device path.  Returns the number of weights touched."""
    if not isinstance(tensors, Factors):
        unet._sync(unet.device)
        tensors = upload_factors(unet, tensors, unet.device)
    return LR.attach_loras(unet, [(tensors, lyco_id, scale)])[0]
