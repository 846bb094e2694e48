"""Per-request adapters of the TEXT ENCODER: the ``lora_te_`` half of a LoRA / LyCORIS file and textual-inversion embeddings.

The text encoder stays the host PyTorch module the manager loaded; what changes per request is its weights (and its token table).

LoRA / LyCORIS.  The reference hooks the same file it hooks onto the UNet onto the text encoder (gyre/pipeline/lora.py:269-330
apply_kohya_to_pipe, lycoris.py:431-445 apply_lycoris) and scales it by the ``"text_encoder"`` / ``"*"`` entries of the request's
weights (unified_pipeline.py:2210-2233).  Here the same linear map is merged into the weight, as gyre_amd/lora.py and lycoris.py do for
the UNet - with the one deviation they make: base + sum of deltas is summed in fp32 and rounded to the encoder's dtype ONCE (a 16-bit
master must not accumulate deltas: an element below half an ulp of W would vanish, lora.py's own note).
  * keys: ``lora_te_<module path with _>`` resolved by the reference's greedy attribute walk (lora.py:306-316): of
    ``text_model_encoder_layers_0_mlp_fc1`` the longest prefix that is an attribute wins, so it reaches
    ``text_model.encoder.layers[0].mlp.fc1``.  A CLIPTextModel that holds its tower directly (transformers 5 dropped the ``text_model``
    wrapper) takes a leading ``text_model`` as itself.  A key that resolves to nothing: the reference's RuntimeError; a target that is
    not an nn.Linear (CLIP has no other): its ValueError.  diffusers-format files carry no text side (as in the reference); cloneofsimo
    files and the embeddings packed inside them stay unsupported (lora.py).
  * terms: built by the parsers of the UNet side, not by copies of them - lycoris._kind / file_scale / make_term (Term, _core) and
    lora.lora_term for a kohya LoRA pair; IA3, DyLoRA and sparse-bias modules are NotImplementedError exactly as there.  A module whose
    tensors are ALL zero is the zero delta whatever its shapes and is skipped before any shape rule (placeholders).
  * native path (the default wherever the encoder is on a GPU): ``upload_text_factors`` puts the factors on the device once per file,
    ``attach`` keeps each touched weight's original tensor as ``base`` (its own dtype) and issues ONE gyre_op_merge_delta per weight
    with all terms of all files of the request, written into the live parameter's storage (csrc/kernels_lyco.hip k_merge_delta: the
    arithmetic of the UNet's repack, row-major, rounded to fp32 / bf16 / fp16 as the encoder is).  More than 8 terms on one weight is
    a ValueError.  ``detach`` issues the same call with zero terms, which restores every touched weight bit for bit.
  * host path (an encoder that is not on a GPU): the weight-space merge through lora.lora_delta / lycoris.lyco_delta, summed in
    fp32 (float64 for a float64 encoder) and rounded once; ``detach`` copies the kept tensor back.
  * scale: what the reference's loop leaves on the text encoder - the request's ``weights`` walked in order, ``"*"`` and
    ``"text_encoder"`` set it, default 1.0 (``text_scale``).

Textual inversion (gyre/pipeline/textual_inversion.py, unified_pipeline.py:1847-1868, 2190-2206): ``apply_ti_to_tokenizer`` on a
per-request deepcopy of the tokenizer (a 1-D tensor is one token; a 2-D [n, dim] tensor becomes the sub-tokens ``<name00>`` ... and
a text replacement of ``<name>`` by their space-joined list, ``replace_text``), ``apply_ti_to_encoder`` resizes the token table to
``len(tokenizer)`` and writes the rows in the table's dtype, ``match_encoder_to_tokenizer`` at the start of every request shrinks
it back.  The tokenizer contract is what these call: ``add_tokens``, ``convert_tokens_to_ids``, ``__len__`` (and ``encode`` or
``__call__`` for the engine's tokenize closure, which applies ``replace_text`` first so that long-prompt weighting sees the
sub-tokens).  A vector whose length is not the encoder's embedding dim is a ValueError before anything changed (``check_ti``).
"""
from __future__ import annotations

import ctypes as C
from itertools import groupby
from typing import List, Mapping, Optional

import torch

from . import lora as LR
from . import lycoris as LY

Tensor = torch.Tensor
MAX_TERMS = 8
_STATE = "_gyre_text_adapters"


# ---- LoRA / LyCORIS ----------------------------------------------------------------------------------------------------------
def has_text_keys(tensors) -> bool:
    return any(k.startswith("lora_te_") for k in tensors.keys())


def text_scale(weights) -> float:
    """The scale the reference's loop (unified_pipeline.py:2221-2233) leaves on the text encoder."""
    scale = 1.0
    if isinstance(weights, dict):
        for key, weight in weights.items():
            if key in ("*", "text_encoder"):
                scale = weight
    return float(scale)


def resolve(text_encoder, module_key: str):
    """``lora_te_<name>`` -> the module, by the reference's greedy attribute walk (lora.py:306-316, lycoris.py:458-470)."""
    parts = module_key[len("lora_te_"):].split("_")
    module = text_encoder
    while parts:
        for n in range(len(parts), 0, -1):
            child = getattr(module, "_".join(parts[:n]), False)
            if child:
                module, parts = child, parts[n:]
                break
        else:
            if module is text_encoder and parts[:2] == ["text", "model"]:       # the tower itself (module docstring)
                parts = parts[2:]
                continue
            raise RuntimeError(f"Couldn't find model for {module_key} when applying LoRA")
    return module


def _all_zero(fields: Mapping[str, Tensor]) -> bool:
    return all(not bool(torch.as_tensor(t).any()) for k, t in fields.items() if k not in LY._SCALARS)


def text_modules(text_encoder, tensors) -> List[tuple]:
    """[(module key, nn.Linear, fields, is_lycoris)] per targeted text-encoder module; fields = {parameter key: tensor} as lycoris._modules
    gives them (a kohya LoRA module: lora_up.weight, lora_down.weight and alpha when present)."""
    if not has_text_keys(tensors):
        return []
    get = tensors.get_tensor if hasattr(tensors, "get_tensor") else tensors.__getitem__
    lyco = LY.is_lycoris(tensors)
    found = []
    if lyco:
        for module_key, keys in groupby(sorted(tensors.keys()), lambda key: key.split(".")[0]):
            keys = list(keys)
            if not module_key.startswith("lora_te_"):
                continue                                                  # lora_unet_ and unknown prefixes: lycoris._modules' business
            if any("." not in k for k in keys):
                raise ValueError(f"Don't know how to handle key {module_key}")
            found.append((module_key, {k.split(".", 1)[1]: get(k) for k in keys}))
    elif LR.detect_lora_type(tensors) == "kohya-ss":                      # diffusers: UNet only; cloneofsimo: refused by the UNet side
        for key in tensors.keys():
            if not key.endswith(".lora_down.weight") or not key.startswith("lora_te_"):
                continue
            fields = {"lora_down.weight": get(key), "lora_up.weight": get(key.replace(".lora_down.", ".lora_up."))}
            alpha = key.replace(".lora_down.weight", ".alpha")
            if alpha in tensors.keys():
                fields["alpha"] = get(alpha)
            found.append((key.split(".")[0], fields))
    out = []
    for module_key, fields in found:
        module = resolve(text_encoder, module_key)
        if not isinstance(module, torch.nn.Linear):
            raise ValueError(f"Can't apply {'Lycoris' if lyco else 'LoRA'} to module of type {type(module).__name__}")
        if _all_zero(fields):
            continue
        LY._kind(fields, module_key + " ")                                # IA3 / DyLoRA / sparse bias: NotImplementedError, as for the UNet
        out.append((module_key, module, fields, lyco))
    return out


class TextFactors:
    """One file's text-encoder side for ONE encoder object: ``terms = [(nn.Linear, lycoris.Term)]`` with the operands on ``device``
    (native path), or ``deltas = [(nn.Linear, fp32 delta with the file scale)]`` (host path).  ``source`` keeps the mapping referenced
    (an identity-keyed cache must not see its key's address recycled)."""

    def __init__(self, terms, deltas, device, source=None):
        self.terms, self.deltas, self.device, self.source = terms, deltas, device, source

    def __len__(self):
        return len(self.terms if self.terms is not None else self.deltas)


def _device_of(text_encoder) -> torch.device:
    if isinstance(text_encoder, torch.nn.Module):
        for p in text_encoder.parameters():
            return p.device
    return torch.device("cpu")


def upload_text_factors(text_encoder, tensors, device=None) -> TextFactors:
    """Parse the ``lora_te_`` side of ``tensors`` against ``text_encoder`` and prepare it for ``device`` (default: the encoder's):
    on a GPU the factors stay factors (each in its own dtype; Tucker cores and a low-rank W1 contracted once, gyre_op_lyco_core), off
    it every module is multiplied out (lora_delta / lyco_delta).  Shapes are checked against the weights they target (ValueError)."""
    device = torch.device(device) if device is not None else _device_of(text_encoder)
    mods = text_modules(text_encoder, tensors)
    if device.type != "cuda":
        deltas = []
        for key, module, fields, lyco in mods:
            w = module.weight
            d = LY.lyco_delta(fields, w.shape) if lyco else LR.lora_delta(fields["lora_up.weight"], fields["lora_down.weight"], fields.get("alpha"))
            if tuple(d.shape) != tuple(w.shape):
                raise ValueError(f"LoRA for {key}: the delta has shape {tuple(d.shape)}, the weight {tuple(w.shape)}")
            deltas.append((module, d))
        return TextFactors(None, deltas, device, tensors)
    from . import _lib
    L = _lib.lib()
    with torch.cuda.device(device):
        terms = [(module, LY.make_term(L, fields, module.weight, key, device) if lyco else
                  LR.lora_term(fields["lora_up.weight"], fields["lora_down.weight"], fields.get("alpha"), module.weight, key, device))
                 for key, module, fields, lyco in mods]
    return TextFactors(terms, None, device, tensors)


def _state(text_encoder) -> dict:
    st = getattr(text_encoder, _STATE, None)
    if st is None:
        st = {}                                            # nn.Linear -> its original weight tensor (own dtype, own device)
        setattr(text_encoder, _STATE, st)
    return st


def _merge_call(L, base: Tensor, hits, out: Tensor) -> None:
    from . import _lib
    arr = (_lib.DeltaTerm * max(len(hits), 1))()
    for j, (term, scale) in enumerate(hits):
        term.fill(arr[j], scale)
    O, I = base.shape
    _lib.check(L.gyre_op_merge_delta(C.c_void_p(_lib.stream_ptr(base.device)), C.c_void_p(base.data_ptr()), _lib.dtype_code(base), O, I,
                                     len(hits), arr, C.c_void_p(out.data_ptr()), _lib.dtype_code(out)), L)


@torch.no_grad()
def attach(text_encoder, specs) -> int:
    """``specs = [(TextFactors, user scale), ...]``: all files of one request.  Every touched weight is written ONCE, from its kept
    original and every term that hits it in spec order.  Returns the number of weights touched.  Whatever a previous attach left is
    taken off first."""
    detach(text_encoder)
    specs = [(f, float(s)) for f, s in specs if len(f) and float(s) != 0]         # (scale 0 contributes nothing, as in lora._issue)
    if not specs:
        return 0
    st = _state(text_encoder)
    native = specs[0][0].terms is not None
    if any((f.terms is not None) != native for f, _ in specs):
        raise ValueError("text-encoder factors prepared for a GPU and for the host in one request")
    plan: dict = {}
    for f, scale in specs:
        for module, hit in (f.terms if native else f.deltas):
            plan.setdefault(module, []).append((hit, scale))
    # everything is checked before the first write: the kernel trusts these shapes
    for module, hits in plan.items():
        w = module.weight
        if len(hits) > MAX_TERMS:
            raise ValueError(f"{len(hits)} LoRA / LyCORIS terms hit one text-encoder weight {tuple(w.shape)}: at most {MAX_TERMS} per weight")
        if native:
            if not w.is_cuda or w.ndim != 2 or not w.is_contiguous() or w.shape[1] % 4 or w.dtype not in LR._FACTOR_DTYPES:
                raise ValueError(f"text-encoder weight {tuple(w.shape)} {w.dtype} on {w.device}: the native merge needs a contiguous fp32 / bf16 / "
                                 "fp16 matrix on the GPU with a multiple of 4 columns")
            for term, _ in hits:
                if any(t.device != w.device for t in term.tensors()) or not term.fits(w):
                    raise ValueError(f"text-encoder term does not fit its weight {tuple(w.shape)} on {w.device} (factors uploaded for another model?)")
        elif any(tuple(d.shape) != tuple(w.shape) for d, _ in hits):
            raise ValueError(f"text-encoder delta does not fit its weight {tuple(w.shape)} (factors prepared for another model?)")
    try:
        if native:
            from . import _lib
            L = _lib.lib()
            dev = next(iter(plan)).weight.device
            with torch.cuda.device(dev):
                for module, hits in plan.items():
                    w = module.weight.data
                    st[module] = w.clone()                                  # out must not alias base: the caller keeps the original
                    _merge_call(L, st[module], hits, w)
        else:
            for module, hits in plan.items():
                w = module.weight.data
                st[module] = w.clone()
                acc = st[module].to(torch.float64 if w.dtype == torch.float64 else torch.float32)
                for d, scale in hits:
                    acc = acc + d.to(acc.device, acc.dtype) * scale
                w.copy_(acc.to(w.dtype))
    except Exception:
        detach(text_encoder)
        raise
    return len(plan)


@torch.no_grad()
def detach(text_encoder) -> None:
    """Restore every weight the last attach touched, bit for bit (GPU: gyre_op_merge_delta with zero terms; host: a copy)."""
    st = getattr(text_encoder, _STATE, None)
    if not st:
        return
    for module, base in list(st.items()):
        w = module.weight.data
        if w.shape != base.shape or w.dtype != base.dtype or w.device != base.device:
            continue                                       # the encoder was moved or reloaded since: nothing of ours is in that tensor
        if w.is_cuda and w.ndim == 2 and w.is_contiguous() and w.shape[1] % 4 == 0 and w.dtype in LR._FACTOR_DTYPES:
            from . import _lib
            with torch.cuda.device(w.device):
                _merge_call(_lib.lib(), base, [], w)
        else:
            w.copy_(base)
    st.clear()


# ---- textual inversion -------------------------------------------------------------------------------------------------------
def replace_text(tokenizer, text):
    """The multi-vector replacement of textual_inversion.py:57-66: every ``<name>`` of a 2-D embedding by its sub-token list."""
    if isinstance(text, list):
        return [replace_text(tokenizer, t) for t in text]
    for token, replacement in getattr(tokenizer, "_multidim_mappings", {}).items():
        text = text.replace(token, replacement)
    return text


def embedding_dim(text_encoder) -> int:
    return text_encoder.get_input_embeddings().weight.shape[1]


def check_ti(text_encoder, tensors: Mapping[str, Tensor]) -> None:
    """ValueError for an embedding that is not a vector or a matrix of the encoder's embedding dim - before anything is changed."""
    dim = embedding_dim(text_encoder)
    for token, tensor in tensors.items():
        if tensor.ndim not in (1, 2) or tensor.shape[-1] != dim:
            raise ValueError(f"token embedding {token!r} has shape {tuple(tensor.shape)}; the text encoder's embedding dim is {dim}")


def apply_ti_to_tokenizer(tokenizer, tensors: Mapping[str, Tensor]) -> dict:
    """textual_inversion.py:88-116 on a tokenizer that meets the contract of the module docstring: returns {token: vector}."""
    flattened = {}
    for token, tensor in tensors.items():
        if len(tensor.shape) == 2:
            if not hasattr(tokenizer, "_multidim_mappings"):
                tokenizer._multidim_mappings = {}
            subbase = token.lstrip("<").rstrip(">")
            subtokens = [f"<{subbase}{i:02x}>" for i in range(0, tensor.shape[0])]
            for i, subtoken in enumerate(subtokens):
                flattened[subtoken] = tensor[i]
            tokenizer._multidim_mappings[token] = " ".join(subtokens)
        else:
            flattened[token] = tensor
    tokenizer.add_tokens(list(flattened.keys()))            # (a list: a str would be one token; overlap with known tokens is fine)
    return flattened


def _resize(text_encoder, n: int):
    import inspect
    fn = text_encoder.resize_token_embeddings
    try:
        plain = "mean_resizing" in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        plain = False
    # (newer transformers initialise added rows from the table's mean and covariance: every added row is overwritten here)
    return fn(n, mean_resizing=False) if plain else fn(n)


@torch.no_grad()
def apply_ti_to_encoder(tokenizer, text_encoder, flattened: Mapping[str, Tensor]) -> None:
    """textual_inversion.py:119-150 without its offload hooks: the table grows to len(tokenizer), the rows are written in its dtype."""
    new_embedding = _resize(text_encoder, len(tokenizer))
    weight = (new_embedding if new_embedding is not None else text_encoder.get_input_embeddings()).weight
    for token, tensor in flattened.items():
        weight.data[tokenizer.convert_tokens_to_ids(token)] = tensor.to(weight.device, weight.dtype)


@torch.no_grad()
def match_encoder_to_tokenizer(tokenizer, text_encoder) -> None:
    """textual_inversion.py:153-169: the table back to the tokenizer's own length (what a previous request's embeddings added goes).
    A bare callable tokenizer (no ``__len__``) can never have had tokens added: nothing to do."""
    if not hasattr(tokenizer, "__len__") or not hasattr(text_encoder, "resize_token_embeddings"):
        return
    n = len(tokenizer)
    if text_encoder.get_input_embeddings().weight.shape[0] != n:
        _resize(text_encoder, n)
