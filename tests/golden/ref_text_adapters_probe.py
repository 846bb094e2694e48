"""Runs the REFERENCE's own text-encoder adapter functions (/root/reference: gyre/pipeline/textual_inversion.py, lora.py, lycoris.py)
and gyre_amd/text_adapters.py over the same tiny CLIP text encoder and stub tokenizer, and prints what tests/
test_reference_text_adapters.py compares as one ``PROBE_JSON`` line.  Build container only.  The un-vendored
gyre.src.lora.lora_diffusion.lora import of lora.py is stubbed (its three names are not used by the kohya path)."""
import copy
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), "/root/reference"]

import text_adapter_util as U  # noqa: E402
from gyre_amd import text_adapters as TA  # noqa: E402

out = {}


def ref_import(name):
    try:
        return __import__(name, fromlist=["x"])
    except Exception as e:  # noqa: BLE001
        out.setdefault("import_errors", {})[name] = f"{type(e).__name__}: {e}"
        return None


for n in ("gyre.src", "gyre.src.lora", "gyre.src.lora.lora_diffusion"):
    sys.modules.setdefault(n, types.ModuleType(n))
stub = types.ModuleType("gyre.src.lora.lora_diffusion.lora")
stub._find_modules = stub.parse_safeloras = stub.parse_safeloras_embeds = None
sys.modules["gyre.src.lora.lora_diffusion.lora"] = stub
RTI, RLO, RLY = (ref_import(f"gyre.pipeline.{m}") for m in ("textual_inversion", "lora", "lycoris"))


class Nested(torch.nn.Module):
    """The layout the reference's keys address (transformers 4): the tower under ``.text_model``."""

    def __init__(self, te):
        super().__init__()
        self.text_model = U.tower(te)


class Handle:
    """keys() / get_tensor(): what apply_lycoris reads a file through."""

    def __init__(self, d):
        self.d = d

    def keys(self):
        return self.d.keys()

    def get_tensor(self, k):
        return self.d[k]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- textual inversion -----------------------------------------------------------------------------------------------------------
if RTI is not None:
    g = torch.Generator().manual_seed(3)
    ti = {"<cat>": torch.randn(32, generator=g), "<style>": torch.randn(3, 32, generator=g)}
    prompt = "a photo of <cat> by <style> please"
    for dt in ("float32", "bfloat16"):
        dtype = getattr(torch, dt)
        te_r, te_m = U.tiny_encoder(dtype=dtype), U.tiny_encoder(dtype=dtype)
        base_tok = U.StubTokenizer(128)
        tok_r, tok_m = copy.deepcopy(base_tok), copy.deepcopy(base_tok)
        flat_r = RTI.apply_ti_to_tokenizer(tok_r, ti)
        flat_m = TA.apply_ti_to_tokenizer(tok_m, ti)
        RTI.apply_ti_to_encoder(tok_r, te_r, flat_r)
        TA.apply_ti_to_encoder(tok_m, te_m, flat_m)
        wr, wm = te_r.get_input_embeddings().weight, te_m.get_input_embeddings().weight
        c = {"flattened_keys_equal": list(flat_r) == list(flat_m),
             "flattened_values_equal": all(torch.equal(flat_r[k], flat_m[k]) for k in flat_r),
             "token_ids_equal": [tok_r.convert_tokens_to_ids(k) for k in flat_r] == [tok_m.convert_tokens_to_ids(k) for k in flat_m],
             "mappings_equal": tok_r._multidim_mappings == tok_m._multidim_mappings, "len": [len(tok_r), len(tok_m)],
             "prompt_ids_ref": tok_r.encode(prompt)[1:-1],                       # the reference's patched encode replaces the text itself
             "prompt_ids_mine": tok_m(TA.replace_text(tok_m, prompt))["input_ids"],
             "table_shape": [list(wr.shape), list(wm.shape)], "table_dtype": [str(wr.dtype), str(wm.dtype)],
             "added_rows_equal": bool(torch.equal(wr[128:], wm[128:])), "old_rows_equal": bool(torch.equal(wr[:128], wm[:128])),
             "rows_are_the_vectors": bool(torch.equal(wm[128], ti["<cat>"].to(dtype)) and torch.equal(wm[129:132], ti["<style>"].to(dtype)))}
        ids = torch.tensor([[126] + c["prompt_ids_mine"] + [127] * (76 - len(c["prompt_ids_mine"]))])
        c["encoded_equal"] = bool(torch.equal(U.encode(te_r, ids), U.encode(te_m, ids)))
        RTI.match_encoder_to_tokenizer(base_tok, te_r)
        TA.match_encoder_to_tokenizer(base_tok, te_m)
        wr, wm = te_r.get_input_embeddings().weight, te_m.get_input_embeddings().weight
        c["shrunk_shape"] = [list(wr.shape), list(wm.shape)]
        c["shrunk_equal"] = bool(torch.equal(wr, wm))
        out[f"ti_{dt}"] = c

# ---- lora_te_ entries: the reference's hooks against the merged weights, float64 ----------------------------------------------------
ids = U.ids_batch(128)
with torch.no_grad():
    for form, mod in (("lora", RLO), ("loha", RLY), ("lokr_lowrank", RLY), ("lokr_dense", RLY), ("full", RLY)):
        if mod is None:
            continue
        te_r, te_m = U.tiny_encoder(dtype=torch.float64), U.tiny_encoder(dtype=torch.float64)
        base = U.encode(te_m, ids)
        tensors = U.te_file(te_m, form, shrink=2.0 ** -2)
        for name, weights in (("default", {}), ("text_encoder", {"unet": 3.0, "text_encoder": 0.75}), ("star_last", {"text_encoder": 0.75, "*": 0.5})):
            nested = Nested(te_r)
            if mod is RLO:
                RLO.apply_kohya_to_pipe(tensors, 0, unet=None, text_encoder=nested)
                set_scale, remove = RLO.set_lora_scale, RLO.remove_lora_from_model
            else:
                RLY.apply_lycoris(Handle(tensors), 0, unet=None, text_encoder=nested)
                set_scale, remove = RLY.set_lycoris_scale, RLY.remove_lycoris_from_model
            for key, weight in weights.items():                                # unified_pipeline.py:2221-2233
                if key in ("*", "text_encoder"):
                    set_scale(nested, 0, weight)
            want = U.encode(te_r, ids)
            remove(nested)
            TA.attach(te_m, [(TA.upload_text_factors(te_m, tensors), TA.text_scale(weights))])
            got = U.encode(te_m, ids)
            TA.detach(te_m)
            out[f"{form}_{name}"] = {"rel_l2": rel_l2(got, want), "effect": rel_l2(want, base),
                                     "restored": bool(torch.equal(U.encode(te_m, ids), base) and torch.equal(U.encode(te_r, ids), base))}
        # the unknown-key error is the reference's
        bad = {k.replace("mlp_fc1", "mlp_fc9"): v for k, v in tensors.items()}
        errs = []
        for fn in ((lambda: RLO.apply_kohya_to_pipe(bad, 1, unet=None, text_encoder=Nested(te_r))) if mod is RLO else
                   (lambda: RLY.apply_lycoris(Handle(bad), 1, unet=None, text_encoder=Nested(te_r))), lambda: TA.upload_text_factors(te_m, bad)):
            try:
                fn()
                errs.append(None)
            except Exception as e:  # noqa: BLE001
                errs.append([type(e).__name__, str(e)])
        (RLO.remove_lora_from_model if mod is RLO else RLY.remove_lycoris_from_model)(Nested(te_r))
        out[f"{form}_unknown_key"] = errs

print("PROBE_JSON " + json.dumps(out))
