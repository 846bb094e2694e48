"""gyre_amd/text_adapters.py on the CPU: key mapping, the scale rule, the host merge against the reference's hook form in float64,
and textual inversion through the engine's text side (tiny CLIPTextModel, stub tokenizer; nothing downloaded, no GPU).

Parity gate: rel-L2 <= 1e-10 in float64 - many orders above accumulated fp64 roundoff, many below any indexing or scale mistake."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lyco_ref as LY
import text_adapter_util as U
from gyre_amd import text_adapters as TA
from gyre_amd.engine import GyreUnifiedPipeline

GATE = 1e-10


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- key mapping, scale rule ----------------------------------------------------------------------------------------------------
def test_key_mapping_covers_every_linear_of_a_layer():
    te = U.tiny_encoder()
    for layer in (0, 1):
        for name in U.LINEARS:
            assert TA.resolve(te, U.key_of(layer, name)) is U.linear(te, layer, name)
    with pytest.raises(RuntimeError, match="Couldn't find model"):
        TA.resolve(te, "lora_te_text_model_encoder_layers_0_mlp_fc3")
    with pytest.raises(RuntimeError, match="Couldn't find model"):
        TA.resolve(te, "lora_te_text_model_encoder_layers_7_mlp_fc1")
    # an encoder that nests its tower under .text_model (transformers 4) resolves the same keys
    class Nested(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.text_model = inner
    nested = Nested(U.tower(te))
    assert TA.resolve(nested, U.key_of(1, "mlp.fc2")) is U.linear(te, 1, "mlp.fc2")
    # not an nn.Linear: the reference's ValueError
    f = {"lora_te_text_model_encoder_layers_0_layer_norm1.lora_down.weight": torch.ones(4, 32),
         "lora_te_text_model_encoder_layers_0_layer_norm1.lora_up.weight": torch.ones(32, 4)}
    with pytest.raises(ValueError, match="Can't apply LoRA to module of type LayerNorm"):
        TA.text_modules(te, f)
    with pytest.raises(RuntimeError):
        TA.text_modules(te, {k.replace("layer_norm1", "nothing"): v for k, v in f.items()})


def test_unet_entries_and_other_formats_have_no_text_side():
    te = U.tiny_encoder()
    assert TA.text_modules(te, {"lora_unet_mid_block_x.lora_down.weight": torch.ones(2, 2), "lora_unet_mid_block_x.lora_up.weight": torch.ones(2, 2)}) == []
    assert not TA.has_text_keys({"a.processor.to_k_lora.down.weight": 0, "a.processor.to_k_lora.up.weight": 0})
    one = U.te_file(te, "lora", targets=[(0, "mlp.fc1")])
    assert [m[1] for m in TA.text_modules(te, one)] == [U.linear(te, 0, "mlp.fc1")]
    # fail closed exactly as for the UNet: IA3, DyLoRA, sparse bias
    k = U.key_of(0, "mlp.fc1")
    for extra in ({k + ".weight": torch.ones(64), k + ".on_input": torch.tensor(1.0)}, {k + ".dyn_up": torch.ones(64, 1), k + ".dyn_down": torch.ones(1, 32)},
                  {**U.te_file(te, "loha", targets=[(0, "mlp.fc1")]), k + ".bias_indices": torch.ones(1, 1), k + ".bias_values": torch.ones(1),
                   k + ".bias_size": torch.ones(1)}):
        with pytest.raises(NotImplementedError):
            TA.upload_text_factors(te, extra)
    # a mis-shaped module is a ValueError, an all-zero one is the zero delta and is skipped
    bad = {k + ".lora_down.weight": torch.ones(4, 8), k + ".lora_up.weight": torch.ones(8, 4)}
    with pytest.raises(ValueError):
        TA.upload_text_factors(te, bad)
    assert len(TA.upload_text_factors(te, {n: v * 0 for n, v in bad.items()})) == 0


def test_scale_rule():
    s = TA.text_scale
    assert s({}) == 1.0 and s(None) == 1.0 and s({"unet": 0.3}) == 1.0
    assert s({"text_encoder": 0.25}) == 0.25 and s({"*": 0.5}) == 0.5
    assert s({"*": 0.5, "text_encoder": 0.125}) == 0.125 and s({"text_encoder": 0.125, "*": 0.5}) == 0.5      # the last one wins
    assert s({"*": 0.5, "unet": 2.0}) == 0.5 and s({"nobody": 3.0}) == 1.0


# ---- parity with the reference's hook form, float64 -------------------------------------------------------------------------------
def _hooked(te, tensors, scale):
    """The hook form restated from lora.py:145-157 on a copy of ``te``: ``up(down(x)) * alpha / r * scale`` added to the module output
    (LoRA); for LyCORIS modules, whose reference hook swaps ``weight + updown`` in, the float64 delta of lyco_ref applied to the same
    input and added to the output."""
    te = copy.deepcopy(te)
    groups = {}
    for k, v in tensors.items():
        groups.setdefault(k.split(".")[0], {})[k.split(".", 1)[1]] = v.double()
    for key, f in groups.items():
        module = TA.resolve(te, key)
        if set(f) <= {"lora_up.weight", "lora_down.weight", "alpha"}:
            up, down, r = f["lora_up.weight"], f["lora_down.weight"], f["lora_down.weight"].shape[0]
            iscale = float(f["alpha"]) / r if "alpha" in f else 1.0
            hook = lambda m, a, out, up=up, down=down, iscale=iscale: out + F.linear(F.linear(a[0], down), up) * iscale * scale
        else:
            fn = {k: v.numpy() for k, v in f.items()}
            d = torch.from_numpy(LY.delta64(fn, tuple(module.weight.shape))[:, :, 0] * LY.file_scale(fn))
            hook = lambda m, a, out, d=d: out + F.linear(a[0], d) * scale
        module.register_forward_hook(hook)
    return te


@pytest.mark.parametrize("form", ["lora", "loha", "lokr_lowrank", "lokr_dense", "full"])
def test_host_merge_equals_the_hook_form_in_float64(form):
    te = U.tiny_encoder(dtype=torch.float64)
    ids = U.ids_batch(128)
    base = U.encode(te, ids)
    tensors = U.te_file(te, form, shrink=2.0 ** -2)
    want = U.encode(_hooked(te, tensors, 0.75), ids)
    before = {k: v.clone() for k, v in te.state_dict().items()}
    f = TA.upload_text_factors(te, tensors)
    assert f.deltas is not None and len(f) == 7
    assert TA.attach(te, [(f, 0.75)]) == 7
    got = U.encode(te, ids)
    assert rel_l2(want, base) > 1e-3, "the file does not move the encoder: the comparison would show nothing"
    assert rel_l2(got, want) <= GATE, rel_l2(got, want)
    TA.detach(te)
    assert all(torch.equal(v, before[k]) for k, v in te.state_dict().items())
    assert torch.equal(U.encode(te, ids), base)


def test_two_files_sum_and_the_ninth_term_is_refused():
    te = U.tiny_encoder(dtype=torch.float64)
    ids = U.ids_batch(128)
    a, b = U.te_file(te, "lora", seed=1), U.te_file(te, "loha", seed=2)
    fa, fb = TA.upload_text_factors(te, a), TA.upload_text_factors(te, b)
    TA.attach(te, [(fa, 0.5), (fb, 1.0)])
    got = U.encode(te, ids)
    TA.detach(te)
    want = U.encode(_hooked(_hooked(te, a, 0.5), b, 1.0), ids)
    assert rel_l2(got, want) <= GATE
    base = U.encode(te, ids)
    with pytest.raises(ValueError, match="at most 8"):
        TA.attach(te, [(fa, 1.0)] * 9)
    assert torch.equal(U.encode(te, ids), base)
    assert TA.attach(te, [(fa, 0.0)]) == 0                                 # scale 0 contributes nothing


def test_half_precision_master_is_rounded_once():
    """base + sum of deltas in fp32, one rounding to the encoder's dtype: two deltas that cancel leave the bf16 weight's bits, a delta
    below half an ulp of W moves it together with a second one (a 16-bit master accumulating them one by one loses both)."""
    te = U.tiny_encoder(dtype=torch.bfloat16)
    w = U.linear(te, 0, "mlp.fc1").weight
    w.data.fill_(1.0)
    d = torch.full(tuple(w.shape), 2.0 ** -9)                              # ulp(1.0) in bf16 is 2^-7: 2^-9 alone rounds away
    k = U.key_of(0, "mlp.fc1")
    tensors = {k + ".diff": d}
    f = TA.upload_text_factors(te, tensors)
    TA.attach(te, [(f, 1.0)])
    assert bool((w == 1.0).all())
    TA.attach(te, [(f, 1.0), (f, 1.0), (f, 1.0)])                          # 3 * 2^-9 > half an ulp
    assert bool((w == 1.0 + 2.0 ** -7).all())
    TA.detach(te)
    assert bool((w == 1.0).all())


# ---- textual inversion -------------------------------------------------------------------------------------------------------------
def _engine(te, tok):
    return GyreUnifiedPipeline(vae=None, text_encoder=te, tokenizer=tok, unet=torch.nn.Linear(1, 1))


def _embed(eng, prompt, tokenizer=None):
    return eng._embed([prompt], None, 1, 1, True, 3, tokenizer)


def _big_encoder(dtype=torch.float32):
    return U.tiny_encoder(vocab=49408, dtype=dtype)                        # the embedder's BOS / EOS ids are CLIP's


def _hand_extended(te, rows):
    """A copy whose token table was extended and filled by hand."""
    te = copy.deepcopy(te)
    old = te.get_input_embeddings().weight.data
    new = torch.nn.Embedding(old.shape[0] + len(rows), old.shape[1]).to(old.dtype)
    new.weight.data[:old.shape[0]] = old
    for i, r in enumerate(rows):
        new.weight.data[old.shape[0] + i] = r.to(old.dtype)
    te.set_input_embeddings(new)
    return te


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_token_embeddings_equal_the_hand_extended_encoder(dtype):
    te = _big_encoder(dtype)
    tok = U.StubTokenizer()
    eng = _engine(te, tok)
    g = torch.Generator().manual_seed(3)
    one, three = torch.randn(32, generator=g), torch.randn(3, 32, generator=g)
    base = _embed(eng, "a photo of <cat> by <style> please")
    ti = {"<cat>": one, "<style>": three}
    tokenizer = eng._text_side([], ti)
    assert tokenizer is not tok and len(tok) == 49408 and len(tokenizer) == 49412
    assert tokenizer._multidim_mappings == {"<style>": "<style00> <style01> <style02>"}
    table = te.get_input_embeddings().weight
    assert table.shape[0] == 49412 and table.dtype == dtype
    assert torch.equal(table[49408], one.to(dtype)) and torch.equal(table[49409:49412], three.to(dtype))
    got = _embed(eng, "a photo of <cat> by <style> please", tokenizer)
    # the same prompt with the sub-tokens spelt out, on an encoder extended by hand
    hand = _engine(_hand_extended(_big_encoder(dtype), [one, *three]), tokenizer)
    want = _embed(hand, "a photo of <cat> by <style00> <style01> <style02> please", tokenizer)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], base[0])
    # the multi-vector text is replaced BEFORE tokenising: three ids for <style>
    seen = []
    tokenizer2 = copy.deepcopy(tokenizer)
    orig = tokenizer2.__call__
    tokenizer2.__class__ = type("Spy", (U.StubTokenizer,), {"__call__": lambda self, text, **k: (seen.append(text), orig(text, **k))[1]})
    _embed(eng, "by <style>", tokenizer2)
    assert any("<style00> <style01> <style02>" in t for t in seen) and not any("<style>" in t for t in seen)
    # the next request: the table is back, the base prompt encodes as before
    assert eng._text_side([], None) is tok
    assert te.get_input_embeddings().weight.shape[0] == 49408
    again = _embed(eng, "a photo of <cat> by <style> please")
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])


def test_wrong_dimension_raises_before_anything_changed():
    te = _big_encoder()
    tok = U.StubTokenizer()
    eng = _engine(te, tok)
    lora = U.te_file(te, "lora")
    eng._text_side([(lora, {})], None)                                     # something attached by the previous request
    w = U.linear(te, 0, "mlp.fc1").weight.clone()
    for bad in ({"<x>": torch.zeros(33)}, {"<ok>": torch.zeros(32), "<y>": torch.zeros(2, 31)}, {"<z>": torch.zeros(2, 2, 32)}):
        with pytest.raises(ValueError, match="embedding dim"):
            eng._text_side([], bad)
        assert te.get_input_embeddings().weight.shape[0] == 49408 and len(tok) == 49408
        assert torch.equal(U.linear(te, 0, "mlp.fc1").weight, w)           # not even the previous request's adapter was taken off


def test_engine_text_side_applies_and_strips_lora():
    te = _big_encoder()
    tok = U.StubTokenizer()
    eng = _engine(te, tok)
    base = _embed(eng, "a photo of a cat")
    lora = U.te_file(te, "lora")
    assert eng._text_side([(lora, {"text_encoder": 0.5})], None) is tok
    half = _embed(eng, "a photo of a cat")
    eng._text_side([(U.te_file(te, "lora", alpha_factor=0.5), {"unet": 3.0})], None)
    assert torch.equal(_embed(eng, "a photo of a cat")[0], half[0]) and not torch.equal(half[0], base[0])
    assert len(eng._text_uploads) == 2
    eng._text_side([(lora, {"text_encoder": 0.5})], None)
    assert len(eng._text_uploads) == 2                                     # the same mapping object: prepared once
    eng._text_side([], None)
    assert torch.equal(_embed(eng, "a photo of a cat")[0], base[0])
