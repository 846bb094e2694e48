"""Shared by the text-adapter tests (host, reference, gpu): a tiny CLIP text encoder, a stub tokenizer that meets the contract of
gyre_amd/text_adapters.py, and ``lora_te_`` files over the encoder's Linear weights with lyco_ref's lattice tensors (every delta a
multiple of a power of two: exact in fp32 next to any weight, so the device merge and the host merge must agree bit for bit)."""
import numpy as np
import torch

import lyco_ref as LY

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")
BOS, EOS = 49406, 49407


class StubTokenizer:
    """add_tokens / convert_tokens_to_ids / __len__ / __call__: words hash into the base vocabulary (the deterministic word hash of
    tests/test_gpu_engine.tokenizer), added tokens get the next free ids."""

    def __init__(self, vocab_size=49408):
        self.vocab_size, self.added = vocab_size, {}

    def __len__(self):
        return self.vocab_size + len(self.added)

    def add_tokens(self, tokens):
        assert isinstance(tokens, list)
        new = [t for t in tokens if t not in self.added]
        for t in new:
            self.added[t] = len(self)
        return len(new)

    def convert_tokens_to_ids(self, token):
        return self.added[token]

    def word_id(self, w):
        return self.added[w] if w in self.added else 3 + (sum(ord(c) * (i + 1) for i, c in enumerate(w)) % min(40000, self.vocab_size - 8))

    def __call__(self, text, add_special_tokens=False):
        return {"input_ids": [self.word_id(w) for w in text.split()]}

    def encode(self, text):                                 # BOS + ids + EOS, as a CLIP tokenizer's encode
        return [BOS] + self(text)["input_ids"] + [EOS]


def tiny_encoder(hidden=32, intermediate=64, layers=2, vocab=128, dtype=torch.float32, seed=0):
    """A CLIPTextModel of a small CLIPTextConfig, nothing downloaded."""
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(seed)
    te = CLIPTextModel(CLIPTextConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=intermediate, num_hidden_layers=layers,
                                      num_attention_heads=2, max_position_embeddings=77, bos_token_id=vocab - 2, eos_token_id=vocab - 1,
                                      pad_token_id=vocab - 1)).eval()
    shift_final_norm(te)
    return te.to(dtype)


def shift_final_norm(te):
    """A freshly initialised final LayerNorm (weight 1, bias 0) gives every token a zero mean, and long-prompt weighting divides by
    the mean of the embedding: give it the non-trivial affine part every trained encoder has."""
    ln = tower(te).final_layer_norm
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(ln.weight.shape, generator=g))
        ln.bias.copy_(0.1 + 0.2 * torch.randn(ln.bias.shape, generator=g))


def tower(te):
    return getattr(te, "text_model", te)


def linear(te, layer, name):
    m = tower(te).encoder.layers[layer]
    for part in name.split("."):
        m = getattr(m, part)
    return m


def key_of(layer, name):
    return f"lora_te_text_model_encoder_layers_{layer}_{name.replace('.', '_')}"


def te_file(te, form="lora", targets=None, seed=0, shrink=2.0 ** -4, alpha_factor=1.0, **kw):
    """A file with ``lora_te_`` entries only: ``form`` (a lyco_ref form) over ``targets = [(layer, linear name)]`` (default: every
    Linear of layer 0 and mlp.fc1 of the last layer).  alpha_factor scales the file scale (its alpha or scale key)."""
    n_layers = len(tower(te).encoder.layers)
    targets = targets if targets is not None else [(0, n) for n in LINEARS] + [(n_layers - 1, "mlp.fc1")]
    if form.startswith("lokr"):
        kw.setdefault("kron", (4, 2))
    if form != "full" and not form.startswith("lokr_dense"):
        kw.setdefault("rank", 4)
    out = {}
    for i, (layer, name) in enumerate(targets):
        w = linear(te, layer, name).weight
        f = LY.lattice_fields(form, w.shape[0], w.shape[1], seed=seed * 100 + i, shrink=shrink, **kw)
        for p, v in f.items():
            t = torch.from_numpy(np.array(v, dtype=np.float32))
            if p in ("alpha", "scale"):
                t = t * alpha_factor
            out[f"{key_of(layer, name)}.{p}"] = t
    return out


def ids_batch(vocab, seed=0, n=2, length=77):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 8, (n, length), generator=g)
    ids[:, 0], ids[:, -1] = vocab - 2, vocab - 1
    return ids


def encode(te, ids):
    with torch.no_grad():
        return te(input_ids=ids.to(next(te.parameters()).device), return_dict=True).last_hidden_state
