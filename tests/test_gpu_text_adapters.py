"""Per-request text-encoder adapters on the device (-m gpu): ``lora_te_`` entries merged into a CLIP text encoder's weights by
gyre_op_merge_delta (gyre_amd/text_adapters.py), textual-inversion token embeddings, and the engine's ``lora=`` /
``token_embeddings=`` over a tiny UNet / VAE / encoder (3 steps at 128 x 128).

The files carry lyco_ref's lattice tensors: every delta is a multiple of a power of two, so the device merge (factors stay factors,
fp32 fma chain, one rounding to the encoder's dtype) and the host merge (multiplied out, fp32 sum, one rounding) must give the same
bits, in fp32, bf16 and fp16 encoders."""
import copy

import pytest
import torch

import text_adapter_util as U
from gyre_amd import config as gcfg, text_adapters as TA
from gyre_amd.engine import GyreUnifiedPipeline
from gpu_util import DEV

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PROMPT = ["a photo of a cat"]


def encoder(dtype):
    return U.tiny_encoder(hidden=64, intermediate=128, dtype=dtype)


def host_merged(te_cpu, specs):
    """A copy of the (CPU) encoder whose weights were ASSIGNED from the host merge: nothing stays attached to it."""
    te = copy.deepcopy(te_cpu)
    TA.attach(te, [(TA.upload_text_factors(te, t), s) for t, s in specs])
    delattr(te, TA._STATE)
    return te


# ---- the module path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lora", "loha", "lokr_lowrank", "lokr_dense", "full"])
@pytest.mark.parametrize("dtype", list(DT))
def test_attached_encoder_equals_the_host_merged_copy(dtype, form):
    cpu = encoder(DT[dtype])
    te = copy.deepcopy(cpu).to(DEV)
    ids = U.ids_batch(128)
    base = U.encode(te, ids)
    before = {k: v.clone() for k, v in te.state_dict().items()}
    tensors = U.te_file(cpu, form)
    f = TA.upload_text_factors(te, tensors)
    assert f.terms is not None and f.device.type == "cuda" and len(f) == 7
    assert TA.attach(te, [(f, 0.5)]) == 7
    want = host_merged(cpu, [(tensors, 0.5)]).to(DEV)
    for (k, a), (_, b) in zip(te.state_dict().items(), want.state_dict().items()):
        assert torch.equal(a, b), k
    got = U.encode(te, ids)
    assert torch.equal(got, U.encode(want, ids)) and not torch.equal(got, base)
    TA.detach(te)
    assert all(torch.equal(v, before[k]) for k, v in te.state_dict().items())        # bit for bit
    assert torch.equal(U.encode(te, ids), base)


@pytest.mark.parametrize("dtype", list(DT))
def test_scale_equals_a_halved_alpha_and_two_files_sum(dtype):
    cpu = encoder(DT[dtype])
    te = copy.deepcopy(cpu).to(DEV)
    ids = U.ids_batch(128)
    a, a_half = U.te_file(cpu, "lora", seed=1), U.te_file(cpu, "lora", seed=1, alpha_factor=0.5)
    b = U.te_file(cpu, "loha", seed=2)
    fa, fh, fb = (TA.upload_text_factors(te, t) for t in (a, a_half, b))
    TA.attach(te, [(fa, 0.5)])
    half = {k: v.clone() for k, v in te.state_dict().items()}
    TA.attach(te, [(fh, 1.0)])                                             # (attach takes the previous set off first)
    assert all(torch.equal(v, half[k]) for k, v in te.state_dict().items())
    TA.attach(te, [(fa, 0.5), (fb, 1.0)])                                  # two files of one request: ONE write per weight
    want = host_merged(cpu, [(a, 0.5), (b, 1.0)]).to(DEV)
    assert all(torch.equal(v, w) for v, w in zip(te.state_dict().values(), want.state_dict().values()))
    assert torch.equal(U.encode(te, ids), U.encode(want, ids))
    with pytest.raises(ValueError, match="at most 8"):
        TA.attach(te, [(fa, 1.0)] * 9)
    assert all(torch.equal(v, w.to(DEV)) for v, w in zip(te.state_dict().values(), cpu.state_dict().values()))
    TA.detach(te)


# ---- the engine --------------------------------------------------------------------------------------------------------------
def make_engine():
    from test_gpu_engine import build_engine, sample_euler_ancestral
    _, _, eng = build_engine(gcfg.tiny_unet(), gcfg.tiny_vae())
    U.shift_final_norm(eng.text_encoder)
    eng.tokenizer = U.StubTokenizer()
    eng.scheduler = sample_euler_ancestral
    return eng


def req(eng, prompt=PROMPT, **kw):
    from test_gpu_engine import generators, wrapper_kwargs
    return eng(**wrapper_kwargs(prompt=prompt, generator=generators([11]), width=128, height=128, num_inference_steps=3, **kw))[0]


@pytest.fixture(scope="module")
def engine():
    eng = make_engine()
    return eng, req(eng)


def test_a_file_with_only_text_entries_changes_the_conditioning_and_the_image(engine):
    eng, plain = engine
    te = eng.text_encoder
    before = {k: v.clone() for k, v in te.state_dict().items()}
    cond = eng._embed(PROMPT, None, 1, 1, True, 3)[0]
    tensors = U.te_file(te, "lora", shrink=2.0 ** -2)
    got = req(eng, lora=[(tensors, {})])
    assert not torch.equal(got, plain) and bool(torch.isfinite(got).all())
    assert not torch.equal(eng._embed(PROMPT, None, 1, 1, True, 3)[0], cond)          # still attached: stripped by the NEXT request
    # weights = {"text_encoder": 0.5} equals a file with halved alpha, "unet" does not reach the text side
    half = req(eng, lora=[(tensors, {"text_encoder": 0.5, "unet": 2.0})])
    assert torch.equal(half, req(eng, lora=[(U.te_file(te, "lora", shrink=2.0 ** -2, alpha_factor=0.5), {})]))
    assert not torch.equal(half, got) and not torch.equal(half, plain)
    # two files in one request, a LyCORIS one among them
    loha = U.te_file(te, "loha", seed=5, shrink=2.0 ** -2)
    both = req(eng, lora=[(tensors, {"*": 0.5}), (loha, {})])
    want = host_merged(_bare_cpu(te), [(tensors, 0.5), (loha, 1.0)])
    for layer, name in [(0, n) for n in U.LINEARS] + [(1, "mlp.fc1")]:
        assert torch.equal(U.linear(te, layer, name).weight, U.linear(want, layer, name).weight.to(DEV)), name
    assert not torch.equal(both, half)
    # the request after it, with no lora: the pre-adapter image and the pre-adapter weights, bit for bit
    assert torch.equal(req(eng), plain)
    assert all(torch.equal(v, before[k]) for k, v in te.state_dict().items())
    assert len(eng._text_uploads) == 3                                     # three mapping objects, each prepared once


def _bare_cpu(te):
    """A CPU copy of an encoder with whatever is attached taken off the COPY."""
    c = copy.deepcopy(te)
    TA.detach(c)
    return c.cpu()


def test_token_embeddings_equal_the_hand_extended_encoder_and_are_gone_afterwards(engine):
    eng, plain = engine
    te, tok = eng.text_encoder, eng.tokenizer
    g = torch.Generator().manual_seed(3)
    one, three = torch.randn(64, generator=g), torch.randn(3, 64, generator=g)
    prompt = ["a photo of <cat> by <style>"]
    without = req(eng, prompt)
    got = req(eng, prompt, token_embeddings={"<cat>": one, "<style>": three})
    assert not torch.equal(got, without) and bool(torch.isfinite(got).all())
    assert te.get_input_embeddings().weight.shape[0] == 49412 and len(tok) == 49408          # the request's copy got the tokens
    # the same request on an engine whose encoder was extended by hand, sub-tokens spelt out
    hand = make_engine()
    old = hand.text_encoder.get_input_embeddings().weight.data
    new = torch.nn.Embedding(49412, 64).to(DEV)
    new.weight.data[:49408] = old
    new.weight.data[49408], new.weight.data[49409:] = one.to(DEV), three.to(DEV)
    hand.text_encoder.set_input_embeddings(new)
    hand.tokenizer.add_tokens(["<cat>", "<style00>", "<style01>", "<style02>"])
    hand_eng_prompt = ["a photo of <cat> by <style00> <style01> <style02>"]
    from test_gpu_engine import generators, wrapper_kwargs
    hand._text_side = lambda specs, ti: hand.tokenizer                     # keep the hand-made table: no per-request strip on this engine
    want = hand(**wrapper_kwargs(prompt=hand_eng_prompt, generator=generators([11]), width=128, height=128, num_inference_steps=3))[0]
    assert torch.equal(got, want)
    # the next request: gone
    assert torch.equal(req(eng, prompt), without) and te.get_input_embeddings().weight.shape[0] == 49408
    assert torch.equal(req(eng), plain)
    with pytest.raises(ValueError, match="embedding dim"):
        req(eng, prompt, token_embeddings={"<cat>": torch.zeros(63)})
    assert te.get_input_embeddings().weight.shape[0] == 49408


def test_an_sdxl_engine_still_refuses_token_embeddings():
    from types import SimpleNamespace
    from test_gpu_engine import generators, sample_euler_ancestral, wrapper_kwargs
    unet = torch.nn.Linear(1, 1)
    unet.config = SimpleNamespace(addition_embed_type="text_time")
    eng = GyreUnifiedPipeline(vae=None, text_encoder=encoder(torch.float32), tokenizer=U.StubTokenizer(), unet=unet)
    eng.scheduler = sample_euler_ancestral
    with pytest.raises(NotImplementedError, match="SDXL"):
        eng(**wrapper_kwargs(prompt=PROMPT, generator=generators([1]), width=128, height=128, num_inference_steps=2,
                             token_embeddings={"<cat>": torch.zeros(64)}))
