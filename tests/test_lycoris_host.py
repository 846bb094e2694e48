"""LyCORIS on the host (CPU): lycoris.lyco_delta against the deltas the reference's own apply_lycoris + LycorisHook._calc_updown
produced (tests/golden/lycoris_vectors.npz, made by tests/golden/make_lycoris_golden.py from seeded lattice tensors - exact in fp32,
so equality is bit for bit), the key rules and parse errors, and the host merge through lora's registry."""
import json
import os

import numpy as np
import pytest
import torch

import lyco_ref as LY
from gyre_amd import _lib, lora as LR, lycoris as LC

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lycoris_vectors.npz"))
META = json.loads(str(GOLDEN["meta"]))
ENTRIES = META["entries"]


def tree():
    """The module tree of the golden script (names and shapes)."""
    torch.manual_seed(0)
    net = torch.nn.Module()
    net.lin = torch.nn.Linear(8, 12)
    net.block = torch.nn.Module()
    net.block.to_q = torch.nn.Linear(8, 8, bias=False)
    net.block.conv1 = torch.nn.Conv2d(4, 6, 3, padding=1)
    net.block.proj_in = torch.nn.Conv2d(4, 6, 1)
    return net


def fields_of(entry, shape):
    KH, KW = (shape[2], shape[3]) if len(shape) == 4 else (1, 1)
    f = LY.lattice_fields(entry["form"], shape[0], shape[1], KH, KW, seed=entry["seed"], **entry["kwargs"])
    return {k: torch.from_numpy(np.asarray(v)) for k, v in f.items()}


def file_of(entry, shape):
    key = "lora_unet_" + entry["path"].replace(".", "_")
    return {f"{key}.{k}": v for k, v in fields_of(entry, shape).items()}


@pytest.mark.parametrize("i", range(len(ENTRIES)), ids=[f"{i}-{e['form']}-{e['path']}" for i, e in enumerate(ENTRIES)])
def test_lyco_delta_equals_the_reference(i):
    entry, want = ENTRIES[i], GOLDEN[f"delta_{i}"]
    fields = fields_of(entry, want.shape)
    assert sorted(file_of(entry, want.shape)) == entry["keys"]
    assert {"locon": "LycoUpDownModule", "loha": "LycoHadaModule", "lokr": "LycoKronModule", "full": "FullModule"}[LC._kind(fields)] == entry["cls"]
    got = LC.lyco_delta(fields, want.shape) * META["user_scale"]
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.abs(want).max() > 0
    np_fields = {k: v.numpy() for k, v in fields.items()}                 # ... and so does the float64 yardstick of the device tests
    ref = LY.delta64(np_fields, want.shape) * LY.file_scale(np_fields) * META["user_scale"]
    assert np.array_equal(ref.reshape(want.shape), want.astype(np.float64))
    assert LC.file_scale(fields) == LY.file_scale(np_fields)
    # through the key rules, from a whole file
    net = tree()
    (name, parsed), = LC._modules(net, file_of(entry, want.shape))
    assert name == entry["path"] + ".weight" and set(parsed) == set(fields)


def test_golden_covers_every_form_and_scale_rule():
    forms = {e["form"] for e in ENTRIES}
    assert forms == set(LY.FORMS)
    rules = {e["kwargs"].get("scale_rule", "alpha") for e in ENTRIES}
    assert rules == {"alpha", "scale", "scale0", "none"}
    assert {e["path"] for e in ENTRIES} == {"lin", "block.to_q", "block.conv1", "block.proj_in"}


def _one(form="loha", path="lin", **kw):
    net = tree()
    entry = dict(form=form, path=path, seed=7, kwargs=kw)
    return net, file_of(entry, tuple(dict(net.named_parameters())[path + ".weight"].shape))


def test_key_rules_and_parse_errors():
    net, good = _one()
    assert len(LC._modules(net, good)) == 1
    te = {"lora_te_text_model_encoder_layers_0_mlp_fc1.hada_w1_a": torch.zeros(2, 2)}
    assert LC._modules(net, te) == [] and len(LC._modules(net, {**good, **te})) == 1           # lora_te_: ignored
    with pytest.raises(ValueError, match="Unknown module key"):
        LC._modules(net, {"foo_lin.hada_w1_a": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="Couldn't find model"):
        LC._modules(net, {"lora_unet_nope.hada_w1_a": torch.zeros(1)})
    with pytest.raises(ValueError, match="Don't know how to handle key"):
        LC._modules(net, {**good, "lora_unet_lin.what": torch.zeros(1)})
    with pytest.raises(ValueError, match="lacks"):
        LC._modules(net, {k: v for k, v in good.items() if not k.endswith("hada_w2_b")})
    with pytest.raises(NotImplementedError, match="IA3"):
        LC._modules(net, {"lora_unet_lin.weight": torch.zeros(12), "lora_unet_lin.on_input": torch.tensor(False)})
    with pytest.raises(NotImplementedError, match="DyLoRA"):
        LC._modules(net, {"lora_unet_lin.dyn_up": torch.zeros(12, 2), "lora_unet_lin.dyn_down": torch.zeros(2, 8)})
    with pytest.raises(NotImplementedError, match="sparse bias"):
        LC._modules(net, {**good, "lora_unet_lin.bias_indices": torch.zeros(2, 1), "lora_unet_lin.bias_values": torch.zeros(1),
                          "lora_unet_lin.bias_size": torch.tensor([12, 8])})
    # a safetensors handle (keys / get_tensor) reads like a dict
    handle = type("H", (), {"keys": lambda s: good.keys(), "get_tensor": lambda s, k: good[k]})()
    assert LC._modules(net, handle)[0][0] == "lin.weight"


def test_shape_and_rank_errors():
    net, good = _one()
    w = dict(net.named_parameters())["lin.weight"]
    bad = dict(good)
    bad["lora_unet_lin.hada_w2_b"] = torch.zeros(4, 9)                                            # wrong input width
    with pytest.raises(ValueError):
        LC.apply_lycoris(net, bad, "x")
    net, two = _one(rank=3, rank2=2, scale_rule="scale")
    two = {k: v for k, v in two.items() if not k.endswith(".scale")}
    two["lora_unet_lin.alpha"] = torch.tensor(1.0)                                                # alpha / dim with two different dims
    with pytest.raises(ValueError, match="ambiguous"):
        LC.apply_lycoris(net, two, "x")
    net, kron = _one("lokr_dense", kron=(3, 2))
    kron["lora_unet_lin.lokr_w1"] = torch.zeros(5, 2)                                             # 5 does not divide 12
    with pytest.raises(ValueError):
        LC.apply_lycoris(net, kron, "x")
    assert torch.equal(dict(net.named_parameters())["lin.weight"], w)
    assert not getattr(net, "_lora_state", {"loras": {}})["loras"]


def test_host_merge_and_removal_restore_the_weights():
    net = tree()
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    tensors, deltas = {}, {}
    for i in (8, 10, 19, 20):                                             # LoHa, LoHa Tucker on the 3x3 conv, LoKr on the 1x1 conv, Full
        e = ENTRIES[i]
        tensors.update(file_of(e, GOLDEN[f"delta_{i}"].shape))
        deltas[e["path"] + ".weight"] = torch.from_numpy(GOLDEN[f"delta_{i}"]) / META["user_scale"]
    assert len(deltas) == 4
    assert LC.apply_lycoris(net, tensors, "a", 0.5) == 4
    params = dict(net.named_parameters())
    for name, d in deltas.items():
        assert torch.equal(params[name], before[name] + d * 0.5) and not torch.equal(params[name], before[name])
    LR.set_lora_scale(net, "a", 2.0)                                       # lora's registry covers it
    for name, d in deltas.items():
        assert torch.equal(params[name], before[name] + d * 2.0)
    kohya = {"lora_unet_lin.lora_up.weight": torch.ones(12, 1), "lora_unet_lin.lora_down.weight": torch.ones(1, 8)}
    LR.apply_lora(net, kohya, "b", 0.25)                                   # a LoRA stacks onto it in the same registry
    assert torch.equal(params["lin.weight"], before["lin.weight"] + deltas["lin.weight"] * 2.0 + 0.25)
    LR.remove_lora_from_model(net)
    for name, p in net.named_parameters():
        assert torch.equal(p, before[name]), name


def test_existing_lora_entry_points_still_refuse_lycoris():
    net, good = _one("lora", rank=2)
    mixed = {**good, "lora_unet_lin.lora_mid.weight": torch.zeros(2, 2, 1, 1)}
    assert LR.detect_lora_type(good) == "kohya-ss" and not LC.is_lycoris(good)
    with pytest.raises(ValueError, match="Lycoris"):
        LR.detect_lora_type(mixed)
    with pytest.raises(ValueError, match="Lycoris"):
        LR.apply_lora(net, mixed, "x")
    assert LC.is_lycoris(mixed) and LC.is_lycoris(_one()[1])
    term = LR.Term(_lib.DELTA_LORA, [(torch.zeros(12, 2), torch.zeros(2, 8))], 0.5)
    f = LR.Factors({"lin.weight": term}, torch.device("cpu"))
    assert list(f.terms) == ["lin.weight"] and list(f.names()) == ["lin.weight"] and f.hits("nope") == []
    assert f.hits("lin.weight") == [term] and LC.Term is LR.Term and LC.Factors is LR.Factors
