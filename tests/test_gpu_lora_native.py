"""Per-request LoRA on the device (-m gpu): the fused delta-merge repack kernel (gyre_op_repack_lora), the store entry
(gyre_unet_set_weight_lora; the module path issues its pairs as LORA terms of gyre_unet_set_weight_delta), the module path (lora.attach_lora / set_attached_scale / detach_loras) and the engine's ``lora=``.

Yardsticks (tests/lora_ref.py, checked on the CPU by tests/test_lora_ref_host.py): on the LATTICE family every value is exact in
fp32 in any order and representable in the storage type, so the kernel must equal the float64 reference - and the host path
(lora_delta + ``w + d * scale``, then the plain repack) - bit for bit; on GAUSSIAN data it must stay inside the bound derived
from the kernel's stated operation order.  Model tests compare the attached module with a second module that got the same LoRA
through the existing host merge (apply_lora): a lattice LoRA adds an exactly representable delta, so both paths round
base + delta once, to the same bits.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import lora_ref as LRF
from gyre_amd import _lib, config as gcfg, lora as LR, weights
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV, HDT, randn, release_kept, report, st, vp
from test_lora_ref_host import CASES

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "storage": HDT}


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def run_op(base, pairs, I_pad, geglu, scale_p, base_dtype=torch.float32, factor_dtypes=None):
    """gyre_op_repack_lora on device copies of (base, pairs) -> [O][KH][KW][I_pad] tensor of HDT (cpu); the output buffer is
    pre-filled with ones, so an element the kernel does not write (pad columns included) shows."""
    L = _lib.lib()
    O, I, KH, KW = LRF._shape(base)
    b = _t(base, base_dtype).to(DEV)
    arr = (_lib.LoraPair * max(len(pairs), 1))()
    for j, (up, down, s) in enumerate(pairs):
        fdt = factor_dtypes[j] if factor_dtypes else torch.float32
        u, d = _t(up, fdt).to(DEV), _t(down, fdt).to(DEV)
        arr[j].up, arr[j].down = vp(u).value, vp(d).value
        arr[j].dtype, arr[j].rank, arr[j].scale = _lib.dtype_code(u), down.shape[0], s
    out = torch.ones(O * KH * KW * I_pad, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_repack_lora(st(), vp(b), _lib.dtype_code(b), O, I, KH, KW, I_pad, int(geglu), scale_p, len(pairs), arr, vp(out)))
    res = out.cpu().reshape(O, KH, KW, I_pad)
    release_kept()
    return res


def plain_repack(w, I_pad, geglu):
    """The existing repack operators on an fp32 tensor (conv form for everything but the GEGLU interleave)."""
    L = _lib.lib()
    O, I, KH, KW = LRF._shape(w)
    src = _t(w).to(DEV)
    out = torch.ones(O * KH * KW * I_pad, dtype=HDT, device=DEV)
    if geglu:
        assert I_pad == I
        _lib.check(L.gyre_op_repack_linear_weight(st(), vp(src), O, I, 1, vp(out)))
    else:
        _lib.check(L.gyre_op_repack_conv_weight(st(), vp(src), O, I, KH, KW, I_pad, vp(out)))
    res = out.cpu().reshape(O, KH, KW, I_pad)
    release_kept()
    return res


def host_merged(base, pairs, aor):
    """What apply_lora hands to the upload: base + lora_delta * user scale, fp32, in pair order."""
    w = _t(base).clone()
    for (up, down, s), a in zip(pairs, aor):
        w = w + LR.lora_delta(_t(up), _t(down), torch.tensor(a * down.shape[0])) * (s / a)
    return w.numpy()


def quantized(pairs, factor_dtypes):
    """The pairs as the kernel sees them when the factors are stored in 16 bits (the references start from these values)."""
    return [(_t(up, fdt).float().numpy(), _t(down, fdt).float().numpy(), s) for (up, down, s), fdt in zip(pairs, factor_dtypes)]


@pytest.mark.parametrize("case", CASES + [("cancel", 72, 12, 3, 3, 16, False, 1.0, (4,))], ids=[c[0] for c in CASES] + ["cancel"])
def test_operator_lattice_is_bit_exact(case):
    """== the float64 reference, == the plain repack of the host-merged fp32 tensor, pad columns zero."""
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    conv = name.startswith("conv") or KH * KW > 1
    base, pairs, aor = LRF.lattice(O, I, ranks, KH, KW, conv=conv, seed=len(name), cancel=name == "cancel")
    ref = LRF.ref64(base, pairs, I_pad, geglu, scale_p)
    got = run_op(base, pairs, I_pad, geglu, scale_p)
    assert np.array_equal(got.double().numpy(), ref), name
    assert not got[..., I:].any()
    host = plain_repack(host_merged(base, pairs, aor) * np.float32(scale_p), I_pad, geglu)       # (scale_p: a power of two here)
    assert torch.equal(got, host)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_operator_gaussian_within_the_bound(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    sp = scale_p if scale_p == 1.0 else 0.1803
    base, pairs = LRF.gaussian(O, I, ranks, KH, KW, conv=name.startswith("conv") or KH * KW > 1, seed=len(name))
    got = run_op(base, pairs, I_pad, geglu, sp)
    ratio = LRF.worst_ratio(name, got, LRF.ref64(base, pairs, I_pad, geglu, sp), LRF.bound(base, pairs, I_pad, geglu, sp, HDT))
    assert ratio <= 1.0 and not got[..., I:].any()


@pytest.mark.parametrize("fdts", [("f32",), ("bf16",), ("f16",), ("f16", "bf16")])
@pytest.mark.parametrize("bdt", ["f32", "storage"])
def test_operator_dtypes(fdts, bdt):
    """Factors in fp32 / bf16 / fp16 (two pairs: different rank AND dtype), base in fp32 and in the storage type."""
    O, I, KH, KW, I_pad = 72, 12, 3, 3, 16
    ranks = (33, 4)[:len(fdts)]
    fd, bd = [TDT[f] for f in fdts], TDT[bdt]
    base, pairs, aor = LRF.lattice(O, I, ranks, KH, KW, seed=11)
    got = run_op(base, pairs, I_pad, False, 1.0, bd, fd)                   # lattice values are exact in every one of the types
    assert np.array_equal(got.double().numpy(), LRF.ref64(base, pairs, I_pad))
    base, pairs = LRF.gaussian(O, I, ranks, KH, KW, seed=12)
    base, pairs = _t(base, bd).float().numpy(), quantized(pairs, fd)
    got = run_op(base, pairs, I_pad, False, 0.1803, bd, fd)
    assert LRF.worst_ratio(f"{fdts} base {bdt}", got, LRF.ref64(base, pairs, I_pad, False, 0.1803),
                           LRF.bound(base, pairs, I_pad, False, 0.1803, HDT)) <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("linear_padded_k", "conv3x3", "geglu")], ids=lambda c: c[0])
def test_operator_without_pairs_is_the_plain_repack(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    base, _ = LRF.gaussian(O, I, (), KH, KW, conv=KH * KW > 1, seed=3)
    assert torch.equal(run_op(base, [], I_pad, geglu, 1.0), plain_repack(base, I_pad, geglu))


@pytest.mark.parametrize("with_pair", [False, True], ids=["no_pairs", "lattice_pair"])
@pytest.mark.parametrize("shape", [(256, 256, 3, 3), (320, 250, 1, 1)], ids=["conv3x3", "matrix_padded_k"])
def test_operator_folded_scale_has_the_plain_repack_bits(shape, with_pair):
    """A factor that is no power of two (the softmax scale the store folds into to_k), normal base weights, ~600 000 elements:
    the packed bits equal the plain repack's own scale-and-round of the same fp32 values, element by element.  (The fp16 build
    contracts product and conversion into one rounding there; a product rounded to fp32 first differs in ~1 element in 10^4.)
    with a lattice pair: base + delta is one fp32 rounding on either side, so the host-merged tensor is the same input."""
    L = _lib.lib()
    O, I, KH, KW = shape
    I_pad, scale = (I + 7) // 8 * 8, 0.22808579
    conv = KH * KW > 1
    base = (np.random.default_rng(7).standard_normal((O, I, KH, KW) if conv else (O, I)) * 0.05).astype(np.float32)
    pairs, merged = [], base
    if with_pair:
        _, pairs, aor = LRF.lattice(O, I, (33,), KH, KW, conv=conv, seed=8, scales=[(0.5, 2.0 ** -5)])
        merged = host_merged(base, pairs, aor)
    got = run_op(base, pairs, I_pad, False, scale)
    src = _t(merged).to(DEV)
    out = torch.ones(O * KH * KW * I_pad, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_repack_conv_weight_scaled(st(), vp(src), 0, O, I, KH, KW, I_pad, scale, vp(out)))
    want = out.cpu().reshape(O, KH, KW, I_pad)
    release_kept()
    differ = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert differ == 0, f"{differ} of {got.numel()} packed elements differ from the plain repack"


def test_operator_refuses_bad_arguments():
    base, pairs, _ = LRF.lattice(40, 24, (4,), seed=1)
    with pytest.raises(ValueError):
        run_op(base, pairs * 9, 24, False, 1.0)
    with pytest.raises(ValueError):
        run_op(base, [(pairs[0][0][:, :0], pairs[0][1][:0], 1.0)], 24, False, 1.0)            # rank 0
    with pytest.raises(ValueError):
        run_op(base, pairs, 22, False, 1.0)                                                    # I_pad < I
    with pytest.raises(ValueError):
        run_op(base, pairs, 24, True, 1.0)                                                     # GEGLU needs O % 32 == 0
    release_kept()


# ---- model ---------------------------------------------------------------------------------------------------------
_TB = "down_blocks.0.attentions.0.transformer_blocks.0."
TOUCHED = [_TB + "attn1.to_q", _TB + "attn1.to_k",                        # fused Q | K | V buffer, softmax scale folded into to_k
           _TB + "attn2.to_k", _TB + "attn2.to_v",                        # text-context cache
           _TB + "ff.net.0.proj", _TB + "ff.net.2",                       # GEGLU interleave, plain matrix
           "down_blocks.0.attentions.0.proj_in",                          # 1x1 conv
           "down_blocks.1.resnets.0.conv1", "down_blocks.1.resnets.0.conv_shortcut", "down_blocks.1.resnets.0.time_emb_proj"]


def make_unet(seed=0):
    cfg = gcfg.tiny_unet()
    net = GyreHipUNet(cfg)
    net.load_state_dict(weights.synthetic_state_dict(weights.unet_param_shapes(cfg), seed))
    return net.to(DEV), cfg


def kohya(net, names=TOUCHED, r=4, seed=0, alpha_over_r=2.0 ** -5, lattice=True, amp=0.3):
    """A kohya-ss LoRA over `names`.  lattice: factors of lora_ref's lattice (delta = multiples of alpha / r, exact in fp32 next
    to any weight of this model); else normal factors."""
    params = dict(net.named_parameters())
    out = {}
    for i, name in enumerate(names):
        w = params[name + ".weight"]
        O, I = w.shape[:2]
        KH, KW = (w.shape[2], w.shape[3]) if w.ndim == 4 else (1, 1)
        if lattice:
            _, pairs, _ = LRF.lattice(O, I, (r,), KH, KW, conv=w.ndim == 4, seed=seed * 100 + i)
        else:
            _, pairs = LRF.gaussian(O, I, (r,), KH, KW, conv=w.ndim == 4, seed=seed * 100 + i)
            pairs = [(pairs[0][0] * amp / 0.2, pairs[0][1], 1.0)]
        k = "lora_unet_" + name.replace(".", "_")
        out[k + ".lora_up.weight"], out[k + ".lora_down.weight"] = _t(pairs[0][0]), _t(pairs[0][1])
        out[k + ".alpha"] = torch.tensor(alpha_over_r * r)
    out["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = torch.zeros(r, 8)     # ignored by the UNet
    out["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_up.weight"] = torch.zeros(8, r)
    return out


@pytest.fixture(scope="module")
def inputs():
    cfg = gcfg.tiny_unet()
    return (randn(2, 4, 16, 16, seed=1).to(DEV), torch.tensor([700, 30], device=DEV),
            randn(2, 77, cfg.cross_attention_dim, seed=2).to(DEV))


@pytest.fixture(scope="module")
def nets(inputs):
    """(device-path module, host-path module, base output): shared by the model tests, each of which leaves both bare."""
    a, _ = make_unet()
    b, _ = make_unet()
    x, t, ctx = inputs
    return a, b, a(x, t, encoder_hidden_states=ctx).sample.clone()


def fwd(net, inputs):
    x, t, ctx = inputs
    return net(x, t, encoder_hidden_states=ctx).sample.clone()


def test_attached_module_equals_the_host_merged_module(nets, inputs):
    a, b, base = nets
    lora = kohya(a)
    sd_before = {k: v.clone() for k, v in a.state_dict().items()}
    assert torch.equal(fwd(a, inputs), base)                        # the context tensor is cached from here on (same object below)
    assert LR.attach_lora(a, lora, "x", 0.5) == len(TOUCHED)
    got = fwd(a, inputs)
    assert not torch.equal(got, base), "stale weights or a stale text-context cache: the attach did not change the output"
    assert float((got - base).norm() / base.norm()) > 1e-2
    assert all(torch.equal(v, sd_before[k]) for k, v in a.state_dict().items())              # the masters are never written
    assert LR.apply_lora(b, lora, "x", 0.5) == len(TOUCHED)
    assert torch.equal(got, fwd(b, inputs))
    # re-scaling, and a second LoRA stacked on the same keys
    LR.set_attached_scale(a, "x", 0.25)
    LR.set_lora_scale(b, "x", 0.25)
    assert torch.equal(fwd(a, inputs), fwd(b, inputs))
    two = kohya(a, names=TOUCHED[:6], r=33, seed=1)
    LR.attach_lora(a, two, "y", 2.0)
    LR.apply_lora(b, two, "y", 2.0)
    stacked = fwd(a, inputs)
    assert torch.equal(stacked, fwd(b, inputs)) and not torch.equal(stacked, got)
    with pytest.raises(KeyError):
        LR.set_attached_scale(a, "nope", 1.0)
    LR.detach_loras(a)
    LR.remove_lora_from_model(b)
    assert torch.equal(fwd(a, inputs), base) and torch.equal(fwd(b, inputs), base)


def test_input_gradient_through_an_attached_lora(nets, inputs):
    """The transposed-weight copies of the reverse sweep follow the attach (and the detach)."""
    a, b, _ = nets
    x, t, ctx = inputs
    g = randn(*x.shape, seed=9).to(DEV)

    def grad(net):
        xi = x.clone().requires_grad_(True)
        out = net(xi, t, encoder_hidden_states=ctx).sample
        out.backward(g)
        return out.detach().clone(), xi.grad.clone()
    e0, g0 = grad(a)
    lora = kohya(a, seed=2)
    LR.attach_lora(a, lora, "x", 1.0)
    LR.apply_lora(b, lora, "x", 1.0)
    ea, ga = grad(a)
    eb, gb = grad(b)
    assert torch.equal(ea, eb) and torch.equal(ga, gb) and not torch.equal(ga, g0)
    LR.detach_loras(a)
    LR.remove_lora_from_model(b)
    e1, g1 = grad(a)
    assert torch.equal(e1, e0) and torch.equal(g1, g0)


def test_attached_lora_follows_to_and_is_dropped_by_load_state_dict(inputs):
    other = torch.float16 if HDT == torch.bfloat16 else torch.bfloat16
    a, _ = make_unet()
    b, _ = make_unet()
    lora = kohya(a, seed=3)
    LR.attach_lora(a, lora, "x", 0.5)
    a = a.to(other)                                                  # other storage flavour: new handle, full upload, LoRA re-applied
    b = b.to(other)
    LR.apply_lora(b, lora, "x", 0.5)                                 # host merge onto the same 16-bit masters (fp32 override)
    with_lora = fwd(a, inputs)
    assert torch.equal(with_lora, fwd(b, inputs))
    c = copy.deepcopy(a)                                             # a copy starts without attached LoRAs
    assert not getattr(c, "_lora_attached", None)
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    a.load_state_dict(sd)                                            # new weights: what was attached is gone
    bare = fwd(a, inputs)
    assert not a._lora_attached["loras"] and not torch.equal(bare, with_lora)
    assert torch.equal(fwd(c, inputs), bare)
    LR.remove_lora_from_model(b)
    assert torch.equal(fwd(b, inputs), bare)


def test_gaussian_lora_against_the_fp32_oracle(nets, inputs):
    from oracle import models_ref as M
    a, _, base = nets
    x, t, ctx = inputs
    lora = kohya(a, lattice=False, alpha_over_r=0.75, seed=4)
    merged = {k: v.detach().cpu().float().clone() for k, v in a.state_dict().items()}
    for name in TOUCHED:
        k = "lora_unet_" + name.replace(".", "_")
        merged[name + ".weight"] += LR.lora_delta(lora[k + ".lora_up.weight"], lora[k + ".lora_down.weight"], lora[k + ".alpha"]) * 0.8
    LR.attach_lora(a, lora, "g", 0.8)
    try:
        got = fwd(a, inputs)
        ref = M.unet_forward(merged, gcfg.tiny_unet(), x.cpu(), t.cpu(), ctx.cpu())
        report("tiny unet + attached LoRA", got.cpu(), ref, 3e-2)
        assert float((got - base).norm() / base.norm()) > 1e-2
    finally:
        LR.detach_loras(a)
    assert torch.equal(fwd(a, inputs), base)


def test_no_reupload(nets, inputs):
    """attach + forward + detach + forward: one gyre_unet_set_weight_delta per TOUCHED key each way, not one gyre_unet_set_weight,
    and no master parameter written."""
    a, _, base = nets
    L = a._L()
    fwd(a, inputs)
    calls = {"set_weight": 0, "lora_pairs": 0, "lora_restore": 0}
    orig_set, orig_lora = L.gyre_unet_set_weight, L.gyre_unet_set_weight_delta

    class CountSet:
        def __call__(self, *args):
            calls["set_weight"] += 1
            return orig_set(*args)

    class CountLora:
        def __call__(self, *args):
            calls["lora_pairs" if args[6] > 0 else "lora_restore"] += 1
            return orig_lora(*args)
    versions = {k: p._version for k, p in a.named_parameters()}
    L.gyre_unet_set_weight, L.gyre_unet_set_weight_delta = CountSet(), CountLora()
    try:
        LR.attach_lora(a, kohya(a, seed=5), "x", 1.0)
        with_lora = fwd(a, inputs)
        LR.detach_loras(a)
        after = fwd(a, inputs)
    finally:
        L.gyre_unet_set_weight, L.gyre_unet_set_weight_delta = orig_set, orig_lora
    k = len(TOUCHED)
    assert calls == {"set_weight": 0, "lora_pairs": k, "lora_restore": k}, calls
    assert k < len(list(a.named_parameters())) // 10
    assert versions == {n: p._version for n, p in a.named_parameters()}
    assert torch.equal(after, base) and not torch.equal(with_lora, base)


def test_zero_pairs_write_set_weight_bits_for_every_key(nets, inputs):
    """gyre_unet_set_weight_lora with no pairs, for EVERY matrix / convolution of the model (folded attention scale, fused
    buffers, GEGLU interleave, padded K included): the forward afterwards equals the one on gyre_unet_set_weight's own bits."""
    a, _, base = nets
    names = [n[:-len(".weight")] for n, p in a.named_parameters() if n.endswith(".weight") and p.ndim >= 2]
    assert len(names) > 100 and not getattr(a, "_lora_attached", {"loras": {}})["loras"]
    LR._issue(a, [n + ".weight" for n in names])
    assert torch.equal(fwd(a, inputs), base)


def test_errors(nets):
    a, b, _ = nets
    L, h = a._L(), C.c_void_p(a._handle)
    name = TOUCHED[0] + ".weight"
    w = dict(a.named_parameters())[name]

    def call(key, n_pairs=0, rank=4, shape=None):
        shape = tuple(w.shape) if shape is None else shape
        arr = (_lib.LoraPair * max(n_pairs, 1))()
        up, down = torch.zeros(w.shape[0], max(rank, 1), device=DEV), torch.zeros(max(rank, 1), w.shape[1], device=DEV)
        for j in range(n_pairs):
            arr[j].up, arr[j].down, arr[j].dtype, arr[j].rank, arr[j].scale = up.data_ptr(), down.data_ptr(), 0, rank, 1.0
        rc = L.gyre_unet_set_weight_lora(h, key.encode(), C.c_void_p(w.data_ptr()), _lib.dtype_code(w),
                                         (C.c_int64 * len(shape))(*shape), len(shape), n_pairs, arr, st())
        torch.cuda.synchronize()
        _lib.check(rc, L)
    with pytest.raises(KeyError):
        call("no.such.weight")
    with pytest.raises(KeyError):                                    # set_weight's own answer to a wrong shape
        call(name, shape=(w.shape[0], w.shape[1] + 8))
    with pytest.raises(ValueError):
        call(TOUCHED[0].replace("to_q", "to_out.0") + ".bias")       # a vector key
    with pytest.raises(ValueError):
        call(name, n_pairs=9)
    with pytest.raises(ValueError):
        call(name, n_pairs=1, rank=0)
    call(name)                                                       # zero pairs: fine, and the handle stays finalized
    k = "lora_unet_" + TOUCHED[0].replace(".", "_")
    good = kohya(a, names=TOUCHED[:1])
    bad_rank = dict(good); bad_rank[k + ".lora_up.weight"] = torch.zeros(w.shape[0], 5)
    bad_shape = dict(good); bad_shape[k + ".lora_down.weight"] = torch.zeros(4, w.shape[1] + 8)
    for bad in (bad_rank, bad_shape):
        with pytest.raises(ValueError):
            LR.attach_lora(a, bad, "x")
    for i in range(8):
        LR.attach_lora(a, good, i)
    with pytest.raises(ValueError):                                  # a ninth pair on one key
        LR.attach_lora(a, good, 8)
    assert len(a._lora_attached["loras"]) == 8
    with pytest.raises(ValueError):                                  # the two paths do not stack
        LR.apply_lora(a, good, "h")
    LR.detach_loras(a)
    stale = LR.Factors({name: LR.Term(_lib.DELTA_LORA, [(torch.zeros(w.shape[0] + 8, 4, device=DEV), torch.zeros(4, w.shape[1], device=DEV))], 1.0)},
                       a._handle_device)                           # factors uploaded for another model: refused before any call
    with pytest.raises(ValueError):
        LR.attach_lora(a, stale, "z")
    assert not a._lora_attached["loras"] and not a._dirty
    with pytest.raises(NotImplementedError):
        LR.attach_lora(a, {"unet:0:up": torch.zeros(1)}, "c")
    with pytest.raises(ValueError, match="Lycoris"):
        LR.attach_lora(a, {"a.lora_up.weight": torch.zeros(1), "a.hada_w1_a": torch.zeros(1)}, "c")
    LR.apply_lora(b, good, "h")
    with pytest.raises(ValueError):
        LR.attach_lora(b, good, "d")
    LR.remove_lora_from_model(b)
    cpu = GyreHipUNet(gcfg.tiny_unet())
    with pytest.raises(_lib.GyreError):
        LR.attach_lora(cpu, good, "x")


# ---- engine --------------------------------------------------------------------------------------------------------
def test_engine_lora_request(monkeypatch):
    from test_gpu_engine import build_engine, generators, sample_euler_ancestral, wrapper_kwargs
    ucfg, vcfg = gcfg.tiny_unet(), gcfg.tiny_vae()
    usd, _, eng = build_engine(ucfg, vcfg)
    _, _, host = build_engine(ucfg, vcfg)
    eng.scheduler = host.scheduler = sample_euler_ancestral
    req = lambda e, **kw: e(**wrapper_kwargs(prompt=["a photo of a cat"], generator=generators([11]), width=128, height=128,
                                             num_inference_steps=3, **kw))[0]
    plain = req(host)                                                # a never-patched engine
    lora = kohya(eng.unet, seed=6)
    merged = {k: v.clone() for k, v in usd.items()}
    for name in TOUCHED:                                             # merged on the host beforehand, as apply_lora merges
        k = "lora_unet_" + name.replace(".", "_")
        d = LR.lora_delta(lora[k + ".lora_up.weight"], lora[k + ".lora_down.weight"], lora[k + ".alpha"])
        merged[name + ".weight"] = merged[name + ".weight"].float() + d * 0.5
    host.unet.load_state_dict(merged)
    want = req(host)
    uploads = {"n": 0}
    orig = LR.upload_factors

    def counting(*a, **k):
        uploads["n"] += 1
        return orig(*a, **k)
    monkeypatch.setattr(LR, "upload_factors", counting)
    got = req(eng, lora=[(lora, {"unet": 0.5})])
    assert torch.equal(got, want) and not torch.equal(got, plain) and uploads["n"] == 1
    assert torch.equal(req(eng), plain)                              # the next request is bare again
    assert torch.equal(req(eng, lora=[(lora, {"unet": 0.5})]), want) and uploads["n"] == 1      # same mapping: no second upload
    assert not eng.unet._lora_state["loras"] and len(eng._lora_uploads) == 1
