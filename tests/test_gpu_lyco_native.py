"""Per-request LyCORIS on the device (-m gpu): the fused term repack (gyre_op_repack_delta), the core contraction
(gyre_op_lyco_core), the store entry (gyre_unet_set_weight_delta), the module path (lycoris.attach_lycoris / attach_adapters, the
registry it shares with lora.attach_lora) and the engine's ``lora=`` routing.

Yardsticks (tests/lyco_ref.py, checked on the CPU by tests/test_lyco_ref_host.py): on the LATTICE family every value is exact in
fp32 in any order and representable in the storage type, so the kernels must equal the float64 reference computed from the FILE
tensors - and the plain repack of the host-merged tensor (lycoris.lyco_delta) - bit for bit; on GAUSSIAN data they must stay inside
the bound derived from the kernels' stated operation order.  The operands are prepared the way lycoris.upload_factors prepares them
(lyco_ref.lower with the device core operator).  Model tests compare the attached module with a second module that got the same
file through the host merge (apply_lycoris).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import lora_ref as LRF
import lyco_ref as LY
from gyre_amd import _lib, config as gcfg, lora as LR, lycoris as LC
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV, HDT, randn, release_kept, st, vp
from test_gpu_lora_native import TOUCHED, _t, fwd, kohya, make_unet, plain_repack
from test_gpu_lora_native import run_op as run_lora_op

pytestmark = pytest.mark.gpu

KIND = {"LORA": _lib.DELTA_LORA, "HADA": _lib.DELTA_HADA, "KRON": _lib.DELTA_KRON, "FULL": _lib.DELTA_FULL}
IDS = [c[0] for c in LY.CASES]


def gpu_core(core, right, core_dtype=torch.float32, right_dtype=torch.float32):
    """gyre_op_lyco_core on device copies -> numpy fp32 [A, C, T]"""
    L = _lib.lib()
    A, B = core.shape[:2]
    T = int(np.prod(core.shape[2:])) if core.ndim > 2 else 1
    c, r = _t(core, core_dtype).to(DEV), _t(right, right_dtype).to(DEV)
    out = torch.full((A, right.shape[1], T), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(L.gyre_op_lyco_core(st(), vp(c), _lib.dtype_code(c), vp(r), _lib.dtype_code(r), A, B, right.shape[1], T, vp(out)))
    res = out.cpu().numpy()
    release_kept()
    return res


def fill_terms(base_shape, terms, pair_dtype=None, edit=None):
    """(DeltaTerm array, n) for file terms, operands lowered with the device core operator; pair_dtype(j, q): the torch dtype of
    pair q of term j (default fp32); edit(arr): a last change to the array (bad-argument tests)."""
    arr = (_lib.DeltaTerm * max(len(terms), 1))()
    for j, (fields, user) in enumerate(terms):
        kind, ops, w1 = LY.lower(fields, base_shape, core=gpu_core)
        arr[j].kind, arr[j].scale = KIND[kind], float(user) * LY.file_scale(fields)
        for q, (up, down) in enumerate(ops):
            dt = pair_dtype(j, q) if pair_dtype else torch.float32
            d = _t(down, dt).to(DEV)
            arr[j].down[q], arr[j].dtype[q], arr[j].rank[q] = vp(d).value, _lib.dtype_code(d), 0
            if up is not None:
                arr[j].up[q], arr[j].rank[q] = vp(_t(up, dt).to(DEV)).value, up.shape[1]
        if w1 is not None:
            arr[j].w1, arr[j].O1, arr[j].I1 = vp(_t(w1).to(DEV)).value, w1.shape[0], w1.shape[1]
    if edit:
        edit(arr)
    return arr


def run_op(base, terms, I_pad, geglu, scale_p, base_dtype=torch.float32, pair_dtype=None, edit=None, n_terms=None):
    """gyre_op_repack_delta -> [O][KH][KW][I_pad] tensor of HDT (cpu); the output buffer is pre-filled with ones, so an element the
    kernel does not write (pad columns included) shows."""
    L = _lib.lib()
    O, I, KH, KW = LY._shape(base)
    b = _t(base, base_dtype).to(DEV)
    arr = fill_terms(base.shape, terms, pair_dtype, edit)
    out = torch.ones(O * KH * KW * I_pad, dtype=HDT, device=DEV)
    try:
        _lib.check(L.gyre_op_repack_delta(st(), vp(b), _lib.dtype_code(b), O, I, KH, KW, I_pad, int(geglu), scale_p,
                                          len(terms) if n_terms is None else n_terms, arr, vp(out)))
    finally:
        run_op.last = out.cpu().reshape(O, KH, KW, I_pad)
        release_kept()
    return run_op.last


def host_merged(base, terms):
    """What apply_lycoris hands to the upload: base + lyco_delta * user scale, fp32, in term order."""
    w = _t(base).clone()
    for fields, user in terms:
        w = w + LC.lyco_delta({k: _t(np.asarray(v)) for k, v in fields.items()}, base.shape) * user
    return w.numpy()


def quantized(terms, pair_dtype):
    """The file tensors as the kernel sees them when pair q of term j is stored in 16 bits (references start from these values)."""
    out = []
    for j, (fields, user) in enumerate(terms):
        f = {}
        for k, v in fields.items():
            q = 1 if ("w2" in k or "t2" in k) and LY.kind_of(fields) == "loha" else 0
            f[k] = v if k in LY.SCALARS or k.startswith("lokr_w1") else _t(v, pair_dtype(j, q)).float().numpy()
        out.append((f, user))
    return out


# ---- operators -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LY.CASES, ids=IDS)
def test_operator_lattice_is_bit_exact(case):
    """== the float64 reference from the file tensors, == the plain repack of the host-merged fp32 tensor, pad columns zero."""
    name, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    base, terms = LY.case_terms(case)
    ref = LY.ref64(base, terms, I_pad, geglu, scale_p)
    assert LY.on_lattice(ref)
    got = run_op(base, terms, I_pad, geglu, scale_p)
    assert np.array_equal(got.double().numpy(), ref), name
    assert not got[..., I:].any()
    host = plain_repack(host_merged(base, terms) * np.float32(scale_p), I_pad, geglu)            # (scale_p: a power of two here)
    assert torch.equal(got, host)


@pytest.mark.parametrize("case", LY.CASES, ids=IDS)
def test_operator_gaussian_within_the_bound(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    sp = scale_p if scale_p == 1.0 else 0.1803
    base, terms = LY.case_terms(case, "gaussian")
    got = run_op(base, terms, I_pad, geglu, sp)
    ratio = LY.worst_ratio(name, got, LY.ref64(base, terms, I_pad, geglu, sp), LY.bound(base, terms, I_pad, geglu, sp, HDT))
    assert ratio <= 1.0 and not got[..., I:].any()


MIXES = {"bf16": lambda j, q: torch.bfloat16, "f16": lambda j, q: torch.float16,
         "mixed_in_a_term": lambda j, q: (torch.bfloat16, torch.float16)[q] if j % 2 == 0 else (torch.float32, torch.bfloat16)[q]}


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("bdt", [torch.float32, HDT], ids=["base_f32", "base_storage"])
@pytest.mark.parametrize("name", ["loha_conv_r33_r4", "lokr_lowrank_conv_pad_r33", "mixed_half"])
def test_operator_dtypes(name, bdt, mix):
    """Factors in bf16 / fp16 / fp32, two dtypes inside one HADA term; base in fp32 and in the storage type."""
    case = LY.CASES[IDS.index(name)]
    _, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    pd = MIXES[mix]
    base, terms = LY.case_terms(case)                                      # lattice values are exact in every one of the types
    got = run_op(base, terms, I_pad, geglu, scale_p, bdt, pd)
    assert np.array_equal(got.double().numpy(), LY.ref64(base, terms, I_pad, geglu, scale_p))
    base, terms = LY.case_terms(case, "gaussian")
    base, terms = _t(base, bdt).float().numpy(), quantized(terms, pd)
    got = run_op(base, terms, I_pad, geglu, 0.1803, bdt, pd)
    assert LY.worst_ratio(f"{name} {mix}", got, LY.ref64(base, terms, I_pad, geglu, 0.1803),
                          LY.bound(base, terms, I_pad, geglu, 0.1803, HDT)) <= 1.0


BIT_SHAPES = [(72, 12, 3, 3, 16, False, (33, 4)), (64, 24, 1, 1, 24, True, (130,)), (40, 20, 1, 1, 24, False, (1, 4, 33))]
BIT_IDS = ["conv_pad", "geglu_r130", "matrix_pad"]


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_lora_terms_have_the_bits_of_repack_lora(shape):
    """LORA terms only, gaussian data (every rounding matters): bit-identical to gyre_op_repack_lora."""
    O, I, KH, KW, I_pad, geglu, ranks = shape
    base, pairs = LRF.gaussian(O, I, ranks, KH, KW, seed=21)
    terms = [({"lora_up.weight": up, "lora_down.weight": down, "scale": np.float32(s)}, 1.0) for up, down, s in pairs]
    pairs = [(up, down, float(np.float32(s))) for up, down, s in pairs]
    got = run_op(base, terms, I_pad, geglu, 0.1803)
    assert torch.equal(got.view(torch.int16), run_lora_op(base, pairs, I_pad, geglu, 0.1803).view(torch.int16))


@pytest.mark.parametrize("bdt", [torch.float32, HDT], ids=["base_f32", "base_storage"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=BIT_IDS)
def test_operator_instantiations_agree(shape, bdt):
    """launch_repack_delta runs the LoRA-only instantiation of the kernel when every term is a LORA term and the general one
    otherwise; on the same LORA terms the two must write the same bits.  The second call appends one FULL term whose diff is all
    zeros at scale 1, which takes the general instantiation and adds fma(1, 0, acc) = acc to every element (exact unless acc is -0,
    which gaussian data does not give; pad columns are written as +0 by both).  The shapes cover a partial row tile, pad columns,
    the GEGLU interleave, ranks 1 and 33 around the 32-wide rank chunk and several terms.  The opposite mistake, a HADA or KRON
    call sent to the LoRA-only instantiation, would compute those terms as low-rank products: the lattice cases of LY.CASES
    (test_operator_lattice_is_bit_exact) already fail on that."""
    O, I, KH, KW, I_pad, geglu, ranks = shape
    base, pairs = LRF.gaussian(O, I, ranks, KH, KW, seed=21)
    terms = [({"lora_up.weight": up, "lora_down.weight": down, "scale": np.float32(s)}, 1.0) for up, down, s in pairs]
    zero = ({"diff": np.zeros(base.shape, np.float32), "scale": np.float32(1.0)}, 1.0)
    lora_only = run_op(base, terms, I_pad, geglu, 0.1803, bdt)
    general = run_op(base, terms + [zero], I_pad, geglu, 0.1803, bdt)
    assert torch.equal(lora_only.view(torch.int16), general.view(torch.int16))
    assert bool(lora_only[..., :I].any()) and not lora_only[..., I:].any()


@pytest.mark.parametrize("shape", [(256, 256, 3, 3), (320, 250, 1, 1), (64, 24, 1, 1)], ids=["conv3x3", "matrix_padded_k", "geglu"])
def test_zero_terms_are_the_plain_and_the_folded_scale_repack(shape):
    L = _lib.lib()
    O, I, KH, KW = shape
    geglu = shape == (64, 24, 1, 1)
    I_pad = I if geglu else (I + 7) // 8 * 8
    base = LY.gaussian_base(O, I, KH, KW, seed=3)
    assert torch.equal(run_op(base, [], I_pad, geglu, 1.0), plain_repack(base, I_pad, geglu))
    if geglu:
        return
    scale = 0.22808579                                                     # the softmax scale the store folds into to_k
    got = run_op(base, [], I_pad, False, scale)
    src = _t(base).to(DEV)
    out = torch.ones(O * KH * KW * I_pad, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_repack_conv_weight_scaled(st(), vp(src), 0, O, I, KH, KW, I_pad, scale, vp(out)))
    want = out.cpu().reshape(O, KH, KW, I_pad)
    release_kept()
    differ = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert differ == 0, f"{differ} of {got.numel()} packed elements differ from the plain repack"


@pytest.mark.parametrize("shape", [(5, 7, 9, (3, 3)), (3, 130, 300, ()), (1, 1, 1, ())], ids=["tucker", "matrix_many_blocks", "one"])
@pytest.mark.parametrize("dts", [(torch.float32, torch.float32), (torch.bfloat16, torch.float16)], ids=["f32", "bf16_x_f16"])
def test_core_operator(shape, dts):
    A, B, Cn, tail = shape
    g = np.random.default_rng(A + B)
    core = _t(g.standard_normal((A, B, *tail)).astype(np.float32), dts[0]).float().numpy()
    right = _t(g.standard_normal((B, Cn)).astype(np.float32), dts[1]).float().numpy()
    got = gpu_core(core, right, *dts).astype(np.float64)
    want = LY.core64(core, right)
    tol = B * LY.U32 * LY.core64(np.abs(core), np.abs(right)) * (1 + 2.0 ** -10)      # B fmas, partial sums bounded by the abs sum
    ratio = float(np.max(np.abs(got - want) / tol))
    print(f"[lyco core] {shape} {dts}: worst |err| / tol = {ratio:.3g}")
    assert got.shape == want.shape and ratio <= 1.0
    assert np.array_equal(got, LY.core_emulate(core, right).astype(np.float64))        # the stated order, bit for bit
    L = _lib.lib()
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_lyco_core(st(), None, 0, None, 0, A, B, Cn, 1, None))
    c = torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_lyco_core(st(), vp(c), 0, vp(c), 0, 1, 0, 1, 1, vp(c)))
    release_kept()


def test_operator_refuses_bad_arguments_and_writes_nothing():
    case = LY.CASES[IDS.index("mixed_half")]
    _, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    base, terms = LY.case_terms(case)

    def refused(**kw):
        with pytest.raises(ValueError):
            run_op(base, kw.pop("terms", terms), kw.pop("I_pad", I_pad), kw.pop("geglu", False), 1.0, **kw)
        assert bool((run_op.last == 1).all()), "a refused call wrote to the output"
    refused(terms=terms * 3, n_terms=9)                                    # more than 8 terms
    refused(edit=lambda a: setattr(a[0], "kind", 7))                       # unknown kind
    refused(edit=lambda a: a[0].rank.__setitem__(0, 0))                    # LORA: rank 0
    refused(edit=lambda a: a[1].rank.__setitem__(1, 0))                    # HADA: second rank 0
    refused(edit=lambda a: a[1].up.__setitem__(1, None))                   # HADA: null second up
    refused(edit=lambda a: a[3].down.__setitem__(0, None))                 # FULL: null diff
    refused(edit=lambda a: setattr(a[2], "w1", None))                      # KRON: null w1
    refused(edit=lambda a: setattr(a[2], "O1", 5))                         # KRON: 5 does not divide 72
    refused(edit=lambda a: setattr(a[2], "I1", 0))
    refused(edit=lambda a: a[2].rank.__setitem__(0, -1))
    refused(edit=lambda a: a[0].dtype.__setitem__(0, 3))
    refused(I_pad=10)                                                      # I_pad < I
    refused(geglu=True)                                                    # GEGLU needs a matrix with O % 32 == 0


# ---- model -----------------------------------------------------------------------------------------------------------
_TB = "down_blocks.0.attentions.0.transformer_blocks.0."
# one file mixing all forms: attention (fused Q | K | V buffer, softmax scale folded into to_k, text-context cache), feed-forward incl.
# the GEGLU projection, resnet 3x3 convs and 1x1 convs
TARGETS = [(_TB + "attn1.to_q", "loha", dict(rank=4)),
           (_TB + "attn1.to_k", "lokr_lowrank", dict(rank=4, kron=(4, 2))),
           (_TB + "attn2.to_k", "lokr_dense", dict(kron=(2, 4))),
           (_TB + "attn2.to_v", "full", {}),
           (_TB + "ff.net.0.proj", "loha", dict(rank=33, rank2=4, scale_rule="scale")),
           (_TB + "ff.net.2", "lokr_w1_lowrank", dict(rank=4, kron=(4, 8))),
           ("down_blocks.0.attentions.0.proj_in", "lokr_lowrank", dict(rank=4, kron=(2, 2))),
           ("down_blocks.1.resnets.0.conv1", "loha_t", dict(rank=4)),
           ("down_blocks.1.resnets.0.conv2", "locon_mid", dict(rank=4)),
           ("mid_block.resnets.0.conv1", "lokr_t", dict(rank=4, kron=(4, 4))),
           ("mid_block.resnets.0.conv2", "lora", dict(rank=33)),
           ("down_blocks.1.resnets.0.conv_shortcut", "full", {}),
           ("down_blocks.1.resnets.0.time_emb_proj", "lokr_dense", dict(kron=(8, 2)))]


def lyco_file(net, targets=TARGETS, seed=0, shrink=2.0 ** -4):
    """A LyCORIS file over `targets` with lyco_ref's lattice tensors: every delta is a multiple of a power of two, exact in fp32
    next to any weight of this model, and small next to the weights."""
    params = dict(net.named_parameters())
    out = {}
    for i, (name, form, kw) in enumerate(targets):
        w = params[name + ".weight"]
        KH, KW = (w.shape[2], w.shape[3]) if w.ndim == 4 else (1, 1)
        f = LY.lattice_fields(form, w.shape[0], w.shape[1], KH, KW, seed=seed * 100 + i, shrink=shrink, **kw)
        k = "lora_unet_" + name.replace(".", "_")
        out.update({f"{k}.{p}": _t(np.asarray(v)) for p, v in f.items()})
    out["lora_te_text_model_encoder_layers_0_mlp_fc1.hada_w1_a"] = torch.zeros(8, 2)        # ignored by the UNet
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
    return a, b, fwd(a, inputs)


class Counter:
    """Counts the repack calls of a library by key while it is installed."""

    def __init__(self, L):
        self.L, self.calls = L, []
        self.orig = {n: getattr(L, n) for n in ("gyre_unet_set_weight", "gyre_unet_set_weight_lora", "gyre_unet_set_weight_delta")}

    def __enter__(self):
        for n, f in self.orig.items():
            setattr(self.L, n, (lambda n, f: lambda *a: (self.calls.append((n[len("gyre_unet_"):], a[1].decode(), a[6] if len(a) > 7 else None)), f(*a))[1])(n, f))
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(self.L, n, f)


def test_attached_lycoris_equals_the_host_merged_module(nets, inputs):
    a, b, base = nets
    lyco = lyco_file(a)
    sd_before = {k: v.clone() for k, v in a.state_dict().items()}
    assert torch.equal(fwd(a, inputs), base)
    assert LC.attach_lycoris(a, lyco, "x", 0.5) == len(TARGETS)
    got = fwd(a, inputs)
    assert not torch.equal(got, base) and float((got - base).norm() / base.norm()) > 1e-2 and bool(torch.isfinite(got).all())
    assert all(torch.equal(v, sd_before[k]) for k, v in a.state_dict().items())              # the masters are never written
    assert LC.apply_lycoris(b, lyco, "x", 0.5) == len(TARGETS)
    assert torch.equal(got, fwd(b, inputs))
    LR.set_attached_scale(a, "x", 0.25)
    LR.set_lora_scale(b, "x", 0.25)
    assert torch.equal(fwd(a, inputs), fwd(b, inputs))
    with pytest.raises(ValueError):                                  # the two paths do not stack
        LC.apply_lycoris(a, lyco, "h")
    with pytest.raises(ValueError):
        LC.attach_lycoris(b, lyco, "d")
    LR.detach_loras(a)
    LR.remove_lora_from_model(b)
    assert torch.equal(fwd(a, inputs), base) and torch.equal(fwd(b, inputs), base)


def test_lora_and_lycoris_share_a_weight_one_repack_per_key(nets, inputs):
    a, b, base = nets
    targets = TARGETS[2:]                                            # attn1.to_q / to_k stay LoRA-only
    lyco, lora = lyco_file(a, targets, seed=1), kohya(a, seed=7)
    lyco_keys = {n + ".weight" for n, _, _ in targets}
    lora_keys = {n + ".weight" for n in TOUCHED}
    shared = lyco_keys & lora_keys
    assert len(shared) >= 4 and lora_keys - lyco_keys and lyco_keys - lora_keys
    fwd(a, inputs)
    with Counter(a._L()) as c:
        assert LC.attach_adapters(a, [(lyco, "l", 0.5), (lora, "k", 0.5)]) == [len(targets), len(TOUCHED)]
        got = fwd(a, inputs)
        attach, c.calls[:] = list(c.calls), []
        LR.detach_loras(a)
        bare = fwd(a, inputs)
    keys = [k for _, k, _ in attach]
    assert sorted(keys) == sorted(lyco_keys | lora_keys), "one repack per touched weight"
    assert all(f == "set_weight_delta" for f, _, _ in attach), "every key goes through the one entry, never gyre_unet_set_weight"
    assert {k: n for _, k, n in attach} == {k: (k in lyco_keys) + (k in lora_keys) for k in lyco_keys | lora_keys}      # pairs + terms that hit it
    assert sorted(k for _, k, _ in c.calls) == sorted(lyco_keys | lora_keys) and all(f == "set_weight_delta" and n == 0 for f, _, n in c.calls)
    LC.apply_lycoris(b, lyco, "l", 0.5)                              # the same order on the host
    LR.apply_lora(b, lora, "k", 0.5)
    assert torch.equal(got, fwd(b, inputs)) and not torch.equal(got, base)
    LR.remove_lora_from_model(b)
    assert torch.equal(bare, base) and torch.equal(fwd(b, inputs), base)


def test_attached_lycoris_follows_to_and_is_dropped_by_load_state_dict(inputs):
    other = torch.float16 if HDT == torch.bfloat16 else torch.bfloat16
    a, _ = make_unet()
    b, _ = make_unet()
    lyco = lyco_file(a, seed=3)
    LC.attach_lycoris(a, lyco, "x", 0.5)
    a = a.to(other)                                                  # other storage flavour: new handle, full upload, terms re-applied
    b = b.to(other)
    LC.apply_lycoris(b, lyco, "x", 0.5)
    with_lyco = fwd(a, inputs)
    assert torch.equal(with_lyco, fwd(b, inputs))
    c = copy.deepcopy(a)                                             # a copy starts without attached adapters
    assert not getattr(c, "_lora_attached", None)
    a.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    bare = fwd(a, inputs)
    assert not a._lora_attached["loras"] and not torch.equal(bare, with_lyco)
    assert torch.equal(fwd(c, inputs), bare)
    LR.remove_lora_from_model(b)
    assert torch.equal(fwd(b, inputs), bare)


def test_errors(nets, inputs):
    a, _, base = nets
    L, h = a._L(), C.c_void_p(a._handle)
    name = TARGETS[1][0] + ".weight"                                 # attn1.to_k, 32 x 32
    w = dict(a.named_parameters())[name]
    ops = torch.zeros(64 * 64, device=DEV)

    def call(key, edit=None, n=1):
        arr = (_lib.DeltaTerm * 9)()
        for j in range(9):
            arr[j].kind, arr[j].scale = _lib.DELTA_KRON, 1.0
            arr[j].up[0], arr[j].down[0], arr[j].w1 = ops.data_ptr(), ops.data_ptr(), ops.data_ptr()
            arr[j].rank[0], arr[j].O1, arr[j].I1 = 4, 4, 2
        if edit:
            edit(arr[0])
        rc = L.gyre_unet_set_weight_delta(h, key.encode(), C.c_void_p(w.data_ptr()), _lib.dtype_code(w),
                                          (C.c_int64 * 2)(*w.shape), 2, n, arr, st())
        torch.cuda.synchronize()
        _lib.check(rc, L)
    with pytest.raises(KeyError):
        call("no.such.weight")
    with pytest.raises(ValueError):
        call(TARGETS[0][0].replace("to_q", "to_out.0") + ".bias")    # a vector key
    with pytest.raises(ValueError):
        call(name, n=9)
    with pytest.raises(ValueError):
        call(name, lambda t: t.up.__setitem__(0, None))              # null operand
    with pytest.raises(ValueError):
        call(name, lambda t: setattr(t, "kind", _lib.DELTA_HADA))    # rank < 1 where a rank is needed (second pair)
    with pytest.raises(ValueError):
        call(name, lambda t: setattr(t, "O1", 5))                    # 5 x O2 is not 32
    assert torch.equal(fwd(a, inputs), base), "a refused call changed the native copy"
    call(name, n=0)                                                  # zero terms: fine, the base bits, the handle stays finalized
    a._ctx_slots = []                                                # (what lora._issue does after its calls: the library dropped its contexts)
    assert torch.equal(fwd(a, inputs), base)
    # a ninth term on one key: ValueError, the registry as it was
    one = lyco_file(a, targets=TARGETS[:1])
    for i in range(8):
        LC.attach_lycoris(a, one, i)
    with pytest.raises(ValueError):
        LC.attach_lycoris(a, one, 8)
    with pytest.raises(ValueError):
        LR.attach_lora(a, kohya(a, names=TOUCHED[:1]), "ninth")      # (attn1.to_q: the same key)
    assert list(a._lora_attached["loras"]) == list(range(8)) and not a._dirty
    LR.detach_loras(a)
    assert torch.equal(fwd(a, inputs), base)
    stale = LC.Factors({name: LC.Term(_lib.DELTA_FULL, [(None, torch.zeros(40, 32, device=DEV))], 1.0)}, a._handle_device)
    with pytest.raises(ValueError):                                  # terms uploaded for another model: refused before any call
        LC.attach_lycoris(a, stale, "z")
    assert not a._lora_attached["loras"] and not a._dirty
    with pytest.raises(NotImplementedError):
        LC.attach_lycoris(a, {"lora_unet_" + TARGETS[0][0].replace(".", "_") + ".weight": torch.zeros(32)}, "ia3")
    with pytest.raises(ValueError):                                  # lora's own entry point still refuses the mapping
        LR.attach_lora(a, one, "c")
    cpu = GyreHipUNet(gcfg.tiny_unet())
    with pytest.raises(_lib.GyreError):
        LC.attach_lycoris(cpu, one, "x")


# ---- engine ----------------------------------------------------------------------------------------------------------
def test_engine_lycoris_request(monkeypatch):
    from test_gpu_engine import build_engine, generators, sample_euler_ancestral, wrapper_kwargs
    ucfg, vcfg = gcfg.tiny_unet(), gcfg.tiny_vae()
    usd, _, eng = build_engine(ucfg, vcfg)
    _, _, host = build_engine(ucfg, vcfg)
    eng.scheduler = host.scheduler = sample_euler_ancestral
    req = lambda e, **kw: e(**wrapper_kwargs(prompt=["a photo of a cat"], generator=generators([11]), width=128, height=128,
                                             num_inference_steps=3, **kw))[0]
    plain = req(host)                                                # a never-patched engine
    lyco, lora = lyco_file(eng.unet, seed=6), kohya(eng.unet, seed=6)
    merged = {k: v.clone().float() for k, v in usd.items()}
    for mod, fields in LC._modules(eng.unet, lyco):                  # merged on the host beforehand, in request order
        merged[mod] = merged[mod] + LC.lyco_delta(fields, merged[mod].shape) * 0.5
    for name in TOUCHED:
        k = "lora_unet_" + name.replace(".", "_")
        merged[name + ".weight"] = merged[name + ".weight"] + \
            LR.lora_delta(lora[k + ".lora_up.weight"], lora[k + ".lora_down.weight"], lora[k + ".alpha"]) * 1.0
    host.unet.load_state_dict(merged)
    want = req(host)
    uploads = {"lyco": 0, "lora": 0}
    orig_lc, orig_lr = LC.upload_factors, LR.upload_factors
    monkeypatch.setattr(LC, "upload_factors", lambda *a, **k: (uploads.__setitem__("lyco", uploads["lyco"] + 1), orig_lc(*a, **k))[1])
    monkeypatch.setattr(LR, "upload_factors", lambda *a, **k: (uploads.__setitem__("lora", uploads["lora"] + 1), orig_lr(*a, **k))[1])
    request = [(lyco, {"unet": 0.5}), (lora, {})]
    got = req(eng, lora=request)
    assert torch.equal(got, want) and not torch.equal(got, plain) and uploads == {"lyco": 1, "lora": 1}
    assert torch.equal(req(eng), plain)                              # the next request is bare again
    assert torch.equal(req(eng, lora=request), want) and uploads == {"lyco": 1, "lora": 1}      # same mappings: nothing uploaded
    assert not eng.unet._lora_state["loras"] and len(eng._lora_uploads) == 2
