"""gyre_op_merge_delta on the device (-m gpu): the row-major, output-typed delta merge a CLIP text encoder's weights get their
per-request adapters with (csrc/kernels_lyco.hip k_merge_delta), in BOTH storage libraries (picked here with _lib.lib(storage): the
output type is independent of the flavour) and for every output type x base type of fp32, bf16, fp16.

Yardsticks (tests/merge_delta_ref.py, checked on the CPU by tests/test_merge_delta_ref_host.py): on the LATTICE family every value
is exact in fp32 in any order and representable in all three types, so the kernel must equal the float64 reference computed from the
FILE tensors - and the host merge (lycoris.lyco_delta) - bit for bit; on GAUSSIAN data every element must stay inside the bound
derived from the kernel's stated operation order.  Zero terms copy base, LORA-only terms have gyre_op_repack_lora's bits, and a
refused call leaves a sentinel-filled output untouched."""
import itertools

import numpy as np
import pytest
import torch

import lora_ref as LRF
import lyco_ref as LY
import merge_delta_ref as MD
from gyre_amd import _lib, lycoris as LC
from gpu_util import DEV, release_kept, st, vp

pytestmark = pytest.mark.gpu

KIND = {"LORA": _lib.DELTA_LORA, "HADA": _lib.DELTA_HADA, "KRON": _lib.DELTA_KRON, "FULL": _lib.DELTA_FULL}
STORAGES = {"bf16lib": _lib.BF16, "f16lib": _lib.F16}
TYPES = (torch.float32, torch.bfloat16, torch.float16)
SENTINEL = 7.0


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def gpu_core(L):
    def core(c, r):
        A, B = c.shape[:2]
        T = int(np.prod(c.shape[2:])) if c.ndim > 2 else 1
        cd, rd = _t(c).to(DEV), _t(r).to(DEV)
        out = torch.zeros((A, r.shape[1], T), dtype=torch.float32, device=DEV)
        _lib.check(L.gyre_op_lyco_core(st(), vp(cd), 0, vp(rd), 0, A, B, r.shape[1], T, vp(out)), L)
        res = out.cpu().numpy()
        release_kept()
        return res
    return core


def fill_terms(L, shape, terms, pair_dtype=None, edit=None):
    arr = (_lib.DeltaTerm * max(len(terms), 1))()
    for j, (fields, user) in enumerate(terms):
        kind, ops, w1 = LY.lower(fields, shape, core=gpu_core(L))
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


def run_op(L, base, terms, bdt=torch.float32, odt=torch.float32, pair_dtype=None, edit=None, n_terms=None, I=None, out_code=None,
           alias=False):
    """gyre_op_merge_delta -> [O][I] tensor of odt (cpu); the output buffer is pre-filled with SENTINEL, so an element the kernel does
    not write shows.  I / out_code / alias: overrides for the refusal tests."""
    O, Ib = base.shape
    b = _t(base, bdt).to(DEV)
    arr = fill_terms(L, base.shape, terms, pair_dtype, edit)
    out = b if alias else torch.full((O, Ib), SENTINEL, dtype=odt, device=DEV)
    try:
        _lib.check(L.gyre_op_merge_delta(st(), vp(b), _lib.dtype_code(b), O, Ib if I is None else I,
                                         len(terms) if n_terms is None else n_terms, arr, vp(out),
                                         _lib.dtype_code(out) if out_code is None else out_code), L)
    finally:
        run_op.last = out.cpu()
        release_kept()
    return run_op.last


def host_merged(base, terms):
    """What the host path (text_adapters on a CPU encoder, lycoris.apply_lycoris) computes: base + lyco_delta * user scale, fp32."""
    w = _t(base).clone()
    for fields, user in terms:
        w = w + LC.lyco_delta({k: _t(np.asarray(v)) for k, v in fields.items()}, base.shape) * user
    return w


def quantized(terms, pair_dtype):
    """The file tensors as the kernel sees them when pair q of term j is held in 16 bits (references start from these values)."""
    out = []
    for j, (fields, user) in enumerate(terms):
        f = {}
        for k, v in fields.items():
            q = 1 if ("w2" in k or "t2" in k) and LY.kind_of(fields) == "loha" else 0
            f[k] = v if k in LY.SCALARS or k.startswith("lokr_w1") else MD.quantize(v, pair_dtype(j, q))
        out.append((f, user))
    return out


@pytest.fixture(params=list(STORAGES))
def L(request):
    return _lib.lib(STORAGES[request.param])


@pytest.mark.parametrize("case", MD.CASES, ids=MD.IDS)
def test_lattice_is_bit_exact(L, case):
    """== the float64 reference from the file tensors and == the host merge, for every output type x base type."""
    base, terms = MD.case_terms(case)
    ref = MD.ref64(base, terms)
    assert MD.on_lattice(ref)
    host = host_merged(base, terms)
    for bdt, odt in itertools.product(TYPES, TYPES):
        got = run_op(L, base, terms, bdt, odt)
        assert got.dtype == odt and np.array_equal(got.double().numpy(), ref), (case[0], bdt, odt)
        assert torch.equal(got, host.to(odt))


@pytest.mark.parametrize("case", MD.CASES, ids=MD.IDS)
def test_gaussian_within_the_bound(L, case):
    base32, terms = MD.case_terms(case, "gaussian")
    for bdt in TYPES:
        base = MD.quantize(base32, bdt)
        ref = MD.ref64(base, terms)
        for odt in TYPES:
            got = run_op(L, base, terms, bdt, odt)
            assert MD.worst_ratio(f"{case[0]} base {bdt} out {odt}", got, ref, MD.bound(base, terms, odt)) <= 1.0


MIXES = {"bf16": lambda j, q: torch.bfloat16, "f16": lambda j, q: torch.float16,
         "mixed_in_a_term": lambda j, q: (torch.bfloat16, torch.float16)[q] if j % 2 == 0 else (torch.float32, torch.bfloat16)[q]}


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("name", ["loha_r33_r4", "lokr_lowrank_r33", "four_terms", "eight_terms"])
def test_operand_dtypes(L, name, mix):
    """Factors in bf16 / fp16 / fp32, two dtypes inside one HADA term."""
    case, pd = MD.CASES[MD.IDS.index(name)], MIXES[mix]
    base, terms = MD.case_terms(case)                                      # lattice values are exact in every one of the types
    ref = MD.ref64(base, terms)
    for odt in TYPES:
        assert np.array_equal(run_op(L, base, terms, torch.float32, odt, pd).double().numpy(), ref)
    base, terms = MD.case_terms(case, "gaussian")
    terms = quantized(terms, pd)
    ref = MD.ref64(base, terms)
    for odt in TYPES:
        got = run_op(L, base, terms, torch.float32, odt, pd)
        assert MD.worst_ratio(f"{name} {mix} out {odt}", got, ref, MD.bound(base, terms, odt)) <= 1.0


@pytest.mark.parametrize("shape", [(40, 20), (64, 24), (130, 68)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_terms_copy_base_bit_for_bit(L, shape):
    for dt in TYPES:
        base = LY.gaussian_base(*shape, seed=3) * 40
        base[0, :4] = (-0.0, 0.0, 65504.0, -1.0)
        b = _t(base, dt)
        got = run_op(L, b.float().numpy(), [], dt, dt)
        ints = torch.int32 if dt == torch.float32 else torch.int16
        assert torch.equal(got.view(ints), b.view(ints)), dt


@pytest.mark.parametrize("shape", [(40, 20, (1, 4, 33)), (64, 24, (130,)), (130, 68, (4,)), (72, 12, (33, 4))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lora_terms_have_the_bits_of_repack_lora(L, shape):
    """LORA terms only, gaussian data (every rounding matters), output in the library's own storage type: bit-identical to
    gyre_op_repack_lora with I_pad = I and scale_p = 1 (a multiplication by one changes nothing)."""
    O, I, ranks = shape
    hdt = _lib.STORAGE_TORCH_DTYPE[L.gyre_storage_dtype()]
    base, pairs = LRF.gaussian(O, I, ranks, seed=21)
    terms = [({"lora_up.weight": up, "lora_down.weight": down, "scale": np.float32(s)}, 1.0) for up, down, s in pairs]
    got = run_op(L, base, terms, torch.float32, hdt)
    b = _t(base).to(DEV)
    arr = (_lib.LoraPair * len(pairs))()
    for j, (up, down, s) in enumerate(pairs):
        u, d = _t(up).to(DEV), _t(down).to(DEV)
        arr[j].up, arr[j].down, arr[j].dtype, arr[j].rank, arr[j].scale = vp(u).value, vp(d).value, 0, down.shape[0], float(np.float32(s))
    out = torch.ones(O * I, dtype=hdt, device=DEV)
    _lib.check(L.gyre_op_repack_lora(st(), vp(b), 0, O, I, 1, 1, I, 0, 1.0, len(pairs), arr, vp(out)), L)
    want = out.cpu().reshape(O, I)
    release_kept()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_refused_calls_write_nothing(L):
    case = MD.CASES[MD.IDS.index("four_terms")]                            # LORA, HADA, KRON, FULL on 72 x 12
    base, terms = MD.case_terms(case)

    def refused(odt=torch.bfloat16, **kw):
        with pytest.raises(ValueError):
            run_op(L, kw.pop("base", base), kw.pop("terms", terms), torch.float32, odt, **kw)
        assert bool((run_op.last == SENTINEL).all()), "a refused call wrote to the output"
    for odt in TYPES:
        refused(odt, terms=terms * 3, n_terms=9)                           # more than 8 terms
        refused(odt, edit=lambda a: a[0].rank.__setitem__(0, 0))           # LORA: rank 0
        refused(odt, edit=lambda a: a[3].down.__setitem__(0, None))        # FULL: null diff
        refused(odt, I=10)                                                 # I % 4 != 0 (the buffers hold 12 columns)
        refused(odt, edit=lambda a: setattr(a[2], "O1", 5))                # KRON: 5 does not divide 72
    refused(edit=lambda a: a[1].rank.__setitem__(1, 0))                    # HADA: second rank 0
    refused(edit=lambda a: a[1].up.__setitem__(1, None))                   # HADA: null second up
    refused(edit=lambda a: setattr(a[2], "w1", None))                      # KRON: null w1
    refused(edit=lambda a: setattr(a[2], "I1", 5))                         # KRON: 5 does not divide 12
    refused(edit=lambda a: setattr(a[2], "I1", 0))
    refused(edit=lambda a: setattr(a[0], "kind", 7))
    refused(edit=lambda a: a[0].dtype.__setitem__(0, 3))
    refused(out_code=3)                                                    # no such output type
    refused(base=LY.lattice_base(72, 10), terms=[])                        # a 10-column matrix
    # out is base: refused, and base keeps its values
    with pytest.raises(ValueError):
        run_op(L, base, terms, torch.float32, torch.float32, alias=True)
    assert torch.equal(run_op.last, _t(base))
    # ... as is an output that is an operand
    d = torch.full((72, 12), SENTINEL, device=DEV)
    arr = (_lib.DeltaTerm * 1)()
    arr[0].kind, arr[0].scale, arr[0].down[0], arr[0].dtype[0] = _lib.DELTA_FULL, 1.0, d.data_ptr(), 0
    b = _t(base).to(DEV)
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_merge_delta(st(), vp(b), 0, 72, 12, 1, arr, vp(d), 0), L)
    release_kept()
    assert bool((d == SENTINEL).all())
