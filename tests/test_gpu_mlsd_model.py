"""The native MLSD line detector (-m gpu; model_mlsd.hip behind gyre_amd.hinters.GyreHipMLSD) against the fp64 restatement of the net
(tests/mlsd_ref.py, itself held to the reference's own module by tests/test_reference_mlsd.py and to its stored outputs by
tests/test_mlsd_ref_host.py), in both storage flavours; two forwards; batch independence; input dtypes; workspace sizing; refusals."""
import ctypes as C

import pytest
import torch

import mlsd_ref as R
from gyre_amd import _lib
from gyre_amd.hinters import GyreHipMLSD
from gpu_util import DEV
# (max-abs, rel-L2) of the CPU emulation that folds the BatchNorms as the native path does and rounds every stored tensor to the
# storage type, against the fp64 net, per mlsd_ref.MODEL_CASES entry (measured, printed and re-checked by
# tests/test_mlsd_ref_host.py::test_storage_emulation_distance).  The gate is twice that, the factor of the HED, line-art and upscaler
# model tests.
from test_mlsd_ref_host import EMULATION

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
_MODEL = {}


def _model(sdt):
    """one module per flavour for the whole file: the weights are the same in every case"""
    if sdt not in _MODEL:
        m = GyreHipMLSD()
        m.load_state_dict(R.model_weights())
        _MODEL[sdt] = m.to(sdt).to(DEV)
    return _MODEL[sdt]


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_mlsd_forward_against_the_fp64_net(name, sdt):
    x, ref = R.model_input(name), R.model_ref64(name)
    m = _model(sdt)
    got = m(x.to(DEV))
    assert got.dtype == sdt and got.is_contiguous() and tuple(got.shape) == tuple(ref.shape)
    gate_ma, gate_rl = EMULATION[(name, sdt)]
    ma, rl = R.max_abs(got.float().cpu(), ref), R.rel_l2(got.float().cpu(), ref)
    print(f"[mlsd] {name} {sdt}: max-abs {ma:.3e} (gate {2 * gate_ma:.3e}), rel-L2 {rl:.3e} (gate {2 * gate_rl:.3e})")
    assert ma <= 2 * gate_ma and rl <= 2 * gate_rl
    again = m(x.to(DEV))
    assert torch.equal(R.bits(got.cpu()), R.bits(again.cpu())), "two forwards differ"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", ["16x16", "17x49"])
def test_mlsd_sample_alone_equals_sample_in_a_batch_of_three(name, sdt):
    m = _model(sdt)
    x3 = torch.cat([R.model_input(name, seed=7 + i)[:1] for i in range(3)]).to(DEV)
    batch = m(x3)
    for i in range(3):
        assert torch.equal(R.bits(m(x3[i:i + 1]).cpu()), R.bits(batch[i:i + 1].cpu())), f"sample {i}"


@pytest.mark.parametrize("idt", [torch.float32, torch.float16])
def test_mlsd_input_dtypes(idt):
    """the entry convolution reads the image in the dtype it arrives in: an fp16 image gives the bits of its fp32 copy"""
    m = _model(torch.float16)
    x = R.model_input("17x49").to(idt)
    got, want = m(x.to(DEV)), m(x.float().to(DEV))
    assert got.dtype == torch.float16 and torch.equal(R.bits(got.cpu()), R.bits(want.cpu()))


@pytest.mark.parametrize("name", ["16x16", "17x49"])
def test_mlsd_workspace_dry_run_equals_use(name):
    x = R.model_input(name)
    m = _model(torch.bfloat16)
    L, dev = m._L(), torch.device(DEV)
    B, _, H, W = x.shape
    xd = x.to(DEV)
    want = m(xd)
    need = m.workspace_bytes(B, H, W, dev)
    assert need > 0
    h = C.c_void_p(m._handle)
    out = torch.empty(m.out_shape(x.shape), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes, hh=H: L.gyre_mlsd_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, B, hh, W,
                                                    C.c_void_p(wp), nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(want.cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one byte less is refused, not overrun
        _lib.check(call(need - 1), L)
    for bad in (15, 18, 20, 0):                                     # a size outside the rule: refused before any launch
        with pytest.raises(ValueError):
            _lib.check(call(need, bad), L)
        assert m.workspace_bytes(B, bad, W, dev) == 0
    torch.cuda.synchronize()
    assert m.workspace_bytes(1, 65536, 65536, dev) == 0             # more rows than the planner indexes: refused, not wrapped


def test_mlsd_refusals():
    m = _model(torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 16, 16), device=DEV))
    for H, W in ((16, 18), (34, 16), (8, 16)):
        with pytest.raises(ValueError):
            m(torch.rand((1, 4, H, W), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 4, 16, 16)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    bad, h = _lib.MlsdCfg(reserved=1), C.c_void_p()
    with pytest.raises(ValueError):
        _lib.check(L.gyre_mlsd_create(C.byref(bad), 0, C.byref(h)), L)
    ok = _lib.MlsdCfg(reserved=0)
    _lib.check(L.gyre_mlsd_create(C.byref(ok), 0, C.byref(h)), L)
    try:
        assert L.gyre_mlsd_num_params(h) == 305                      # the reference's 362 keys less the 57 num_batches_tracked
        keys = [L.gyre_mlsd_param_key(h, i).decode() for i in range(305)]
        from gyre_amd import weights
        assert keys == [k for k in weights.mlsd_param_shapes() if not k.endswith("num_batches_tracked")]
        with pytest.raises(_lib.GyreError):                          # no weights: finalize names the first missing one
            _lib.check(L.gyre_mlsd_finalize(h, None), L)
    finally:
        L.gyre_mlsd_destroy(h)
