"""The native HED edge detector (-m gpu; model_hed.hip behind gyre_amd.hinters.GyreHipHED) against the fp64 restatement of the net
(tests/hed_ref.py, itself held bit for bit in fp32 to the reference's own module by tests/test_reference_hed.py), in both storage
flavours and per map; two forwards; batch independence; workspace sizing; input dtypes; refusals."""
import ctypes as C

import pytest
import torch

import hed_ref as R
from gyre_amd import _lib
from gyre_amd.hinters import GyreHipHED
from gpu_util import DEV
# (max-abs, rel-L2) per map of the CPU emulation that rounds every stored tensor to the storage type against the fp64 net, per
# hed_ref.MODEL_CASES entry (measured, printed and re-checked by tests/test_hed_ref_host.py::test_storage_emulation_distance).  The gate is
# twice that, the factor of the RRDB / SwinIR / HAT / line-art model tests.
from test_hed_ref_host import EMULATION

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
_REF, _MODEL = {}, {}


def _setup(name):
    """(state dict, image, fp64 maps) - computed once per case and shared"""
    if name not in _REF:
        sd, x = R.model_case(name)
        _REF[name] = (sd, x, R.net(sd, x, compute=torch.float64))
    return _REF[name]


def _model(sdt):
    """one module per flavour for the whole file: the weights are the same in every case"""
    if sdt not in _MODEL:
        m = GyreHipHED()
        m.load_state_dict(R.model_weights())
        _MODEL[sdt] = m.to(sdt).to(DEV)
    return _MODEL[sdt]


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_hed_forward_against_the_fp64_net(name, sdt):
    sd, x, ref = _setup(name)
    m = _model(sdt)
    got = m(x.to(DEV))
    assert isinstance(got, list) and len(got) == 6
    assert all(g.dtype == sdt and g.is_contiguous() and tuple(g.shape) == tuple(r.shape) for g, r in zip(got, ref))
    gate_ma, gate_rl = EMULATION[(name, sdt)]
    fails = []
    for k in range(6):
        ma, rl = R.max_abs(got[k].float().cpu(), ref[k]), R.rel_l2(got[k].float().cpu(), ref[k])
        print(f"[hed] {name} {sdt} map {k + 1}: max-abs {ma:.3e} (gate {2 * gate_ma[k]:.3e}), rel-L2 {rl:.3e} (gate {2 * gate_rl[k]:.3e})")
        if not (ma <= 2 * gate_ma[k] and rl <= 2 * gate_rl[k]):
            fails.append(k + 1)
    assert not fails, f"maps {fails} outside twice the emulation's distance"
    again = m(x.to(DEV))
    assert all(torch.equal(R.bits(a.cpu()), R.bits(b.cpu())) for a, b in zip(got, again)), "two forwards differ"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", ["1x1", "5x7"])
def test_hed_sample_alone_equals_sample_in_a_batch_of_three(name, sdt):
    m = _model(sdt)
    x3 = R.model_input(name, batch=3, seed=7).to(DEV)
    batch = m(x3)
    for i in range(3):
        one = m(x3[i:i + 1])
        assert all(torch.equal(R.bits(a.cpu()), R.bits(b[i:i + 1].cpu())) for a, b in zip(one, batch)), f"sample {i}"


@pytest.mark.parametrize("idt", [torch.float32, torch.float16])
def test_hed_input_dtypes(idt):
    """the entry pass rounds the image to storage whatever it arrives as: an fp16 image into the fp16 flavour gives the bits of its fp32 copy"""
    m = _model(torch.float16)
    x = R.model_input("5x7").to(idt)
    got = m(x.to(DEV))
    want = m(x.float().to(DEV))
    assert all(g.dtype == torch.float16 for g in got)
    assert all(torch.equal(R.bits(a.cpu()), R.bits(b.cpu())) for a, b in zip(got, want))


@pytest.mark.parametrize("name", ["1x1", "33x20"])
def test_hed_workspace_dry_run_equals_use(name):
    sd, x, _ = _setup(name)
    m = _model(torch.bfloat16)
    L, dev = m._L(), torch.device(DEV)
    B, _, H, W = x.shape
    xd = x.to(DEV)
    want = torch.cat(m(xd), 0)
    need = m.workspace_bytes(B, H, W, dev)
    assert need > 0
    h = C.c_void_p(m._handle)
    out = torch.empty(m.out_shape(x.shape), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes, hh=H: L.gyre_hed_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, B, hh, W,
                                                   C.c_void_p(wp), nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(want.cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one byte less is refused, not overrun
        _lib.check(call(need - 1), L)
    with pytest.raises(ValueError):                                 # no image: refused before any launch
        _lib.check(call(need, 0), L)
    torch.cuda.synchronize()
    assert m.workspace_bytes(B, 0, W, dev) == 0
    assert m.workspace_bytes(1, 40000, 40000, dev) == 0             # more rows than the planner indexes: refused, not wrapped


def test_hed_refusals():
    m = _model(torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.rand((1, 4, 16, 16), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 3, 16, 16)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    bad, h = _lib.HedCfg(reserved=1), C.c_void_p()
    with pytest.raises(ValueError):
        _lib.check(L.gyre_hed_create(C.byref(bad), 0, C.byref(h)), L)
