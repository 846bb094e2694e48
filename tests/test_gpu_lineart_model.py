"""The native line-art generator (-m gpu; model_lineart.hip behind gyre_amd.hinters.GyreHipDrawingGenerator) against the fp32 restatement
of the net (tests/lineart_ref.py, itself held bit for bit to the reference's own module by tests/test_reference_lineart.py), in both
storage flavours; batch independence; workspace sizing; refusals; the smallest image."""
import ctypes as C

import pytest
import torch

import lineart_ref as R
from gyre_amd import _lib
from gyre_amd.hinters import GyreHipDrawingGenerator
from gpu_util import DEV
# rel-L2 of the CPU emulation that rounds every stored tensor to the storage type against the fp32 net, per lineart_ref.MODEL_CASES entry
# (measured, printed and re-checked by tests/test_lineart_ref_host.py::test_storage_emulation_distance).  The gate is twice that, the
# factor of the RRDB / SwinIR / HAT model tests.
from test_lineart_ref_host import EMULATION

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
_REF = {}


def _setup(name):
    """(cfg, state dict, image, fp32 reference) - computed once per case and shared"""
    if name not in _REF:
        cfg, sd, x = R.model_case(name)
        _REF[name] = (cfg, sd, x, R.net(sd, cfg, x))
    return _REF[name]


def _model(cfg, sd, sdt):
    m = GyreHipDrawingGenerator(cfg.input_nc, cfg.output_nc, cfg.n_residual_blocks, cfg.sigmoid)
    m.load_state_dict(sd)
    return m.to(sdt).to(DEV)


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_lineart_forward_against_fp32_net(name, sdt):
    cfg, sd, x, ref = _setup(name)
    m = _model(cfg, sd, sdt)
    got = m(x.to(DEV))
    assert got.dtype == sdt and tuple(got.shape) == tuple(ref.shape)
    d, gate = R.rel_l2(got.float().cpu(), ref), 2 * EMULATION[(name, sdt)]
    print(f"[lineart] {name} {sdt}: rel-L2 against the fp32 net {d:.3e} (emulation {EMULATION[(name, sdt)]:.3e}, gate {gate:.3e})")
    assert d <= gate
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x.to(DEV)).cpu())), "two forwards differ"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_lineart_sample_alone_equals_sample_in_a_batch_of_three(name, sdt):
    cfg, sd, x, _ = _setup(name)
    m = _model(cfg, sd, sdt)
    x3 = torch.rand((3,) + tuple(x.shape[1:]), generator=torch.Generator().manual_seed(7)).to(DEV)
    batch = m(x3)
    for i in range(3):
        assert torch.equal(R.bits(m(x3[i:i + 1]).cpu()), R.bits(batch[i:i + 1].cpu())), f"sample {i}"


@pytest.mark.parametrize("name", ["tiny", "odd"])
def test_lineart_workspace_dry_run_equals_use(name):
    cfg, sd, x, _ = _setup(name)
    m = _model(cfg, sd, torch.bfloat16)
    L, dev = m._L(), torch.device(DEV)
    B, _, H, W = x.shape
    need = m.workspace_bytes(B, H, W, dev)
    assert need > 0
    h = C.c_void_p(m._handle)
    xd = x.to(DEV)
    out = torch.empty(m.out_shape(x.shape), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes, hh=H: L.gyre_lineart_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, B, hh, W,
                                                       C.c_void_p(wp), nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(m(xd).cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one allocation unit less is refused, not overrun
        _lib.check(call(need - 256), L)
    with pytest.raises(ValueError):                                 # the ABI takes images of at least 5 x 5 only
        _lib.check(call(need, 4), L)
    torch.cuda.synchronize()
    assert m.workspace_bytes(B, 4, W, dev) == 0


def test_lineart_refusals():
    cfg, sd, x, _ = _setup("tiny")
    m = _model(cfg, sd, torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.rand((1, 4, 16, 16), device=DEV))
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 4, 16), device=DEV))                   # torch's reflection paddings refuse that size too
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 3, 16, 16)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    for field, value in (("input_nc", 1), ("output_nc", 3), ("n_residual_blocks", 0), ("n_residual_blocks", 17)):
        bad = m._c_cfg()
        setattr(bad, field, value)
        h = C.c_void_p()
        with pytest.raises(NotImplementedError):
            _lib.check(L.gyre_lineart_create(C.byref(bad), 0, C.byref(h)), L)


@pytest.mark.parametrize("sdt", SDTS)
def test_lineart_smallest_image(sdt):
    """5 x 6 -> 3 x 3 -> 2 x 2 planes at the residual blocks, output 8 x 8.  No numeric gate at this size: a 2 x 2 normalisation plane
    amplifies storage rounding beyond what a gate could usefully hold."""
    cfg, sd, _, _ = _setup("tiny")
    m = _model(cfg, sd, sdt)
    x = torch.rand((1, 3, 5, 6), generator=torch.Generator().manual_seed(3)).to(DEV)
    got = m(x)
    assert tuple(got.shape) == (1, 1, 8, 8) and got.dtype == sdt
    assert torch.isfinite(got.float()).all()
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x).cpu()))
