"""The native HAT (-m gpu; model_hat.hip behind gyre_amd.upscaler.GyreHipHAT) against the fp32 restatement of the net (tests/hat_ref.py,
itself held bit for bit to the reference's own code by tests/test_reference_hat.py), in both storage flavours; batch independence;
workspace sizing; refusals."""
import ctypes as C

import pytest
import torch

import hat_ref as R
from gyre_amd import _lib
from gyre_amd.upscaler import GyreHipHAT
from gpu_util import DEV
# rel-L2 of the CPU emulation that rounds every stored tensor to the storage type against the fp32 net, per hat_ref.MODEL_CASES entry
# (measured, printed and re-checked by tests/test_hat_ref_host.py::test_storage_emulation_distance).  The gate is twice that, the factor
# of tests/test_gpu_swinir_model.py and tests/test_gpu_rrdb_model.py.
from test_hat_ref_host import EMULATION

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
    m = GyreHipHAT(cfg)
    m.load_state_dict(sd, strict=False)                            # (the synthetic dict carries no buffers)
    return m.to(sdt).to(DEV)


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_hat_forward_against_fp32_net(name, sdt):
    cfg, sd, x, ref = _setup(name)
    m = _model(cfg, sd, sdt)
    got = m(x.to(DEV))
    assert got.dtype == sdt and tuple(got.shape) == tuple(ref.shape)
    d, gate = R.rel_l2(got.float().cpu(), ref), 2 * EMULATION[(name, sdt)]
    print(f"[hat] {name} {sdt}: rel-L2 against the fp32 net {d:.3e} (emulation {EMULATION[(name, sdt)]:.3e}, gate {gate:.3e})")
    assert d <= gate
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x.to(DEV)).cpu())), "two forwards differ"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", ["tiny", "w180"])
def test_hat_sample_alone_equals_sample_in_a_batch_of_three(name, sdt):
    cfg, sd, x, _ = _setup(name)
    m = _model(cfg, sd, sdt)
    x3 = torch.rand((3,) + tuple(x.shape[1:]), generator=torch.Generator().manual_seed(7)).to(DEV)
    batch = m(x3)
    for i in range(3):
        assert torch.equal(R.bits(m(x3[i:i + 1]).cpu()), R.bits(batch[i:i + 1].cpu())), f"sample {i}"


@pytest.mark.parametrize("name", ["tiny", "tiny2"])
def test_hat_workspace_dry_run_equals_use(name):
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
    call = lambda nbytes, hh=H: L.gyre_hat_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, B, hh, W, C.c_void_p(wp),
                                                   nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(m(xd).cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one allocation unit less is refused, not overrun
        _lib.check(call(need - 256), L)
    with pytest.raises(ValueError):                                 # the ABI takes multiples of the window only
        _lib.check(call(need, H - 8), L)
    torch.cuda.synchronize()
    assert m.workspace_bytes(B, H - 8, W, dev) == 0


def test_hat_refusals():
    cfg, sd, x, _ = _setup("tiny")
    m = _model(cfg, sd, torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.rand((1, 4, 16, 16), device=DEV))
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 24, 16), device=DEV))                  # not a multiple of 16: the reference has no padding either
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 16, 8), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 3, 16, 16)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    for field, value in (("window_size", 8), ("embed_dim", 64), ("upscale", 3), ("upscale", 8), ("mlp_hidden", 125), ("in_chans", 1),
                         ("overlap_ratio", 0.25), ("compress_ratio", 4), ("squeeze_factor", 16)):
        bad = m._c_cfg()
        setattr(bad, field, value)
        h = C.c_void_p()
        with pytest.raises(NotImplementedError):
            _lib.check(L.gyre_hat_create(C.byref(bad), 0, C.byref(h)), L)
    bad = m._c_cfg()
    bad.num_heads[1] = 4
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_hat_create(C.byref(bad), 0, C.byref(C.c_void_p())), L)
