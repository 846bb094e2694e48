"""The native SwinIR (-m gpu; model_swinir.hip behind gyre_amd.upscaler.GyreHipSwinIR) against the fp32 restatement of the net
(tests/swinir_ref.py, itself held bit for bit to the reference's own code by tests/test_reference_swinir.py), in both storage flavours;
batch independence; host padding; workspace sizing; refusals."""
import ctypes as C

import pytest
import torch

import swinir_ref as R
from gyre_amd import _lib
from gyre_amd.upscaler import GyreHipSwinIR
from gpu_util import DEV

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
# rel-L2 of the CPU emulation that rounds every stored tensor to the storage type against the fp32 net, per swinir_ref.MODEL_CASES entry
# (measured by tests/test_swinir_ref_host.py::test_storage_emulation_distance, printed and re-checked there).  The gate is twice that,
# the factor of tests/test_gpu_rrdb_model.py: the native graph sums in another order, so it should sit at or below the emulation.
EMULATION = {("tiny", torch.bfloat16): 3.928e-03, ("tiny", torch.float16): 5.073e-04,
             ("tiny3", torch.bfloat16): 3.939e-03, ("tiny3", torch.float16): 4.876e-04,
             ("w180", torch.bfloat16): 3.520e-03, ("w180", torch.float16): 4.663e-04,
             ("w240", torch.bfloat16): 3.192e-03, ("w240", torch.float16): 3.770e-04}
_REF = {}


def _setup(name):
    """(cfg, state dict, image, fp32 reference) - computed once per case and shared"""
    if name not in _REF:
        cfg, sd, x = R.model_case(name)
        _REF[name] = (cfg, sd, x, R.net(sd, cfg, x))
    return _REF[name]


def _model(cfg, sd, sdt):
    m = GyreHipSwinIR(cfg)
    m.load_state_dict(sd, strict=False)                            # (the synthetic dict carries no buffers)
    return m.to(sdt).to(DEV)


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_swinir_forward_against_fp32_net(name, sdt):
    cfg, sd, x, ref = _setup(name)
    m = _model(cfg, sd, sdt)
    got = m(x.to(DEV))
    assert got.dtype == sdt and tuple(got.shape) == tuple(ref.shape)
    d, gate = R.rel_l2(got.float().cpu(), ref), 2 * EMULATION[(name, sdt)]
    print(f"[swinir] {name} {sdt}: rel-L2 against the fp32 net {d:.3e} (emulation {EMULATION[(name, sdt)]:.3e}, gate {gate:.3e})")
    assert d <= gate
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x.to(DEV)).cpu())), "two forwards differ"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", ["tiny", "w240"])
def test_swinir_sample_alone_equals_sample_in_a_batch_of_three(name, sdt):
    cfg, sd, x, _ = _setup(name)
    m = _model(cfg, sd, sdt)
    x3 = torch.rand((3,) + tuple(x.shape[1:]), generator=torch.Generator().manual_seed(7)).to(DEV)
    batch = m(x3)
    for i in range(3):
        assert torch.equal(R.bits(m(x3[i:i + 1]).cpu()), R.bits(batch[i:i + 1].cpu())), f"sample {i}"


@pytest.mark.parametrize("sdt", SDTS)
def test_swinir_unaligned_image_is_the_crop_of_the_host_padded_call(sdt):
    cfg, sd, _, _ = _setup("tiny")
    m = _model(cfg, sd, sdt)
    x = torch.rand((1, 3, 13, 21), generator=torch.Generator().manual_seed(1))
    got = m(x.to(DEV))
    padded = torch.nn.functional.pad(x, (0, 3, 0, 3), "reflect")
    full = m(padded.to(DEV))
    assert tuple(got.shape) == (1, 3, 52, 84) and torch.equal(R.bits(got.cpu()), R.bits(full[:, :, :52, :84].cpu()))
    d = R.rel_l2(got.float().cpu(), R.net(sd, cfg, x))
    print(f"[swinir] tiny 13x21 {sdt}: rel-L2 against the fp32 net {d:.3e}")
    assert d <= 2 * EMULATION[("tiny", sdt)]


@pytest.mark.parametrize("name", ["tiny", "tiny3"])
def test_swinir_workspace_dry_run_equals_use(name):
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
    call = lambda nbytes, hh=H: L.gyre_swinir_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, B, hh, W, C.c_void_p(wp),
                                                      nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(m(xd).cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one allocation unit less is refused, not overrun
        _lib.check(call(need - 256), L)
    with pytest.raises(ValueError):                                 # the ABI takes multiples of the window only
        _lib.check(call(need, H - 4), L)
    torch.cuda.synchronize()
    assert m.workspace_bytes(B, H - 4, W, dev) == 0


def test_swinir_refusals():
    cfg, sd, x, _ = _setup("tiny")
    m = _model(cfg, sd, torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.rand((1, 4, 16, 16), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 3, 16, 16)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    for field, value in (("window_size", 7), ("embed_dim", 64), ("upscale", 3), ("mlp_hidden", 125), ("in_chans", 1)):
        bad = m._c_cfg()
        setattr(bad, field, value)
        h = C.c_void_p()
        with pytest.raises(NotImplementedError):
            _lib.check(L.gyre_swinir_create(C.byref(bad), 0, C.byref(h)), L)
    bad = m._c_cfg()
    bad.num_heads[1] = 4
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_swinir_create(C.byref(bad), 0, C.byref(C.c_void_p())), L)
