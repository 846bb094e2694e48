"""The native RRDBNet (-m gpu; model_rrdb.hip behind gyre_amd.upscaler.GyreHipRRDBNet) against the fp32 restatement of the net
(tests/rrdb_ref.py), on the generic path (the planner's GEMM kernels + the epilogue kernel) and on the fused dense-block kernel, in
both storage flavours; workspace sizing; derived weight copies after a weight change."""
import ctypes as C

import pytest
import torch

import rrdb_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.upscaler import GyreHipRRDBNet
from gpu_util import DEV

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
CASES = {"x4": dict(scale=4), "x2": dict(scale=2), "x1": dict(scale=1), "plus": dict(scale=4, plus=True)}
# rel-L2 of the CPU emulation that rounds every stored tensor to the storage type against the fp32 net, for tiny_rrdb on the
# [2, 3, 24, 20] image below (measured by tests/test_rrdb_ref_host.py::test_storage_emulation_distance, printed there).  The gate is
# twice that: the native graph sums in another order and - on the fused path - rounds less often, so it should sit at or below it.
EMULATION = {("x4", torch.bfloat16): 1.204e-02, ("x4", torch.float16): 1.162e-03,
             ("x2", torch.bfloat16): 6.946e-03, ("x2", torch.float16): 9.113e-04,
             ("x1", torch.bfloat16): 6.039e-03, ("x1", torch.float16): 6.770e-04,
             ("plus", torch.bfloat16): 1.177e-02, ("plus", torch.float16): 1.147e-03}
_REF = {}


def _setup(name):
    """(cfg, state dict, image, fp32 reference) - computed once per case and shared"""
    if name not in _REF:
        cfg = gcfg.tiny_rrdb(**CASES[name])
        sd = weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))
        x = torch.rand((2, 3, 24, 20), generator=torch.Generator().manual_seed(0))
        _REF[name] = (cfg, sd, x, R.net(sd, cfg, x))
    return _REF[name]


def _model(cfg, sd, sdt, path):
    m = GyreHipRRDBNet(cfg)
    m.load_state_dict(sd)
    m = m.to(sdt).to(DEV)
    m.set_path(path)
    return m


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("path", ["generic", "fused"])
@pytest.mark.parametrize("name", list(CASES))
def test_rrdb_forward_against_fp32_net(name, path, sdt):
    cfg, sd, x, ref = _setup(name)
    m = _model(cfg, sd, sdt, path)
    got = m(x.to(DEV))
    assert got.dtype == sdt and tuple(got.shape) == tuple(ref.shape)
    d, gate = R.rel_l2(got.float().cpu(), ref), 2 * EMULATION[(name, sdt)]
    print(f"[rrdb] {name} {path} {sdt}: rel-L2 against the fp32 net {d:.3e} (emulation {EMULATION[(name, sdt)]:.3e}, gate {gate:.3e})")
    assert d <= gate
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x.to(DEV)).cpu())), "two forwards differ"
    one = m(x[1:2].to(DEV))                                         # a sample alone = the same sample inside the batch
    assert torch.equal(R.bits(one.cpu()), R.bits(got[1:2].cpu()))


@pytest.mark.parametrize("path", ["generic", "fused"])
def test_rrdb_input_dtype_does_not_matter(path):
    cfg, sd, x, ref = _setup("x4")
    m = _model(cfg, sd, torch.bfloat16, path)
    a = m(x.to(DEV)).float().cpu()
    b = m(x.to(torch.bfloat16).to(DEV)).float().cpu()               # the image is rounded to storage on entry either way
    assert torch.equal(a, b)


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(CASES))
def test_rrdb_paths_agree(name, sdt):
    """generic against fused.  Both are realisations of the same storage-rounding graph with independent rounding errors of the size
    the emulation measures, so their distance is about sqrt(2) times it: gated at the same twice the emulation value."""
    cfg, sd, x, _ = _setup(name)
    a = _model(cfg, sd, sdt, "generic")(x.to(DEV)).float().cpu()
    b = _model(cfg, sd, sdt, "fused")(x.to(DEV)).float().cpu()
    d = R.rel_l2(a, b)
    print(f"[rrdb] {name} {sdt}: generic against fused rel-L2 {d:.3e} (gate {2 * EMULATION[(name, sdt)]:.3e})")
    assert 0 < d <= 2 * EMULATION[(name, sdt)]


@pytest.mark.parametrize("path", ["generic", "fused"])
def test_rrdb_workspace_dry_run_equals_use(path):
    cfg, sd, x, _ = _setup("plus")
    m = _model(cfg, sd, torch.bfloat16, path)
    L, dev = m._L(), torch.device(DEV)
    need = m.workspace_bytes(2, 24, 20, dev)
    assert need > 0
    h = C.c_void_p(m._handle)
    xd = x.to(DEV)
    out = torch.empty((2, 3, 96, 80), dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes: L.gyre_rrdb_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(xd.data_ptr()), 0, 2, 24, 20, C.c_void_p(wp),
                                              nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(m(xd).cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one allocation unit less is refused, not overrun
        _lib.check(call(need - 256), L)
    torch.cuda.synchronize()


def test_rrdb_set_weight_after_finalize_refreshes_derived_copies():
    cfg, sd, x, _ = _setup("x4")
    m = _model(cfg, sd, torch.float16, "fused")
    xd = x.to(DEV)
    before = m(xd).cpu()
    sd2 = dict(sd)
    key = "body.1.rdb3.conv5.weight"
    sd2[key] = sd[key] * -1.5
    fresh = _model(cfg, sd2, torch.float16, "fused")
    want = fresh(xd).cpu()
    # one key through the C ABI on the live, finalized handle: the chunk-ordered copy of that weight must be remade
    L, t = m._L(), sd2[key].to(DEV).contiguous()
    shape = (C.c_int64 * 4)(*t.shape)
    _lib.check(L.gyre_rrdb_set_weight(C.c_void_p(m._handle), key.encode(), C.c_void_p(t.data_ptr()), 0, shape, 4,
                                      C.c_void_p(_lib.stream_ptr(torch.device(DEV)))), L)
    _lib.check(L.gyre_rrdb_finalize(C.c_void_p(m._handle), None), L)
    after = m(xd).cpu()
    assert not torch.equal(R.bits(after), R.bits(before))
    assert torch.equal(R.bits(after), R.bits(want))


def test_rrdb_refusals():
    cfg, sd, x, _ = _setup("x2")
    m = _model(cfg, sd, torch.bfloat16, "auto")
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 25, 20), device=DEV))                  # scale 2 needs even sizes, as BasicSR asserts
    with pytest.raises(ValueError):
        m(torch.rand((1, 4, 24, 20), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.rand((1, 3, 24, 20)))                              # CPU tensor: no fallback
    L = _lib.lib(_lib.BF16)
    bad = _lib.RRDBCfg(3, 3, 48, 2, 32, 4, 0)
    h = C.c_void_p()
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_rrdb_create(C.byref(bad), 0, C.byref(h)), L)
    with pytest.raises(ValueError):
        _lib.check(L.gyre_rrdb_set_path(C.c_void_p(m._handle), 3), L)
