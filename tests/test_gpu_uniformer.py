"""The native UniFormer backbone (-m gpu; kernels_uniformer.hip, model_uniformer.hip behind gyre_amd.hinters.GyreHipUniFormer) against
the float64 restatement tests/uniformer_ref.py (held to the reference's code by tests/test_uniformer_ref_host.py), both storage flavours.

k_uf_local, element by element (uniformer_ref.local_bound).  u = 2^-8 (bf16) / 2^-11 (fp16), fl = half the smallest storage subnormal,
e = 2^-24; x, W1, W2 are storage values, so every product of the two matrix stages is exact in fp32.  No factor is fitted:
    conv1     dt = (2 C + 2) e (|x| |W1|^T + |b1|)      C products in MFMA chains of 32, doubled for the undocumented adder tree as in
              dt <- dt + u (|t| + dt) + fl               tests/gemm_ref.py, the bias add and one spare; then the one rounding of the
                                                        intermediate - a position outside the map is exactly 0
    depthwise dd = dw(dt, |wd|) + 26 e dw(|t| + dt, |wd|, |bd|)     the error of t through the 25 taps; 25 fma and the bias
              dd <- dd + u (|d| + dd) + fl               the one rounding of the A operand of conv2
    conv2     dy = dd |W2|^T + (2 C + 3) e ((|d| + dd) |W2|^T + |b2| + |x|)       second MFMA chain; bias and residual adds
    bound = dy + u (|y| + dy) + fl                       the final rounding
The conv1 bias of the cases is 4 N(0, 1) against unit activations: writing it instead of 0 into a halo position outside the map moves
the border outputs hundreds of bounds away (tests/test_uniformer_ref_host.py shows the seeded mistake leaving the bound on the host).
Measured on an MI355X: worst |got - value| / bound 0.22 (bf16) and 0.16 (fp16) over the cases below.

k_uf_cpe: value = x + sum w x + b; bound = p + u (|value| + p) + fl with p = 11 e (|b| + sum |w| |x| + |x|) (nine fma, the bias, the
residual add); measured worst 0.998 - the final rounding is nearly all of it, and u is the exact rounding unit.  The gathers and
k_uf_taps move bits (the image gather after its one rounding): exact.

Whole module.  The bar of the SwinIR / HAT / Swin-B whole-network tests: twice the rel-L2 of the restatement with every stored tensor
rounded to the storage type (the folded weights included) against the float64 restatement, both on storage-rounded weights; EMULATION
holds that distance per size, batch and map, computed on the CPU.  Measured on an MI355X the native maps sit at 0.93 - 1.11 of it (the
deepest map at 104 x 88, B = 1: 1.397e-2 against 1.260e-2 in bf16, 1.541e-3 against 1.648e-3 in fp16).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import uniformer_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hinters import GyreHipUniFormer
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
U, FL, E = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}, {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}, 2.0 ** -24
# the tile is 8 rows x 16 columns: below the halo reach / exactly one tile / one more row and column / 3 x 3 tiles with remainders
LOCAL_MAPS = [(3, 2), (8, 16), (9, 17), (21, 37)]
EMULATION = {((96, 96), 1, torch.bfloat16): [5.290e-03, 9.773e-03, 1.275e-02, 1.506e-02],
             ((96, 96), 2, torch.bfloat16): [5.278e-03, 9.745e-03, 1.238e-02, 1.384e-02],
             ((104, 88), 1, torch.bfloat16): [5.225e-03, 9.898e-03, 1.125e-02, 1.260e-02],
             ((104, 88), 2, torch.bfloat16): [5.200e-03, 9.863e-03, 1.165e-02, 1.344e-02],
             ((96, 96), 1, torch.float16): [6.570e-04, 1.202e-03, 1.388e-03, 1.488e-03],
             ((96, 96), 2, torch.float16): [6.590e-04, 1.208e-03, 1.442e-03, 1.491e-03],
             ((104, 88), 1, torch.float16): [6.620e-04, 1.173e-03, 1.388e-03, 1.648e-03],
             ((104, 88), 2, torch.float16): [6.628e-04, 1.195e-03, 1.436e-03, 1.687e-03]}
_REF = {}


_p = lambda t: C.c_void_p(t.data_ptr())
_st = lambda: C.c_void_p(_lib.stream_ptr(torch.device(DEV)))
_taps = lambda w: w.flatten(1).t().contiguous().float()                # [C, 1, k, k] -> the kernels' [k k][C] fp32


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("Cn", [64, 128])
@pytest.mark.parametrize("hw", LOCAL_MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_uf_local_element_by_element(hw, Cn, storage, sdt):
    (H, W), B, lib = hw, 2, _lib.lib(storage)
    th, tw = C.c_int32(), C.c_int32()
    _lib.check(lib.gyre_op_uf_local_tile(C.byref(th), C.byref(tw)), lib)
    assert (th.value, tw.value) == (8, 16), "LOCAL_MAPS is chosen for this tile"
    x, w1, b1, wd, bd, w2, b2 = R.local_case(Cn, H, W, sdt)
    y0 = torch.full((B * H * W, Cn + 8), 7.0, dtype=sdt)
    dev = [t.to(DEV) for t in (x.to(sdt), w1.to(sdt), b1.float(), _taps(wd), bd.float(), w2.to(sdt), b2.float())]
    y = y0.to(DEV)
    _lib.check(lib.gyre_op_uf_local(_st(), _p(dev[0]), Cn, _p(y), Cn + 8, B, H, W, Cn, _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]),
                                    _p(dev[5]), _p(dev[6])), lib)
    torch.cuda.synchronize()
    got = y.cpu()
    val, bound = R.local_bound(x, w1, b1.float().double(), wd.float().double(), bd.float().double(), w2, b2.float().double(), U[sdt], FL[sdt])
    worst = float(((got[:, :Cn].double() - val.reshape(-1, Cn)).abs() / bound.reshape(-1, Cn)).nan_to_num(nan=float("inf")).max())
    print(f"[uniformer] uf_local {sdt} C {Cn} {H}x{W}: worst |got - value64| / bound = {worst:.3f}")
    assert torch.equal(got[:, Cn:], y0[:, Cn:]), "a guard column was written"
    assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("Cn", [64, 192])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (26, 22)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_uf_cpe_and_gather(hw, Cn, storage, sdt):
    (H, W), B, lib = hw, 2, _lib.lib(storage)
    g = torch.Generator().manual_seed(H * 100 + W + Cn)
    x = torch.randn((B, H, W, Cn), generator=g).to(sdt)
    w, b = 0.4 * torch.randn((Cn, 1, 3, 3), generator=g), 0.5 * torch.randn(Cn, generator=g)
    xd, wd, bd = x.to(DEV), _taps(w).to(DEV), b.to(DEV)
    y, wt = torch.empty_like(xd), torch.empty_like(wd)
    _lib.check(lib.gyre_op_uf_taps(_st(), _p(w.flatten(1).to(DEV)), Cn, 9, _p(wt)), lib)
    assert torch.equal(wt, wd)
    _lib.check(lib.gyre_op_uf_cpe(_st(), _p(xd), B, H, W, Cn, _p(wd), _p(bd), _p(y)), lib)
    x64, w64, b64 = x.double(), w.double(), b.double()
    val = R.cpe(x64, w64, b64)
    pre = 11 * E * (R.dw(x64.abs(), w64.abs(), b64.abs()) + x64.abs())
    worst = float(((y.cpu().double() - val).abs() / (pre + U[sdt] * (val.abs() + pre) + FL[sdt])).max())
    print(f"[uniformer] uf_cpe {sdt} C {Cn} {H}x{W}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0
    if H >= 2 and W >= 2:                                            # odd sizes: the last row / column is dropped
        o = torch.empty((B, H // 2, W // 2, 4 * Cn), dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_uf_gather(_st(), _p(xd), B, H, W, Cn, _p(o)), lib)
        assert torch.equal(o.cpu(), R.gather(x))
    if H >= 4 and W >= 4 and Cn == 64:                               # the first embedding's gather: NCHW fp32 image, 4 x 4 patches, floor
        img = torch.rand((B, 3, H, W), generator=g)
        o = torch.full((B, H // 4, W // 4, 64), 7.0, dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_uf_gather_img(_st(), _p(img.to(DEV)), _lib.F32, B, H, W, _p(o)), lib)
        nhwc = F.pad(img.to(sdt).permute(0, 2, 3, 1), (0, 1))       # channel 3 of every group is zero
        assert torch.equal(o.cpu(), R.gather(R.gather(nhwc)).view(B, H // 4, W // 4, 2, 2, 2, 2, 4).transpose(4, 5).reshape(o.shape))


def _tiny(sdt):
    """(state dict rounded to storage as fp32, the same as float64) - shared"""
    if sdt not in _REF:
        sd = R.seeded_state_dict(weights.uniformer_param_shapes(gcfg.uniformer_config(**R.TINY)))
        sd = {k: v.to(sdt).float() for k, v in sd.items()}
        _REF[sdt] = (sd, {k: v.double() for k, v in sd.items()})
    return _REF[sdt]


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(96, 96), (104, 88)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_uniformer_maps_against_the_float64_restatement(hw, B, storage, sdt):
    sd, sd64 = _tiny(sdt)
    m = GyreHipUniFormer(**R.TINY)
    m.load_state_dict(sd, strict=False)                              # (the synthetic dict carries no num_batches_tracked)
    m = m.to(sdt).to(DEV)
    x = torch.rand((B, 3) + hw, generator=torch.Generator().manual_seed(1)).to(sdt)
    key = (hw, B, sdt)
    if key not in _REF:
        _REF[key] = R.net(sd64, R.TINY, x.double())
    got = m(x.to(DEV))
    assert len(got) == 4
    for i, (a, ref) in enumerate(zip(got, _REF[key])):
        assert a.dtype == sdt and a.is_contiguous() and tuple(a.shape) == tuple(ref.shape)
        dist, gate = R.rel_l2(a.float().cpu(), ref), 2 * EMULATION[key][i]
        print(f"[uniformer] {hw} B {B} {sdt} map {i}: rel-L2 against the float64 restatement {dist:.3e} (gate {gate:.3e})")
        assert dist <= gate


def test_uniformer_real_configuration_and_refusals():
    m = GyreHipUniFormer().to(torch.float16)                         # uniformer_small
    sd = R.seeded_state_dict(weights.uniformer_param_shapes(m.config))
    m.load_state_dict({k: sd[k].to(torch.float16) if k in sd else v for k, v in m.state_dict().items()})      # strict, buffers included
    m = m.to(DEV)
    assert m.workspace_bytes(1, 512, 512, DEV) > 0                   # sized by a dry run: no forward
    for kw in (dict(windows=True), dict(hybrid=True), dict(head_dim=32), dict(embed_dim=(96, 128, 320, 512))):
        with pytest.raises(NotImplementedError):
            GyreHipUniFormer(**kw)
    with pytest.raises(ValueError):
        m(torch.rand((1, 3, 31, 96), device=DEV))
    bad, L = m._c_cfg(), m._L()
    bad.windows = 1
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_uniformer_create(C.byref(bad), 0, C.byref(C.c_void_p())), L)
    # an aliased k_uf_local call is refused before the launch: nothing is written
    x = torch.randn((1, 8, 16, 64), generator=torch.Generator().manual_seed(0)).to(torch.float16).to(DEV)
    keep = x.clone()
    w, v = torch.zeros((64, 64), dtype=torch.float16, device=DEV), torch.zeros(25 * 64, device=DEV)
    rc = L.gyre_op_uf_local(_st(), _p(x), 64, _p(x), 64, 1, 8, 16, 64, _p(w), _p(v), _p(v), _p(v), _p(w), _p(v))
    torch.cuda.synchronize()
    assert rc == -1 and torch.equal(x, keep)
