"""The native BAE normal-map decoder (-m gpu; kernels_bae.hip, model_bae.hip behind gyre_amd.hinters.GyreHipBaeDecoder) against the
float64 restatement tests/bae_ref.py (held to the reference's code by tests/test_reference_bae.py), both storage flavours.

k_bae_refine, raw output, element by element within bae_ref.refine_bound.  u = 2^-8 (bf16) / 2^-11 (fp16), fl = half the smallest
storage subnormal, e = 2^-24; x and W1 .. W3 are storage values, so every MFMA product is exact in fp32.  No factor is fitted:
    layer 1   dt = |W1p| (u |p| + fl) + (2 (CF + 4) + 2) e (|W1| |[x | p]| + |W1p| (u |p| + fl) + |b1|): the prediction's rounding; the
              products in MFMA chains of 32, doubled for the adder tree as in tests/gemm_ref.py, the bias.  t stays fp32: no rounding
    lerp      da = lerp(dt) + ((2 srcy + 2) + (2 srcx + 2) + 6) e sum_corners (|t| + dt): fp32 coordinates and weights; ReLU is 1-Lipschitz
    layer 2/3 dh <- dh + u (h + dh) + fl, the one rounding of the MFMA operand; dz = |W| dh + (2 128 + 4) e (|W| (h + dh) + |b|)
    layer 4   the same without the rounding (h3 stays fp32); 128 fma, two shuffle adds and the bias are inside the same count
The layer-1 bias is 4 N(0, 1) against unit activations and the prediction's weight columns have the size of the others: a dropped bias,
a forgotten p, a wrong halo or an unclamped edge lands far outside the bound.
Normalising epilogue against float64 norm_normalize of the same launch's raw output: the sum of squares in three roundings (1.5 e after
the root), sqrtf, the + 1e-10 and the division correctly rounded (e each): 4.5 e, gate 8 e |value|; kappa = (elu + 1) + 0.01 with expm1f
within 2 ulp of a value below 1 and two adds: gate 8 e max(|value|, 1).
k_bae_up_concat: bound = pre + u (|value| + pre) + fl, pre = bae_ref.lerp_bound of an exactly known map; skip slice and padding exact.
Whole decoder at num_features = 512: twice the rel-L2 of the storage-rounded restatement (bae_ref.decoder(rnd=...)) against the float64
one, both on storage-rounded weights; EMULATION holds that distance per size, batch and map, computed on the CPU.  Measured on an
MI355X: refine worst |got - value| / bound 0.003, epilogue 0.28, up_concat 0.995, the maps at 0.43 - 0.68 of the gate.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import bae_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hinters import GyreHipBaeDecoder
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
U, FL, E = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}, {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}, 2.0 ** -24
# the fine tile is 16 x 16, its coarse footprint 8 x 8: one pixel / below a tile / exactly one tile / one more row and column / 3 x 3 tiles with remainders
REFINE_MAPS = [(1, 1), (2, 3), (8, 8), (9, 9), (19, 21)]
EMULATION = {((8, 12), 1, torch.bfloat16): [2.032e-03, 3.053e-03, 6.431e-03, 2.119e-03],
             ((8, 12), 2, torch.bfloat16): [1.939e-03, 3.022e-03, 6.103e-03, 2.250e-03],
             ((24, 20), 1, torch.bfloat16): [7.274e-03, 4.684e-03, 5.761e-03, 2.602e-03],
             ((24, 20), 2, torch.bfloat16): [2.712e-03, 6.621e-03, 5.147e-03, 2.929e-03],
             ((8, 12), 1, torch.float16): [2.978e-04, 3.760e-04, 8.353e-04, 2.714e-04],
             ((8, 12), 2, torch.float16): [2.375e-04, 4.095e-04, 7.896e-04, 2.776e-04],
             ((24, 20), 1, torch.float16): [6.081e-04, 5.624e-04, 7.405e-04, 5.488e-04],
             ((24, 20), 2, torch.float16): [3.759e-04, 7.394e-04, 5.945e-04, 4.342e-04]}
_REF = {}
GUARD = 64

_p = lambda t: C.c_void_p(t.data_ptr())
_st = lambda: C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _refine(lib, x, pred, sd, sdt, normalize):
    """one launch on x at a pixel stride of CF + 8 into a pre-filled buffer; returns (the output block, the guards around it)"""
    B, CF, Hs, Ws = x.shape
    xp = torch.full((B, Hs, Ws, CF + 8), 7.0, dtype=sdt)
    xp[..., :CF] = x.permute(0, 2, 3, 1).to(sdt)
    w1 = F.pad(sd["s.0.weight"].flatten(1), (0, 28)).to(sdt)
    dev = [t.to(DEV) for t in (xp, pred.float(), w1, sd["s.0.bias"].float(), sd["s.2.weight"].flatten(1).to(sdt), sd["s.2.bias"].float(),
                               sd["s.4.weight"].flatten(1).to(sdt), sd["s.4.bias"].float(), sd["s.6.weight"].flatten(1).float(),
                               sd["s.6.bias"].float())]
    n = B * 4 * 4 * Hs * Ws
    out = torch.full((n + 2 * GUARD,), 7.0, device=DEV)
    _lib.check(lib.gyre_op_bae_refine(_st(), _p(dev[0]), CF + 8, _p(dev[1]), B, Hs, Ws, CF, *[_p(t) for t in dev[2:]], int(normalize),
                                      C.c_void_p(out.data_ptr() + 4 * GUARD)), lib)
    torch.cuda.synchronize()
    out = out.cpu()
    return out[GUARD:GUARD + n].view(B, 4, 2 * Hs, 2 * Ws), torch.cat([out[:GUARD], out[GUARD + n:]])


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("CF", [32, 128, 512])
@pytest.mark.parametrize("hw", REFINE_MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
def test_bae_refine_element_by_element(hw, CF, storage, sdt):
    lib = _lib.lib(storage)
    th, tw = C.c_int32(), C.c_int32()
    _lib.check(lib.gyre_op_bae_refine_tile(C.byref(th), C.byref(tw)), lib)
    assert (th.value, tw.value) == (16, 16), "REFINE_MAPS is chosen for this tile"
    x, pred, sd = R.refine_case(CF, *hw, sdt)
    got, guards = _refine(lib, x, pred, sd, sdt, False)
    w = [sd[f"s.{2 * i}.{k}"].flatten(1) if k == "weight" else sd[f"s.{2 * i}.{k}"] for i in range(4) for k in ("weight", "bias")]
    val, bound = R.refine_bound(x, pred, *w, U[sdt], FL[sdt])
    worst = float(((got.double() - val).abs() / bound).nan_to_num(nan=float("inf")).max())
    print(f"[bae] refine {sdt} CF {CF} {hw[0]}x{hw[1]}: worst |got - value64| / bound = {worst:.3f}")
    assert bool((guards == 7.0).all()), "an element outside the output block was written"
    assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
def test_bae_refine_normalising_epilogue(storage, sdt):
    lib = _lib.lib(storage)
    x, pred, sd = R.refine_case(128, 9, 9, sdt)
    raw, _ = _refine(lib, x, pred, sd, sdt, False)
    got, _ = _refine(lib, x, pred, sd, sdt, True)
    val = R.norm_normalize(raw.double())
    tol = 8 * E * torch.cat([val[:, :3].abs(), val[:, 3:].abs().clamp_min(1.0)], dim=1)
    worst = float(((got.double() - val).abs() / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    print(f"[bae] normalising epilogue {sdt}: worst |got - value64| / tolerance = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("src,dst", [((1, 1), (2, 2)), ((3, 2), (5, 4)), ((8, 8), (16, 16))], ids=["1x1", "3x2", "8x8"])
def test_bae_up_concat(src, dst, storage, sdt):
    lib, B, Cn, Cs, ldo = _lib.lib(storage), 2, 40, 5, 64
    g = torch.Generator().manual_seed(src[0] * 10 + dst[1])
    x, skip = torch.randn((B, Cn) + src, generator=g).to(sdt), torch.randn((B, Cs) + dst, generator=g)
    xp = torch.full((B,) + src + (Cn + 8,), 7.0, dtype=sdt)
    xp[..., :Cn] = x.permute(0, 2, 3, 1)
    y, xd, sk = torch.full((B,) + dst + (ldo,), 7.0, dtype=sdt, device=DEV), xp.to(DEV), skip.to(DEV)
    _lib.check(lib.gyre_op_bae_up_concat(_st(), _p(xd), B, *src, Cn, Cn + 8, _p(sk), _lib.F32, Cs, *dst, _p(y), ldo), lib)
    torch.cuda.synchronize()
    y = y.cpu().permute(0, 3, 1, 2)
    val, pre = R.lerp_bound(x.double(), torch.zeros_like(x, dtype=torch.float64), *dst)
    assert torch.allclose(val, R.interp(x.double(), dst), rtol=1e-12, atol=1e-12)
    worst = float(((y[:, :Cn].double() - val).abs() / (pre + U[sdt] * (val.abs() + pre) + FL[sdt])).max())
    print(f"[bae] up_concat {sdt} {src} -> {dst}: worst |got - value64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(y[:, Cn:Cn + Cs], skip.to(sdt)) and bool((y[:, Cn + Cs:] == 0).all())


def _tiny(sdt):
    """(state dict rounded to storage as fp32, the same as float64) - shared"""
    if sdt not in _REF:
        sd = R.seeded_state_dict(weights.bae_param_shapes(gcfg.bae_config(**R.TINY)))
        sd = {k: v.to(sdt).float() for k, v in sd.items()}
        _REF[sdt] = (sd, {k: v.double() for k, v in sd.items()})
    return _REF[sdt]


@pytest.mark.parametrize("storage,sdt", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(8, 12), (24, 20)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_bae_maps_against_the_float64_restatement(hw, B, storage, sdt):
    sd, sd64 = _tiny(sdt)
    m = GyreHipBaeDecoder(**R.TINY)
    m.load_state_dict(sd, strict=False)                              # (the synthetic dict carries no num_batches_tracked)
    m = m.to(sdt).to(DEV)
    blocks = [b.to(sdt) for b in R.seeded_blocks(R.TINY, B, *hw)]
    key = (hw, B, sdt)
    if key not in _REF:
        _REF[key] = R.decoder(sd64, [b.double() for b in blocks])
    got, second, third = m(R.features([b.to(DEV) for b in blocks]))
    assert len(got) == 4 and second[0] is got[0] and second[1:] == [None] * 3 and third == [None] * 4
    for i, (a, ref) in enumerate(zip(got, _REF[key])):
        assert a.dtype == sdt and a.is_contiguous() and tuple(a.shape) == tuple(ref.shape)
        dist, gate = R.rel_l2(a.float().cpu(), ref), 2 * EMULATION[key][i]
        print(f"[bae] {hw} B {B} {sdt} map {i}: rel-L2 against the float64 restatement {dist:.3e} (gate {gate:.3e}, ratio {dist / gate:.2f})")
        assert dist <= gate


def test_bae_real_configuration_and_refusals():
    m = GyreHipBaeDecoder("BN").to(torch.float16)                    # num_features 2048, skips (24, 40, 64, 176)
    sd = R.seeded_state_dict(weights.bae_param_shapes(m.config))
    m.load_state_dict({k: sd[k].to(torch.float16) if k in sd else v for k, v in m.state_dict().items()})      # strict, buffers included
    m = m.to(DEV)
    assert m.workspace_bytes(1, 256, 256, DEV) > 0                   # a 512 x 512 image, sized by a dry run: no forward
    with pytest.raises(NotImplementedError):
        GyreHipBaeDecoder("GN")
    blocks = [torch.zeros(s, dtype=torch.float16, device=DEV) for s in m.block_shapes(1, 6, 8)]
    with pytest.raises(ValueError):
        m(R.features(blocks))
    with pytest.raises(NotImplementedError):
        m(R.features(blocks), mode="train")
    bad, L = m._c_cfg(), m._L()
    bad.architecture = 1
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_bae_create(C.byref(bad), 0, C.byref(C.c_void_p())), L)
    # an aliased k_bae_refine call is refused before the launch: nothing is written
    p = torch.randn((1, 4, 8, 8), generator=torch.Generator().manual_seed(0)).to(DEV)
    keep = p.clone()
    w, v = torch.zeros((128, 160), dtype=torch.float16, device=DEV), torch.zeros(512, device=DEV)
    rc = L.gyre_op_bae_refine(_st(), _p(w), 128, _p(p), 1, 8, 8, 128, _p(w), _p(v), _p(w), _p(v), _p(w), _p(v), _p(v), _p(v), 0, _p(p))
    torch.cuda.synchronize()
    assert rc == -1 and torch.equal(p, keep)
