"""The VAE graph node by node (-m gpu): the output of every node of gyre_vae_encode / gyre_vae_decode (gyre_vae_debug_tap) and the
complete gradient of every decoder node's output in the sweep of gyre_vae_decode_vjp (gyre_vae_debug_grad_tap) against the fp32
oracle, each gated at twice its own storage-emulation floor (tests/vae_graph_ref.py: configs, emulation, floors, verdict;
tests/test_vae_graph_ref_host.py shows on the CPU which seeded wiring mistakes these criteria catch and which of them the old
whole-tensor gates let through).

Both storage flavours run in this process (net.to(torch.bfloat16 | torch.float16)); nothing here reads gpu_util.HDT.
`[vaegraph]` lines carry the measured native distances next to their floors; they are printed, not asserted - the assertions are the
verdicts.  Inputs: B = 2, latents 8x12 and the odd 5x7 (images 32x48 and 20x28; 96 and 35 tokens in the mid attention).

Tap lifetime as the header states it (include/gyre_hip.h): forward taps belong to the next encode OR decode, which writes those of
its own half and drops all of them; gradient taps belong to the next decode VJP, which drops them also when it refuses the call.
Batch composition is checked WITHOUT batch-invariant planning (gyre_set_batch_invariant stays as the process has it, off by
default): at these sizes every launch of the decoder is planned alike for one sample and for two."""
import ctypes as C

import pytest
import torch

import vae_graph_ref as V
from gyre_amd import _lib
from gyre_amd.modules import GyreHipVAE
from gpu_util import DEV

pytestmark = pytest.mark.gpu
_NET = {}
NAN = float("nan")
DT = pytest.mark.parametrize("dtype", V.DTYPES, ids=lambda d: V.DT_NAME[d])


def _net(name, dtype):
    if (name, dtype) not in _NET:
        cfg = V.CONFIGS[name]
        net = GyreHipVAE(cfg)
        net.load_state_dict(V.state_dict(cfg))
        net = net.to(dtype).to(DEV)
        net._sync(torch.device(DEV))                   # uploads the weights, creates the handle
        _NET[(name, dtype)] = net
    return _NET[(name, dtype)]


def _set(net, grad, shapes):
    """NaN-filled buffers of the given shapes, registered as forward (grad=False) or gradient taps"""
    L = net._L()
    fn = L.gyre_vae_debug_grad_tap if grad else L.gyre_vae_debug_tap
    bufs = {k: torch.full(tuple(sh), NAN, dtype=torch.float32, device=DEV) for k, sh in shapes.items()}
    for k, b in bufs.items():
        _lib.check(fn(C.c_void_p(net._handle), k.encode(), C.c_void_p(b.data_ptr()), b.numel() * 4), L)
    return bufs


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


def _encode(net, img, shapes):
    """one encode with the given node taps set: a result in the layout of vae_graph_ref.oracle_encode()"""
    out = _set(net, False, shapes)
    m = net.encode(img.to(DEV)).latent_dist.parameters
    torch.cuda.synchronize()
    return {"moments": m.float().cpu(), "out": _cpu(out)}


def _decode(net, z, cot, shapes, gshapes=None):
    """one decode with the given node taps set, then (cot given) its VJP with the given gradient taps set: a result in the layout of
    vae_graph_ref.oracle_decode()"""
    out = _set(net, False, shapes)
    zd = z.to(DEV).requires_grad_(cot is not None)
    img = net.decode(zd).sample
    res = {"image": img.detach().float().cpu()}
    if cot is not None:
        grad = _set(net, True, shapes if gshapes is None else gshapes)
        (dz,) = torch.autograd.grad(img, zd, cot.to(DEV))
        res["d_z"] = dz.float().cpu()
    torch.cuda.synchronize()
    res["out"] = _cpu(out)
    if cot is not None:
        res["grad"] = _cpu(grad)
    return res


def _written(res):
    for grp in ("out", "grad"):
        for k, v in res.get(grp, {}).items():
            assert not bool(torch.isnan(v).any()), f"{grp} tap {k} was not written completely"


def _judge(label, got, ref, floors, dtype):
    ok, ratios, worst = V.verdict(got, ref, floors)
    d = V.distances(got, ref)
    tag = f"[vaegraph] {label} {V.DT_NAME[dtype]}"
    print(f"{tag}: " + "  ".join(f"{k} {v:.3e} (floor {floors[k]:.3e})" for k, v in d.items() if not isinstance(v, dict)))
    for k in ref["out"]:
        print(f"{tag} {k}: " + "  ".join(f"{g} {d[g][k]:.3e} (floor {floors[g][k]:.3e})" for g in ("out", "grad") if g in d))
    for grp, (r, k) in worst.items():
        print(f"{tag} worst {grp}: ratio {r:.3f} at {k}")
    # the first failing node in forward order / the last failing node in sweep order (= the first in forward order) locate a finding
    bad = [(g, k) for g in ("out", "grad") if g in ratios for k in ref["out"] if not ratios[g][k] <= 1.0]
    outer = {k: round(v, 2) for k, v in ratios.items() if not isinstance(v, dict)}
    assert ok, f"{label}: over the gate (distance / (2 x floor) > 1): {outer} nodes {bad[:6]}"


def _shapes(ref):
    return {k: v.shape for k, v in ref["out"].items()}


@DT
@pytest.mark.parametrize("size", V.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_encoder_node_and_the_moments(size, dtype):
    cfg, sd, (z, img, cot), ref = V.case("vae_graph", size, "encode")
    got = _encode(_net("vae_graph", dtype), img, _shapes(ref))
    _written(got)
    _judge(f"vae_graph {size[0]}x{size[1]} encode", got, ref, V.floors_for("vae_graph", size, "encode", dtype), dtype)


@DT
@pytest.mark.parametrize("name,size", [("vae_graph", V.SIZES[0]), ("vae_graph", V.SIZES[1]), ("vae_wide", V.SIZES[0])],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_every_decoder_node_output_and_gradient(name, size, dtype):
    cfg, sd, (z, img, cot), ref = V.case(name, size, "decode")
    got = _decode(_net(name, dtype), z, cot, _shapes(ref))
    _written(got)
    _judge(f"{name} {size[0]}x{size[1]} decode", got, ref, V.floors_for(name, size, "decode", dtype), dtype)


@DT
def test_every_node_under_tiling_xy_and_the_sweep_still_refuses(dtype):
    """Every conv wraps, the encoder's explicit (0,1,0,1) pad stays zeros (oracle: M.tiling("xy")).  The sweep has no circular
    convolutions: gyre_vae_decode_vjp refuses, writes no gradient tap and drops the ones set for it."""
    size = V.SIZES[0]
    net = _net("vae_graph", dtype)
    net.set_tiling("xy")
    try:
        cfg, sd, (z, img, cot), ref = V.case("vae_graph", size, "encode", "xy")
        got = _encode(net, img, _shapes(ref))
        _written(got)
        _judge("vae_graph 8x12 encode tiling xy", got, ref, V.floors_for("vae_graph", size, "encode", dtype, "xy"), dtype)
        cfg, sd, (z, img, cot), ref = V.case("vae_graph", size, "decode", "xy")
        got = _decode(net, z, None, _shapes(ref))
        _written(got)
        _judge("vae_graph 8x12 decode tiling xy", got, ref, V.floors_for("vae_graph", size, "decode", dtype, "xy"), dtype)
        zd = z.to(DEV).requires_grad_()
        image = net.decode(zd).sample
        one = "decoder.mid_block.resnets.1"
        gbuf = _set(net, True, {one: ref["out"][one].shape})[one]
        with pytest.raises(NotImplementedError, match="circular"):
            torch.autograd.grad(image, zd, torch.ones_like(image))
    finally:
        net.set_tiling(False)
    cfg, sd, (z, img, cot), plain = V.case("vae_graph", size, "decode")
    res = _decode(net, z, cot, {}, gshapes={})                 # the next sweep runs: the refused call's tap is gone
    assert bool(torch.isnan(gbuf).all())
    assert V.verdict({k: res[k] for k in ("image", "d_z")}, {k: plain[k] for k in ("image", "d_z")},
                     V.floors_for("vae_graph", size, "decode", dtype))[0]


@DT
def test_a_batch_of_two_is_its_two_samples_bit_for_bit_at_every_node(dtype):
    """The rule of test_unet_batch_independence_bit_exact, per node: a tapped decode of B = 2 against the tapped decodes of each
    sample alone.  Batch-invariant planning is not needed and not touched (module docstring)."""
    cfg, sd, (z, img, cot), ref = V.case("vae_graph", V.SIZES[0], "decode")
    net = _net("vae_graph", dtype)
    both = _decode(net, z, None, _shapes(ref))
    _written(both)
    for i in range(2):
        one = _decode(net, z[i:i + 1].contiguous(), None, {k: (1,) + tuple(s[1:]) for k, s in _shapes(ref).items()})
        _written(one)
        differ = [k for k in ref["out"] if not torch.equal(both["out"][k][i:i + 1], one["out"][k])]
        assert not differ, f"sample {i}: first node that differs between batch compositions: {differ[0]}"
        assert torch.equal(both["image"][i:i + 1], one["image"])


@DT
def test_taps_do_not_change_what_runs(dtype):
    """Nothing in the VAE is fused differently for a tap: moments, image and d_z are bit-equal with and without taps, and a tapped
    call launches what the untapped one launches plus one copy per tap."""
    size = V.SIZES[0]
    net = _net("vae_graph", dtype)
    L = net._L()
    cfg, sd, (z, img, cot), ref = V.case("vae_graph", size, "decode")
    count = {}

    def dec(tapped):
        shapes = _shapes(ref) if tapped else {}
        out = _set(net, False, shapes)
        with torch.no_grad():
            image = net.decode(z.to(DEV)).sample
        count["decode", tapped] = L.gyre_last_launch_count()
        grad = _set(net, True, shapes)
        # (called on this thread: the launch count is per thread, and autograd runs a backward on a thread of its own)
        _, dz = net._decode_native(net._handle, z.to(DEV), cot.to(DEV))
        count["vjp", tapped] = L.gyre_last_launch_count()
        torch.cuda.synchronize()
        _written({"out": _cpu(out), "grad": _cpu(grad)})
        return image.cpu(), dz.cpu()
    plain, tapped = dec(False), dec(True)
    assert torch.equal(plain[0], tapped[0]) and torch.equal(plain[1], tapped[1])
    eref = V.case("vae_graph", size, "encode")[3]
    m0 = net.encode(img.to(DEV)).latent_dist.parameters.cpu()
    count["encode", False] = L.gyre_last_launch_count()
    got = _encode(net, img, _shapes(eref))
    count["encode", True] = L.gyre_last_launch_count()
    _written(got)
    assert torch.equal(m0.float(), got["moments"])
    print(f"[vaegraph] vae_graph 8x12 {V.DT_NAME[dtype]} launches untapped / tapped: " +
          "  ".join(f"{k} {count[k, False]} / {count[k, True]}" for k in ("encode", "decode", "vjp")))
    assert count["decode", True] == count["decode", False] + len(ref["out"])
    assert count["vjp", True] == count["vjp", False] + len(ref["out"])
    assert count["encode", True] == count["encode", False] + len(eref["out"])


def test_tap_refusals_and_lifetime():
    size = V.SIZES[0]
    cfg, sd, (z, img, cot), ref = V.case("vae_graph", size, "decode")
    eref = V.case("vae_graph", size, "encode")[3]
    net = _net("vae_graph", torch.bfloat16)
    L, h = net._L(), C.c_void_p(net._handle)
    one, eone = "decoder.mid_block.resnets.1", "encoder.mid_block.resnets.1"
    shape, eshape = {one: ref["out"][one].shape}, {eone: eref["out"][eone].shape}
    buf = torch.full(tuple(shape[one]), NAN, device=DEV)
    # unknown names: nodes this VAE does not have, the UNet's level names, the outputs; an encoder node is no gradient tap
    for fn, bad in ((L.gyre_vae_debug_tap, b"decoder.up_blocks.2.upsamplers.0"), (L.gyre_vae_debug_tap, b"encoder.down_blocks.0.resnets.2"),
                    (L.gyre_vae_debug_tap, b"mid"), (L.gyre_vae_debug_tap, b"decoder.conv_out"), (L.gyre_vae_debug_tap, b"quant_conv"),
                    (L.gyre_vae_debug_grad_tap, eone.encode()), (L.gyre_vae_debug_grad_tap, b"encoder.conv_in"),
                    (L.gyre_vae_debug_grad_tap, b"decoder.conv_out"), (L.gyre_vae_debug_grad_tap, b"decoder.mid")):
        with pytest.raises(ValueError):
            _lib.check(fn(h, bad, C.c_void_p(buf.data_ptr()), buf.numel() * 4), L)
    zd = z.to(DEV).requires_grad_()
    dec = lambda: net.decode(zd).sample
    # four bytes short: the decode refuses a forward tap, the VJP a gradient tap; a refused tap is gone afterwards
    _lib.check(L.gyre_vae_debug_tap(h, one.encode(), C.c_void_p(buf.data_ptr()), buf.numel() * 4 - 4), L)
    with pytest.raises(ValueError):
        dec()
    image = dec()
    _lib.check(L.gyre_vae_debug_grad_tap(h, one.encode(), C.c_void_p(buf.data_ptr()), buf.numel() * 4 - 4), L)
    with pytest.raises(ValueError):
        torch.autograd.grad(image, zd, cot.to(DEV), retain_graph=True)
    (dz,) = torch.autograd.grad(image, zd, cot.to(DEV), retain_graph=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    # taps belong to one call: the second decode / VJP leaves the buffers alone
    bufs = _set(net, False, shape)
    image = dec()                                            # consumes the forward tap
    gbufs = _set(net, True, shape)
    torch.autograd.grad(image, zd, cot.to(DEV), retain_graph=True)       # consumes the gradient tap
    torch.cuda.synchronize()
    for b in (bufs[one], gbufs[one]):
        assert not bool(torch.isnan(b).any())
        b.fill_(NAN)
    (dz2,) = torch.autograd.grad(dec(), zd, cot.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs[one]).all()) and bool(torch.isnan(gbufs[one]).all())
    assert torch.equal(dz, dz2)
    # an encoder node's tap is not written by a decode and is gone after it; a decoder node's likewise with an encode
    ebufs = _set(net, False, eshape)
    dec()
    net.encode(img.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(ebufs[eone]).all())
    dbufs = _set(net, False, shape)
    net.encode(img.to(DEV))
    dec()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbufs[one]).all())
    # the VJP serves gradient taps only: a forward tap set before it waits for the next decode
    image = dec()
    fbufs = _set(net, False, shape)
    torch.autograd.grad(image, zd, cot.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(fbufs[one]).all())
    dec()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(fbufs[one]).any())
