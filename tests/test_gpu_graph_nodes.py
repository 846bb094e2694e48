"""The UNet graph node by node (-m gpu): the output of every node of the activation-keeping forward (gyre_unet_debug_tap) and the
complete gradient of every node's output in the reverse sweep (gyre_unet_debug_grad_tap) against the fp32 oracle, each gated at twice
its own storage-emulation floor (tests/graph_ref.py: config, emulation, floors, verdict; tests/test_graph_ref_host.py shows on the
CPU which seeded wiring mistakes these criteria catch and that the old whole-tensor gates let most of them through).

Both storage flavours run in this process (net.to(torch.bfloat16 | torch.float16)); nothing here reads gpu_util.HDT.
`[graph]` lines carry the measured native distances next to their floors; they are printed, not asserted - the assertions are the
verdicts.  Inputs: B = 2, t = (981, 17), S = 77, latents 16x16 and the odd 9x15."""
import ctypes as C

import pytest
import torch

import graph_ref as G
from gyre_amd import _lib
from gyre_amd.modules import GyreHipUNet, grad_samples
from gpu_util import DEV

pytestmark = pytest.mark.gpu
_REF, _NET = {}, {}
NAN = float("nan")


def _case(name, size, tome_r=0):
    """(cfg, state dict, inputs, fp32 oracle result) of a FLOORS key - computed once and shared, never changed"""
    key = (name, tuple(size), tome_r)
    if key not in _REF:
        cfg = G.CONFIGS[name]
        sd = G.state_dict(cfg)
        x, t, ctx, cot, added = G.inputs(cfg, *size)
        _REF[key] = (cfg, sd, (x, t, ctx, cot, added), G.oracle(sd, cfg, x, t, ctx, cot, tome_r=tome_r, added_cond=added))
    return _REF[key]


def _net(name, dtype):
    if (name, dtype) not in _NET:
        cfg = G.CONFIGS[name]
        net = GyreHipUNet(cfg)
        net.load_state_dict(G.state_dict(cfg))
        net = net.to(dtype).to(DEV)
        x, t, ctx, _, added = G.inputs(cfg, 16, 16)
        with torch.no_grad():                        # uploads the weights, creates the handle
            net(x.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=_dev(added))
        _NET[(name, dtype)] = net
    return _NET[(name, dtype)]


def _dev(added):
    return None if added is None else {k: v.to(DEV) for k, v in added.items()}


def _set(net, grad, shapes):
    """NaN-filled buffers of the given shapes, registered as forward (grad=False) or gradient taps"""
    L = net._L()
    fn = L.gyre_unet_debug_grad_tap if grad else L.gyre_unet_debug_tap
    bufs = {k: torch.full(tuple(sh), NAN, dtype=torch.float32, device=DEV) for k, sh in shapes.items()}
    for k, b in bufs.items():
        _lib.check(fn(C.c_void_p(net._handle), k.encode(), C.c_void_p(b.data_ptr()), b.numel() * 4), L)
    return bufs


def _native(net, x, t, ctx, cot, added, shapes, gshapes=None, rng=None, taps=True, gtaps=True):
    """One keeping forward with every node tap set, then the reverse sweep with every gradient tap set: a result in the layout of
    graph_ref.oracle().  rng = (b0, nb): grad_samples; cot then holds nb samples."""
    out = _set(net, False, shapes) if taps else {}
    xd = x.to(DEV).requires_grad_()
    kw = dict(encoder_hidden_states=ctx.to(DEV), added_cond_kwargs=_dev(added))
    if rng is None:
        eps = net(xd, t.to(DEV), **kw).sample
        target = eps
    else:
        with grad_samples(*rng):
            eps = net(xd, t.to(DEV), **kw).sample
        target = eps[rng[0]:rng[0] + rng[1]]
    grad = _set(net, True, gshapes or shapes) if gtaps else {}
    (dx,) = torch.autograd.grad(target, xd, cot.to(DEV))
    torch.cuda.synchronize()
    return {"eps": eps.detach().float().cpu(), "d_x": dx.float().cpu(), "out": {k: v.cpu() for k, v in out.items()},
            "grad": {k: v.cpu() for k, v in grad.items()}}


def _written(res):
    for grp in ("out", "grad"):
        for k, v in res[grp].items():
            assert not bool(torch.isnan(v).any()), f"{grp} tap {k} was not written completely"


def _judge(label, got, ref, floors, dtype):
    ok, ratios, worst = G.verdict(got, ref, floors, dtype)
    d = G.distances(got, ref)
    tag = f"[graph] {label} {G.DT_NAME[dtype]}"
    print(f"{tag}: eps {d['eps']:.3e} (floor {floors['eps']:.3e})  d_x {d['d_x']:.3e} (floor {floors['d_x']:.3e})")
    for k in ref["out"]:
        print(f"{tag} {k}: out {d['out'][k]:.3e} (floor {floors['out'][k]:.3e})  grad {d['grad'][k]:.3e} (floor {floors['grad'][k]:.3e})")
    for grp, (r, k) in worst.items():
        print(f"{tag} worst {grp}: ratio {r:.3f} at {k}")
    # the first failing node in forward order / the last failing node in sweep order (= the first in forward order) locate a finding
    bad = [(grp, k) for grp in ("out", "grad") for k in ref["out"] if not ratios[grp][k] <= 1.0]
    assert ok, f"{label}: over the gate (distance / (2 x floor) > 1): eps {ratios['eps']:.2f} d_x {ratios['d_x']:.2f} nodes {bad[:6]}"


def _shapes(ref):
    return {k: v.shape for k, v in ref["out"].items()}


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["graph", "graph_lin"])
def test_every_node_output_and_gradient(name, size, dtype):
    cfg, sd, (x, t, ctx, cot, added), ref = _case(name, size)
    got = _native(_net(name, dtype), x, t, ctx, cot, added, _shapes(ref))
    _written(got)
    _judge(f"{name} {size[0]}x{size[1]}", got, ref, G.floors_for(name, size, dtype), dtype)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
def test_every_node_with_token_merging(dtype):
    """ToMe r = 40 against the oracle's tome_r (16x16: both attention levels have a token count that merges)"""
    cfg, sd, (x, t, ctx, cot, added), ref = _case("graph", (16, 16), G.TOME_R)
    net = _net("graph", dtype)
    net.set_tome(G.TOME_R)
    try:
        got = _native(net, x, t, ctx, cot, added, _shapes(ref))
    finally:
        net.set_tome(0)
    _written(got)
    _judge(f"graph 16x16 tome {G.TOME_R}", got, ref, G.floors_for("graph", (16, 16), dtype, G.TOME_R), dtype)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
def test_every_node_of_the_text_time_depth_2_3_net(dtype):
    cfg, sd, (x, t, ctx, cot, added), ref = _case("tiny_sdxl", (16, 16))
    got = _native(_net("tiny_sdxl", dtype), x, t, ctx, cot, added, _shapes(ref))
    _written(got)
    _judge("tiny_sdxl 16x16", got, ref, G.floors_for("tiny_sdxl", (16, 16), dtype), dtype)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
def test_gradient_taps_of_a_sample_range_sweep(dtype):
    """grad_samples(2, 2) on the CFG layout cat[x, x] / cat[t, t] / cat[other context, context]: the forward taps hold four samples, the
    gradient taps the two differentiated ones; that half is the standard case, so its oracle result and floors are the shared ones."""
    cfg, sd, (x, t, ctx, cot, added), ref = _case("graph", (16, 16))
    other = torch.randn(ctx.shape, generator=torch.Generator().manual_seed(12))
    shapes = {k: (4,) + tuple(v.shape[1:]) for k, v in ref["out"].items()}
    got = _native(_net("graph", dtype), torch.cat([x, x]), torch.cat([t, t]), torch.cat([other, ctx]), cot, None, shapes,
                  gshapes=_shapes(ref), rng=(2, 2))
    _written(got)
    assert float(got["d_x"][:2].abs().max()) == 0.0
    half = {"eps": got["eps"][2:], "d_x": got["d_x"][2:], "out": {k: v[2:] for k, v in got["out"].items()}, "grad": got["grad"]}
    _judge("graph 16x16 samples [2, 4) of 4", half, ref, G.floors_for("graph", (16, 16), dtype), dtype)


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
def test_taps_do_not_change_what_runs(dtype):
    """A tapped inference forward loses the proj_out fold and the CFG-pair prefix (include/gyre_hip.h): its eps agrees with the
    untapped one within the eps gate.  The reverse sweep runs the same launches tapped or not: d_x is bit-equal."""
    cfg, sd, (x, t, ctx, cot, added), ref = _case("graph", (16, 16))
    net = _net("graph", dtype)
    floors = G.floors_for("graph", (16, 16), dtype)
    args = (x.to(DEV), t.to(DEV))
    with torch.no_grad():
        plain = net(*args, encoder_hidden_states=ctx.to(DEV)).sample.cpu()
        bufs = _set(net, False, _shapes(ref))
        tapped = net(*args, encoder_hidden_states=ctx.to(DEV)).sample.cpu()
    torch.cuda.synchronize()
    _written({"out": {k: v.cpu() for k, v in bufs.items()}, "grad": {}})
    d = G.rel_l2(tapped, plain)
    print(f"[graph] graph 16x16 {G.DT_NAME[dtype]}: tapped against untapped inference eps {d:.3e} (gate {2 * floors['eps']:.3e})")
    assert d <= 2 * floors["eps"]
    with_taps = _native(net, x, t, ctx, cot, added, _shapes(ref))
    without = _native(net, x, t, ctx, cot, added, _shapes(ref), taps=False, gtaps=False)
    assert torch.equal(with_taps["d_x"], without["d_x"]) and torch.equal(with_taps["eps"], without["eps"])


def test_tap_refusals_and_lifetime():
    cfg, sd, (x, t, ctx, cot, added), ref = _case("graph", (16, 16))
    net = _net("graph", torch.bfloat16)
    L, h = net._L(), C.c_void_p(net._handle)
    one = "mid_block.resnets.1"
    shape = {one: ref["out"][one].shape}
    buf = torch.full(tuple(shape[one]), NAN, device=DEV)
    # unknown names: a node this UNet does not have; a level name is no node for the gradient tap
    for fn, bad in ((L.gyre_unet_debug_tap, b"down_blocks.2.attentions.0"), (L.gyre_unet_debug_tap, b"up_blocks.0.upsamplers.1"),
                    (L.gyre_unet_debug_grad_tap, b"mid"), (L.gyre_unet_debug_grad_tap, b"conv_out")):
        with pytest.raises(ValueError):
            _lib.check(fn(h, bad, C.c_void_p(buf.data_ptr()), buf.numel() * 4), L)
    xd = x.to(DEV).requires_grad_()
    fwd = lambda: net(xd, t.to(DEV), encoder_hidden_states=ctx.to(DEV)).sample
    # too small: the keeping forward refuses a forward tap, the sweep a gradient tap; a refused tap is gone afterwards
    _lib.check(L.gyre_unet_debug_tap(h, one.encode(), C.c_void_p(buf.data_ptr()), buf.numel() * 4 - 4), L)
    with pytest.raises(ValueError):
        fwd()
    eps = fwd()
    _lib.check(L.gyre_unet_debug_grad_tap(h, one.encode(), C.c_void_p(buf.data_ptr()), buf.numel() * 4 - 4), L)
    with pytest.raises(ValueError):
        torch.autograd.grad(eps, xd, cot.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    # taps belong to one call: the second forward / sweep leaves the buffers alone
    first = _native(net, x, t, ctx, cot, added, shape)
    _written(first)
    bufs = _set(net, False, shape)
    eps = fwd()                                              # consumes the forward tap
    gbufs = _set(net, True, shape)
    torch.autograd.grad(eps, xd, cot.to(DEV))                # consumes the gradient tap
    torch.cuda.synchronize()
    for b in (bufs[one], gbufs[one]):
        assert not bool(torch.isnan(b).any())
        b.fill_(NAN)
    torch.autograd.grad(fwd(), xd, cot.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs[one]).all()) and bool(torch.isnan(gbufs[one]).all())
    # a gradient tap left pending when an inference forward drops the kept state is cleared with it
    eps = fwd()
    pend = _set(net, True, shape)
    with torch.no_grad():
        net(x.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV))
    (dx,) = torch.autograd.grad(eps, xd, cot.to(DEV))       # recomputed in one shot: no tap
    torch.cuda.synchronize()
    assert bool(torch.isnan(pend[one]).all())
    assert torch.equal(dx.cpu(), first["d_x"])
