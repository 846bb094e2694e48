"""Bind slots, residual masks and the latent mask of the native ControlNet (-m gpu; gyre_ctrl_bind_slot / gyre_ctrl_forward_slot behind
GyreHipControlNet.bind(slot=, masks=) / forward(slot=, x_mask=)), on the tiny config of tests/test_gpu_ctrl_model.py in both storage
flavours.  Equal-shaped calls of this library are bit-deterministic, so everything here is held to bit equality:

  - two slots bound to different images, sizes and contexts and run alternately give what a fresh model gives that was bound to one of
    them alone through the old entry points (slot 0, no mask: the shell then calls gyre_ctrl_bind / gyre_ctrl_forward themselves);
  - a masked slot with float32 outputs gives the unmasked float32 residual times the mask in float32 (one more correctly rounded product);
  - x_mask gives what the unmasked forward gives on latents multiplied on the host.  The latents are taken in the model's own storage
    dtype (bfloat16 / float16): the kernel rounds the fp32 product x m once to storage, the host product ``(x.float() * m).to(dtype)`` is
    that same single rounding, and the plain entry pass then copies storage values unchanged - so the two are exactly equal.
"""
import ctypes as C
import functools

import pytest
import torch

from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gpu_util import DEV

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
B = 2


@functools.lru_cache(maxsize=None)
def state():
    cfg = gcfg.tiny_controlnet()
    return cfg, weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), 1)


def fresh(dtype):
    cfg, sd = state()
    net = GyreHipControlNet(cfg)
    net.load_state_dict(sd)
    return net.to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def shared(dtype):
    return fresh(dtype)


def request(cfg, h, w, S, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, h, w, generator=g).to(dtype).to(DEV)
    ctx = torch.randn(B, S, cfg.cross_attention_dim, generator=g).to(dtype).to(DEV)
    img = torch.rand(1, 3, 8 * h, 8 * w, generator=g).to(dtype).to(DEV)
    return x, ctx, img


def alone(dtype, x, ctx, img, t, **kw):
    """a fresh model bound to this one request through the old entry points"""
    net = fresh(dtype)
    net.bind(img, ctx)
    return [o.clone() for o in net(x, t, **kw)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_slots_interleaved_are_two_models(dtype):
    net = shared(dtype)
    cfg = net.config
    xa, ca, ia = request(cfg, 8, 8, 7, dtype, 1)           # image 64 x 64
    xb, cb, ib = request(cfg, 12, 8, 11, dtype, 2)         # image 96 x 64, another context length
    want_a, want_b = alone(dtype, xa, ca, ia, 400), alone(dtype, xb, cb, ib, 30)
    net.bind(ia, ca, slot=0)
    net.bind(ib, cb, slot=1)
    for _ in range(2):                                     # 0, 1, 0, 1
        assert same([o.clone() for o in net(xa, 400, slot=0)], want_a)
        assert same([o.clone() for o in net(xb, 30, slot=1)], want_b)
    net.bind(ib, cb, slot=3)                               # the last slot, and a slot bound while others are live
    assert same([o.clone() for o in net(xb, 30, slot=3)], want_b)
    assert same([o.clone() for o in net(xa, 400, slot=0)], want_a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask_batch", [1, B])
def test_masked_slot_is_the_unmasked_residual_times_the_mask(dtype, mask_batch):
    net = shared(dtype)
    cfg = net.config
    x, ctx, img = request(cfg, 12, 8, 9, dtype, 3)
    g = torch.Generator().manual_seed(5)
    shapes = net.residual_shapes(12, 8)
    masks = [torch.rand(mask_batch, 1, rh, rw, generator=g) for _, rh, rw in shapes]
    masks[0][:, :, :, : 4] = 0.0                           # a hard edge: exact zeros on the left half of the first residual
    scales = [0.8 * float(s) for s in torch.logspace(-1, 0, len(shapes))]
    plain = net.new_outputs(B, 12, 8, DEV, dtype=torch.float32)
    net.bind(img, ctx, slot=0)
    net(x, 321, scales=scales, out=plain, slot=0)
    got = net.new_outputs(B, 12, 8, DEV, dtype=torch.float32)
    net.bind(img, ctx, slot=2, masks=masks)
    net(x, 321, scales=scales, out=got, slot=2)
    for o, p, m in zip(got, plain, masks):
        assert torch.equal(o, p * m.to(DEV))               # float32 x float32 on the device: the correctly rounded product
    assert bool((got[0][:, :, :, : 4] == 0).all()) and float(got[0].abs().max()) > 0
    # accumulate on top of the unmasked residuals, into the upper half of a doubled batch
    both = net.new_outputs(2 * B, 12, 8, DEV, dtype=torch.float32)
    net(x, 321, scales=scales, out=both, slot=0, out_batch=2 * B, out_offset=B)
    net(x, 321, scales=scales, out=both, slot=2, out_batch=2 * B, out_offset=B, accumulate=True)
    for o, p, m in zip(both, plain, masks):
        assert bool((o[:B] == 0).all()) and torch.equal(o[B:], p + p * m.to(DEV))
    # rebinding the slot without masks takes them off again
    net.bind(img, ctx, slot=2)
    again = net.new_outputs(B, 12, 8, DEV, dtype=torch.float32)
    net(x, 321, scales=scales, out=again, slot=2)
    assert same(again, plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask_batch", [1, B])
def test_x_mask_is_the_forward_of_premultiplied_latents(dtype, mask_batch):
    net = shared(dtype)
    cfg = net.config
    x, ctx, img = request(cfg, 8, 8, 7, dtype, 4)          # latents in the model's storage dtype (see the module docstring)
    m = torch.rand(mask_batch, 1, 8, 8, generator=torch.Generator().manual_seed(6))
    m[:, :, :3] = 0.0
    m[:, :, 5:] = 1.0
    pre = (x.float() * m.to(DEV)).to(dtype)
    want = alone(dtype, pre, ctx, img, 77)
    net.bind(img, ctx, slot=1)
    got = [o.clone() for o in net(x, 77, slot=1, x_mask=m.to(DEV))]
    assert same(got, want)
    assert not same(got, [o.clone() for o in net(x, 77, slot=1)])
    net.bind(img, ctx)                                     # slot 0 with a latent mask: the slot entry point on the old bind
    assert same([o.clone() for o in net(x, 77, x_mask=m.to(DEV))], want)


def _raw(net):
    L, dev = net._L(), torch.device(DEV)
    return L, C.c_void_p(net._sync(dev)), C.c_void_p(_lib.stream_ptr(dev))


def raw_bind(net, slot, img, ctx, masks=None, hw=None, mask_B=0):
    L, h, st = _raw(net)
    Bi, _, H, W = img.shape
    need = L.gyre_ctrl_bind_workspace_bytes(h, Bi, H, W, ctx.shape[0])
    ws = net._workspace(need, torch.device(DEV))
    n = 0 if masks is None else len(masks)
    marr = None if masks is None else (C.c_void_p * n)(*[None if m is None else m.data_ptr() for m in masks])
    harr = None if hw is None else (C.c_int32 * len(hw))(*hw)
    return L.gyre_ctrl_bind_slot(h, st, slot, C.c_void_p(img.data_ptr()), _lib.dtype_code(img), Bi, H, W, C.c_void_p(ctx.data_ptr()),
                                 _lib.dtype_code(ctx), ctx.shape[0], ctx.shape[1], marr, harr, n, mask_B,
                                 C.c_void_p((ws.data_ptr() + 255) & ~255), need)


def raw_forward(net, slot, x, S, outs, x_mask=None, x_mask_B=0):
    L, h, st = _raw(net)
    Bx, _, H, W = x.shape
    need = L.gyre_ctrl_workspace_bytes(h, Bx, H, W, S)
    ws = net._workspace(need, torch.device(DEV))
    t = torch.full((Bx,), 10, dtype=torch.int64, device=DEV)
    n = len(outs)
    rc = L.gyre_ctrl_forward_slot(h, st, slot, C.c_void_p(x.data_ptr()), _lib.dtype_code(x), None if x_mask is None else C.c_void_p(x_mask.data_ptr()),
                                  x_mask_B, C.c_void_p(t.data_ptr()), Bx, H, W, C.c_void_p((ws.data_ptr() + 255) & ~255), need,
                                  (C.c_float * n)(*([1.0] * n)), 0, Bx, 0, (C.c_void_p * n)(*[o.data_ptr() for o in outs]), n, _lib.dtype_code(outs[0]))
    torch.cuda.synchronize()
    return rc


def test_error_cases_and_set_weight_drops_every_slot():
    dtype = torch.bfloat16
    net = fresh(dtype)
    cfg = net.config
    x, ctx, img = request(cfg, 8, 8, 7, dtype, 8)
    outs = net.new_outputs(B, 8, 8, DEV)
    shapes = net.residual_shapes(8, 8)
    masks = [torch.ones(1, 1, rh, rw, device=DEV) for _, rh, rw in shapes]
    hw = [v for _, rh, rw in shapes for v in (rh, rw)]
    assert raw_bind(net, 0, img, ctx) == 0 and raw_bind(net, 1, img, ctx, masks, hw, 1) == 0
    assert raw_forward(net, 0, x, 7, outs) == 0 and raw_forward(net, 1, x, 7, outs) == 0
    for slot in (-1, 4):                                                            # a slot outside [0, GYRE_CTRL_SLOTS)
        assert raw_bind(net, slot, img, ctx) == -1 and raw_forward(net, slot, x, 7, outs) == -1
        assert _raw(net)[0].gyre_ctrl_bind_slot_workspace_bytes(_raw(net)[1], slot, 1, 64, 64, B) == 0
    assert raw_forward(net, 2, x, 7, outs) == -1                                    # an unbound slot
    x2 = torch.zeros(B, 4, 12, 8, dtype=dtype, device=DEV)
    assert raw_forward(net, 1, x2, 7, net.new_outputs(B, 12, 8, DEV)) == -1          # a geometry other than the slot's
    assert raw_forward(net, 1, x[:1], 7, net.new_outputs(1, 8, 8, DEV)) == -1        # a batch other than the slot's
    assert raw_forward(net, 0, x, 7, outs, torch.ones(3, 1, 8, 8, device=DEV), 3) == -1    # a latent mask batch that is neither 1 nor B
    bad = list(hw)
    bad[2 * 4] += 1
    assert raw_bind(net, 2, img, ctx, masks, bad, 1) == -1                          # a mask whose size is not the residual's
    assert raw_bind(net, 2, img, ctx, masks[:-1], hw[:-2], 1) == -1                 # too few masks
    assert raw_bind(net, 2, img, ctx, [None] + masks[1:], hw, 1) == -1              # partly null
    assert raw_bind(net, 2, img, ctx, masks, hw, 3) == -1                           # a mask batch that is neither 1 nor B
    assert raw_forward(net, 2, x, 7, outs) == -1                                    # none of those bound the slot
    assert raw_bind(net, 2, img, ctx, [None] * len(masks), hw, 1) == 0              # all null: unmasked
    assert raw_forward(net, 2, x, 7, outs) == 0
    with pytest.raises(ValueError):
        net.bind(img, ctx, slot=4)
    with pytest.raises(ValueError):
        net(x, 10, slot=3)                                                          # the shell knows its unbound slots too
    with pytest.raises(ValueError):
        net.bind(img, ctx, slot=1, masks=masks[:-1])
    # new weights: every slot is dropped, in the shell and in the library
    net.bind(img, ctx, slot=0)
    net.bind(img, ctx, slot=1)
    with torch.no_grad():
        next(net.parameters()).mul_(1.0)
    net._invalidate()
    with pytest.raises(ValueError):
        net(x, 10, slot=1)
    for slot in (0, 1, 2):                                                          # (_raw uploads the weights again: gyre_ctrl_set_weight)
        assert raw_forward(net, slot, x, 7, outs) == -1
    net.bind(img, ctx, slot=1)
    assert same([o.clone() for o in net(x, 10, slot=1)], alone(dtype, x, ctx, img, 10))
