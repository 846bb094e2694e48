"""Derived weight copies after a whole re-upload, and the one trunk the UNet and the ControlNet register (-m gpu).

A handle keeps copies derived from its weights (csrc/model_impl.h Store::derived: transposed, LayerNorm-folded, packed, blocked,
shortcut-folded, composed proj_out), each refreshed by its user when any weight was set since.  ``load_state_dict`` on a live module
re-uploads EVERY key into the same handle; a forward afterwards that read one stale copy would differ from a fresh handle's.

  1. the (64, 128) UNet of tests/test_gpu_proj_out_fold.py at 32 x 32 latents, B = 2, S = 77: forward, reload seed 2, forward ==
     a fresh seed-2 twin's, bit for bit; and the input gradient of the tiny UNet at 16 x 16, B = 2, in the same way.
     What the planner (kernels_gemm.hip pick_cfg / gemm_plan) gives these shapes: no output tiling reaches the 160 tiles the 8-wave
     and pipelined configs ask for (M = 2048 / 512 rows, N <= 1024), N is no multiple of 160 / 256 / 320 where K >= 2048, and
     M < 4096 rules the A-resident kernel out - so every 3x3 convolution (K = 576 ... 2304) runs on the register-staged 4-wave tiles
     (configs 1 - 3) and every linear layer on them or on the small-problem kernel (config 32, K <= 640).  Of the six kinds that
     leaves
       composed proj_out   populated: every transformer folds (C = 64 / 128 are whole 64-channel K steps, C x HW = 65536 / 32768
                           >= 8192) - the forward pass
       transposed          populated: every linear and convolution the reverse sweep crosses - the gradient pass
       blocked             not populated: configs 1 - 3 read no blocked copy (the convolutions with K = 1152 > 1024), and no linear
                           layer on config 32 has K > 1024
       LayerNorm-folded    not populated: configs 1 - 3 and 32 fold no LayerNorm, and the fused cross-attention needs C = 320
       packed              not populated: no A-resident launch
       shortcut-folded     not populated: config 24 only
     (the other four go through the same Store::derived lookup);
  2. the tiny ControlNet at 16 x 16, B = 2, S = 7: bind, forward, reload seed 2 - the handle is unbound, forward raises - bind,
     forward: all 13 residuals == a fresh seed-2 twin's;
  3. the native key enumeration of the tiny ControlNet without its controlnet_* keys is that of the tiny UNet up to the first
     up_blocks. key, in order: the two handles register one trunk.
"""
import ctypes as C

import pytest
import torch

from gyre_amd import config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV, randn

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def small_cfg():
    return gcfg.UNetConfig(block_out_channels=(64, 128), attn_levels=(True, True), num_heads=(2, 4), transformer_depth=(1, 2),
                           cross_attention_dim=64, sample_size=16)


def unet(cfg, seed, dtype):
    net = GyreHipUNet(cfg)
    net.load_state_dict(weights.synthetic_state_dict(weights.unet_param_shapes(cfg), seed))
    return net.to(dtype).to(DEV)


def controlnet(cfg, seed, dtype):
    net = GyreHipControlNet(cfg)
    net.load_state_dict(weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), seed))
    return net.to(dtype).to(DEV)


def native_keys(net):
    h = C.c_void_p(net._sync(torch.device(DEV)))
    L, kind = net._L(), net._kind
    n = getattr(L, f"gyre_{kind}_num_params")(h)
    return [getattr(L, f"gyre_{kind}_param_key")(h, i).decode() for i in range(n)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_unet_forward_after_a_whole_reupload_equals_a_fresh_handle(dtype):
    cfg = small_cfg()
    x = randn(2, 4, 32, 32, seed=31).to(dtype).to(DEV)
    t = torch.tensor([640, 25], device=DEV)
    ctx = randn(2, 77, cfg.cross_attention_dim, seed=32).to(dtype).to(DEV)

    def fwd(net):
        return net(x, t, encoder_hidden_states=ctx).sample.clone()
    net = unet(cfg, 1, dtype)
    first = fwd(net)                                         # the derived copies of seed 1 exist from here on
    handle = net._handle
    net.load_state_dict(weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 2))
    got = fwd(net)
    assert net._handle == handle                             # the same native handle, every key set again
    assert not torch.equal(got, first)
    assert torch.equal(got, fwd(unet(cfg, 2, dtype))), "a derived copy of the old weights was read"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_unet_input_gradient_after_a_whole_reupload_equals_a_fresh_handle(dtype):
    cfg = gcfg.tiny_unet()
    x = randn(2, 4, 16, 16, seed=41).to(dtype).to(DEV)
    t = torch.tensor([981, 17], device=DEV)
    ctx = randn(2, 77, cfg.cross_attention_dim, seed=42).to(dtype).to(DEV)
    cot = randn(2, cfg.out_channels, 16, 16, seed=43).to(dtype).to(DEV)

    def grad(net):
        xd = x.clone().requires_grad_()
        (g,) = torch.autograd.grad(net(xd, t, encoder_hidden_states=ctx).sample, xd, cot)
        return g.clone()
    net = unet(cfg, 1, dtype)
    first = grad(net)                                        # the transposed copies of seed 1 exist from here on
    net.load_state_dict(weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 2))
    got = grad(net)
    assert not torch.equal(got, first)
    assert torch.equal(got, grad(unet(cfg, 2, dtype))), "a transposed copy of the old weights was read"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_controlnet_after_a_whole_reupload_is_unbound_and_then_equals_a_fresh_handle(dtype):
    cfg = gcfg.tiny_controlnet()
    g = torch.Generator().manual_seed(51)
    x = torch.randn(2, 4, 16, 16, generator=g).to(dtype).to(DEV)
    ctx = torch.randn(2, 7, cfg.cross_attention_dim, generator=g).to(dtype).to(DEV)
    img = torch.rand(2, 3, 128, 128, generator=g).to(dtype).to(DEV)
    net = controlnet(cfg, 1, dtype)
    net.bind(img, ctx)
    first = [o.clone() for o in net(x, 400)]
    net.load_state_dict(weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), 2))
    with pytest.raises(ValueError):
        net(x, 400)                                          # the embedding and the projected context went with the weights
    net.bind(img, ctx)
    got = [o.clone() for o in net(x, 400)]
    twin = controlnet(cfg, 2, dtype)
    twin.bind(img, ctx)
    ref = twin(x, 400)
    assert len(got) == 13 and len(ref) == 13
    assert all(not torch.equal(a, b) for a, b in zip(got, first))
    assert all(torch.equal(a, b) for a, b in zip(got, ref)), "a derived copy of the old weights was read"


def test_unet_and_controlnet_register_one_trunk():
    ck = [k for k in native_keys(controlnet(gcfg.tiny_controlnet(), 0, torch.bfloat16)) if not k.startswith("controlnet_")]
    uk = native_keys(unet(gcfg.tiny_unet(), 0, torch.bfloat16))
    first_up = next(i for i, k in enumerate(uk) if k.startswith("up_blocks."))
    assert first_up > 100 and ck[-1].startswith("mid_block.")
    assert ck == uk[:first_up]
