"""T2I-adapter hint conditioning on the HIP path (-m gpu): the three element-wise kernels, the native adapter model against the
fp32 restatement tests/t2i_ref.py (itself pinned to the reference's executed classes in tests/test_t2i_host.py), the pipeline
with hints against the same host code over the oracle models, and the engine's hint_images route.  Both storage flavours run in
this process: module dtype for the models, _lib.lib(storage) for the operators.

Gate of the model tests: rel-L2 <= 2e-2 per feature, the project's per-block bf16-vs-fp32 gate."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import t2i_ref
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hints import T2IHint
from gyre_amd.modules import GyreHipUNet, GyreHipVAE, set_batch_invariant
from gyre_amd.pipeline import GyrePipeline
from gyre_amd.t2i import GyreHipT2IAdapter
from gpu_util import DEV
from oracle import models_ref as M
from oracle import pipeline_ref as PR

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("shape", [(2, 3, 16, 24), (1, 1, 8, 8)])
def test_pixel_unshuffle8_is_bit_equal_to_torch(storage, sdt, shape):
    L = _lib.lib(storage)
    B, c, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    ref = F.pixel_unshuffle(x.to(sdt), 8).permute(0, 2, 3, 1).contiguous()
    for src in (x, x.to(sdt)):                                        # from f32 and from the storage dtype
        y = torch.zeros((B, H // 8, W // 8, 64 * c), dtype=sdt, device=DEV)
        _lib.check(L.gyre_op_pixel_unshuffle8(_st(), _p(src), _lib.dtype_code(src), B, c, H, W, _p(y)), L)
        assert torch.equal(_bits(y), _bits(ref))
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_pixel_unshuffle8(_st(), _p(x), 0, B, c, H - 1, W, _p(y)), L)


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_relu_is_bit_equal_to_torch(storage, sdt, n):
    L = _lib.lib(storage)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV, sdt)
    ref = torch.relu(x)
    _lib.check(L.gyre_op_relu(_st(), _p(x), n), L)
    assert torch.equal(_bits(x), _bits(ref))


@pytest.mark.parametrize("storage,sdt", STORAGES)
@pytest.mark.parametrize("shape", [(2, 5, 6, 40), (1, 2, 2, 8)])
def test_avgpool2_against_float64(storage, sdt, shape):
    """bound per element: u |ref| + 2^-22 mean|x_i| + 2^-24 - one storage rounding plus three fp32 additions"""
    L = _lib.lib(storage)
    B, H, W, Cn = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(DEV, sdt)
    y = torch.zeros((B, H // 2, W // 2, Cn), dtype=sdt, device=DEV)
    _lib.check(L.gyre_op_avgpool2(_st(), _p(x), B, H, W, Cn, _p(y)), L)
    xd = x.double().cpu()[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, Cn)
    ref, mabs = xd.mean(dim=(2, 4)), xd.abs().mean(dim=(2, 4))
    err = (y.double().cpu() - ref).abs()
    bound = UNIT[sdt] * ref.abs() + 2.0 ** -22 * mabs + 2.0 ** -24
    print(f"[t2i] avgpool2 {shape} {sdt}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---- model ----------------------------------------------------------------------------------------------------------------------
CASES = {"main_default": dict(type="main"),
         "main_conv": dict(type="main", ksize=3, sk=False, use_conv=True, cin=64, nums_rb=3, channels=(64, 64, 64, 64)),
         "light": dict(type="light")}


def make(cfg, dtype, seed=1):
    sd = weights.synthetic_state_dict(weights.t2i_param_shapes(cfg), seed)
    net = GyreHipT2IAdapter(cfg)
    net.load_state_dict(sd)
    return net.to(dtype).to(DEV), {k: v.to(dtype).float() for k, v in sd.items()}


def rel_l2(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


def model_errors(cfg, shape, label):
    img = torch.rand(shape, generator=torch.Generator().manual_seed(4))
    errs = {}
    for dtype in (torch.bfloat16, torch.float16):
        net, sd_r = make(cfg, dtype)
        x = img.to(dtype)
        ref = t2i_ref.t2i_forward(sd_r, cfg, x.float())
        got = net(x.to(DEV))
        assert [tuple(g.shape) for g in got] == [tuple(r.shape) for r in ref] and all(g.dtype == dtype for g in got)
        errs[dtype] = [rel_l2(g, r) for g, r in zip(got, ref)]
        print(f"[t2i] {label} {tuple(shape)} {dtype}: rel-L2 per level " + " ".join(f"{e:.2e}" for e in errs[dtype]))
    for dtype, e in errs.items():
        assert max(e) <= 2e-2, (label, dtype, e)
    for eb, eh in zip(errs[torch.bfloat16], errs[torch.float16]):
        assert eh < eb, (label, errs)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("hw", [(2, 128, 128), (1, 64, 96)])
def test_tiny_adapters_match_the_restatement(name, hw):
    kw = dict(CASES[name])
    cfg = gcfg.tiny_t2i(kw.pop("type"), **kw)
    model_errors(cfg, (hw[0], cfg.cin // 64, hw[1], hw[2]), name)


def test_full_size_main_adapter_matches_the_restatement():
    model_errors(gcfg.t2i_config("main"), (1, 3, 512, 512), "full-size main")


def test_workspace_is_exact_and_results_are_deterministic_and_batch_invariant():
    cfg = gcfg.tiny_t2i("main")
    net, _ = make(cfg, torch.bfloat16)
    img = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(8)).to(DEV)
    a = net(img)
    b = net(img)
    assert all(torch.equal(x, y) for x, y in zip(a, b))               # a second call is bit-identical
    L, h = net._L(), C.c_void_p(net._handle)
    need = L.gyre_t2i_workspace_bytes(h, 2, 64, 96)
    assert need > 0 and need % 256 == 0

    def raw(nbytes):
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        outs = [torch.empty_like(t) for t in a]
        arr = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
        rc = L.gyre_t2i_forward(h, _st(), _p(img), 0, 2, 64, 96, C.c_void_p((ws.data_ptr() + 255) & ~255), nbytes, arr, 4, _lib.BF16)
        torch.cuda.synchronize()
        return rc, outs
    rc, outs = raw(need)                                              # the dry run's peak is enough ...
    assert rc == 0 and all(torch.equal(x, y) for x, y in zip(a, outs))
    assert raw(need - 256)[0] == -4                                   # ... and nothing less is: it IS the high-water mark
    with pytest.raises(ValueError):
        net(img[:, :, :60])
    prev = set_batch_invariant(16)
    try:
        full = net(img)
        for i in range(2):
            one = net(img[i:i + 1].contiguous())
            assert all(torch.equal(f[i:i + 1], o) for f, o in zip(full, one))
    finally:
        set_batch_invariant(prev)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
class OracleUNet:
    def __init__(self, sd, cfg):
        self.sd, self.config = sd, cfg

    def __call__(self, latents, t, encoder_hidden_states=None, adapter_states=None, **_):
        t = torch.as_tensor(t)
        if t.ndim == 0:
            t = t.expand(latents.shape[0])
        return SimpleNamespace(sample=M.unet_forward(self.sd, self.config, latents, t, encoder_hidden_states, adapter_states=adapter_states))


class OracleAdapter:
    _coadapter_type = False

    def __init__(self, sd, cfg):
        self.sd, self.config = sd, cfg

    def __call__(self, image):
        return t2i_ref.t2i_forward(self.sd, self.config, image)


@pytest.fixture(scope="module")
def tiny():
    from test_host_pipeline import OracleVAE
    ucfg, vcfg, acfg = gcfg.tiny_unet(), gcfg.tiny_vae(), gcfg.tiny_t2i("main")
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg))
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg))
    asd = weights.synthetic_state_dict(weights.t2i_param_shapes(acfg), 1)
    unet, vae, adapter = GyreHipUNet(ucfg), GyreHipVAE(vcfg), GyreHipT2IAdapter(acfg)
    unet.load_state_dict(usd); vae.load_state_dict(vsd); adapter.load_state_dict(asd)
    pipe = GyrePipeline(unet.to(DEV), vae.to(DEV), device=DEV)
    ref_pipe = GyrePipeline(OracleUNet(usd, ucfg), OracleVAE(vsd, vcfg), device="cpu")
    g = torch.Generator().manual_seed(5)
    text = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g)
    unc = torch.randn(1, 77, ucfg.cross_attention_dim, generator=g).expand(2, -1, -1).contiguous()
    image = torch.rand(1, 3, 128, 128, generator=g)
    return SimpleNamespace(pipe=pipe, ref_pipe=ref_pipe, adapter=adapter.to(DEV), oracle_adapter=OracleAdapter(asd, acfg), text=text,
                           unc=unc, image=image, unet=unet)


def test_pipeline_with_hints_matches_the_oracle_and_its_own_variants(tiny, monkeypatch):
    kw = dict(seeds=[5, 6], text_embeddings=tiny.text, uncond_embeddings=tiny.unc, height=128, width=128, num_inference_steps=4,
              sampler="euler")
    hint = lambda **h: [T2IHint(tiny.adapter, tiny.image.to(DEV), **h)]
    plain = tiny.pipe(**kw).cpu()
    got = tiny.pipe(t2i_hints=hint(weight=0.8, soft_injection=True), **kw).cpu()
    ref = tiny.ref_pipe(t2i_hints=[T2IHint(tiny.oracle_adapter, tiny.image, weight=0.8, soft_injection=True)], **kw)
    p, moved = PR.psnr(got, ref), PR.psnr(got, plain)
    print(f"[parity] tiny txt2img + T2I hint, euler 4 steps: PSNR {p:.1f} dB vs oracle; {moved:.1f} dB vs the un-hinted run")
    assert p >= 30.0
    assert not torch.equal(got, plain) and moved < p                  # the hint matters
    assert torch.equal(tiny.pipe(t2i_hints=hint(weight=0.0), **kw).cpu(), plain)     # weight 0: adding zeros changes no bit
    lat = dict(kw, output_type="latent")
    only = tiny.pipe(t2i_hints=hint(weight=0.8, soft_injection=True, cfg_only=True), **lat)
    assert not torch.equal(only, tiny.pipe(t2i_hints=hint(weight=0.8, soft_injection=True), **lat))
    # the shared CFG prefix ends before the level-0 add: with it or without it, the same bits
    monkeypatch.setenv("GYRE_CFG_SHARED_PREFIX", "0")
    assert torch.equal(only, tiny.pipe(t2i_hints=hint(weight=0.8, soft_injection=True, cfg_only=True), **lat))
    monkeypatch.delenv("GYRE_CFG_SHARED_PREFIX")
    seq = tiny.pipe(t2i_hints=hint(weight=0.8, soft_injection=True, cfg_only=True), cfg_execution="sequential", **lat)
    assert torch.equal(only, seq)                                     # (the existing parallel-vs-sequential gate: bit for bit)
    one = tiny.pipe(t2i_hints=hint(weight=0.8), guidance_scale=1.0, **lat)
    assert bool(torch.isfinite(one).all())


def test_adapter_states_of_the_wrong_size_are_refused(tiny):
    """latent height 9: the adapter's average pools give 9, 4, 2, 1 rows, the UNet's stride-2 convolutions 9, 5, 3, 2"""
    states = tiny.adapter(torch.rand(1, 3, 72, 64).to(DEV))
    assert [s.shape[2] for s in states] == [9, 4, 2, 1]
    x = torch.randn(1, 4, 9, 8).to(DEV)
    ctx = torch.randn(1, 77, tiny.unet.config.cross_attention_dim).to(DEV)
    with pytest.raises(ValueError):
        tiny.unet(x, 500, encoder_hidden_states=ctx, adapter_states=states)


def test_engine_hint_images_route(tiny):
    from test_gpu_engine import build_engine, generators, sample_euler_ancestral, wrapper_kwargs
    ucfg, vcfg = gcfg.tiny_unet(), gcfg.tiny_vae()
    manager = SimpleNamespace(for_type=lambda t, default=None: {"sketch": {"sketch": tiny.adapter, "clip_model": None}}.get(t, default))
    _, _, eng = build_engine(ucfg, vcfg, hintset_manager=manager)
    eng.scheduler = sample_euler_ancestral
    seeds, prompt = [7, 8], ["a lighthouse", "a cat"]
    hint = SimpleNamespace(image=tiny.image, hint_type="sketch", weight=0.8, priority="prompt", clip_layer=None)
    args = wrapper_kwargs(prompt=prompt, negative_prompt=None, generator=generators(seeds), width=128, height=128, num_inference_steps=4)
    out = eng(**{**args, "hint_images": [hint]})
    assert isinstance(out, tuple) and len(out) == 2
    images, nsfw = out
    assert images.shape == (2, 3, 128, 128) and images.dtype == torch.float32 and images.device.type == "cpu" and nsfw == [False, False]
    cond, unc = eng._embed(prompt, None, 2, 1, True, 3)
    direct = GyrePipeline(eng.unet, eng.vae, None, device=eng.execution_device)(
        generators=generators(seeds), text_embeddings=cond, uncond_embeddings=unc, height=128, width=128, num_inference_steps=4,
        sampler="euler_a", t2i_hints=[T2IHint(tiny.adapter, tiny.image.to(DEV), weight=0.8, soft_injection=True, cfg_only=False)])
    assert torch.equal(images, direct.float().cpu())
    plain, _ = eng(**{**args, "generator": generators(seeds)})
    assert not torch.equal(images, plain)
    controlnet = SimpleNamespace(for_type=lambda t, default=None: {"model": torch.nn.Linear(1, 1)})
    eng.hintset_manager = controlnet
    with pytest.raises(NotImplementedError):
        eng(**{**args, "hint_images": [hint]})
