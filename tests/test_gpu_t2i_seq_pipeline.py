"""Style adapters and co-adapters in the request route (-m gpu): the pipeline with a style hint (context 77 + 3 and 154 + 3 rows), with a
co-adapter pair and its fuser, and with both under sequential and parallel CFG, each against the same host flow (gyre_amd/hints.py) over
the oracle models and the restated networks of tests/t2i_seq_ref.py at the PSNR gate of tests/test_gpu_t2i.py; the engine's
hint_images -> _hints -> build_t2i_conditioning route with a fake hintset manager; and that nothing of a style context stays behind for
the next request."""
from types import SimpleNamespace

import pytest
import torch

import t2i_ref
import t2i_seq_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.hints import CoAdapterHint, StyleHint
from gyre_amd.modules import GyreHipUNet, GyreHipVAE
from gyre_amd.pipeline import GyrePipeline
from gyre_amd.t2i import GyreHipT2IAdapter, GyreHipT2IFuser, GyreHipT2IStyleAdapter
from gpu_util import DEV
from oracle import pipeline_ref as PR
from test_gpu_t2i import OracleAdapter, OracleUNet

pytestmark = pytest.mark.gpu
GATE = 30.0                                                         # dB, the gate of test_gpu_t2i's pipeline test


class FakeVision:
    """a stand-in for CLIPModel.vision_model: hidden states [N, 5, width] that depend on the preprocessed image, one per layer"""

    def __init__(self, width):
        g = torch.Generator().manual_seed(17)
        self.proj = [torch.randn((3 * 16, 5 * width), generator=g) * 0.3 for _ in range(4)]
        self.width = width

    def __call__(self, image, output_hidden_states=False, return_dict=True):
        pooled = torch.nn.functional.adaptive_avg_pool2d(image.float().cpu(), 4).flatten(1)
        hs = [(pooled @ p).view(-1, 5, self.width).to(image.device) for p in self.proj]
        return SimpleNamespace(last_hidden_state=hs[-1], hidden_states=hs if output_hidden_states else None)


class OracleStyle:
    dtype, _coadapter_type = torch.float32, False

    def __init__(self, sd, cfg, cotype=False):
        self.sd, self.cfg, self._coadapter_type = sd, cfg, cotype

    def __call__(self, x):
        return R.style_net(self.sd, self.cfg, x.float())


@pytest.fixture(scope="module")
def tiny():
    from test_host_pipeline import OracleVAE
    ucfg, vcfg, acfg = gcfg.tiny_unet(), gcfg.tiny_vae(), gcfg.tiny_t2i("main")
    scfg, fcfg = gcfg.tiny_t2i_style(), gcfg.tiny_t2i_fuser()
    assert scfg.context_dim == ucfg.cross_attention_dim == fcfg.width and tuple(acfg.channels) == tuple(fcfg.unet_channels)
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg))
    vsd = weights.synthetic_state_dict(weights.vae_param_shapes(vcfg))
    asd = [weights.synthetic_state_dict(weights.t2i_param_shapes(acfg), seed) for seed in (1, 2)]
    ssd = weights.synthetic_state_dict(weights.t2i_style_param_shapes(scfg), 31)
    fsd = weights.synthetic_state_dict(weights.t2i_fuser_param_shapes(fcfg), 32)

    def native(cls, cfg, sd, cotype=False):
        m = cls(cfg)
        m.load_state_dict(sd)
        m._coadapter_type = cotype
        return m.to(DEV)

    unet, vae = GyreHipUNet(ucfg), GyreHipVAE(vcfg)
    unet.load_state_dict(usd); vae.load_state_dict(vsd)
    g = torch.Generator().manual_seed(5)
    text = torch.randn(2, 154, ucfg.cross_attention_dim, generator=g)
    unc = torch.randn(1, 154, ucfg.cross_attention_dim, generator=g).expand(2, -1, -1).contiguous()
    oracle_fuser = lambda feats: R.fuser_net(fsd, fcfg, list(feats.items()))
    oracle_adapters = [OracleAdapter(asd[0], acfg), OracleAdapter(asd[1], acfg)]
    oracle_adapters[0]._coadapter_type, oracle_adapters[1]._coadapter_type = "sketch", "depth"
    return SimpleNamespace(
        ucfg=ucfg, vcfg=vcfg, usd=usd, vsd=vsd,
        pipe=GyrePipeline(unet.to(DEV), vae.to(DEV), device=DEV), ref_pipe=GyrePipeline(OracleUNet(usd, ucfg), OracleVAE(vsd, vcfg), device="cpu"),
        sketch=native(GyreHipT2IAdapter, acfg, asd[0], "sketch"), depth=native(GyreHipT2IAdapter, acfg, asd[1], "depth"),
        style=native(GyreHipT2IStyleAdapter, scfg, ssd), costyle=native(GyreHipT2IStyleAdapter, scfg, ssd, "style"),
        fuser=native(GyreHipT2IFuser, fcfg, fsd), oracle_adapters=oracle_adapters, oracle_fuser=oracle_fuser,
        oracle_style=OracleStyle(ssd, scfg), oracle_costyle=OracleStyle(ssd, scfg, "style"),
        clip=SimpleNamespace(vision_model=FakeVision(scfg.width)),
        fe=SimpleNamespace(image_mean=[0.48, 0.46, 0.41], image_std=[0.27, 0.26, 0.28], size={"shortest_edge": 32}),
        text=text, unc=unc, images=[torch.rand(1, 3, 128, 128, generator=g) for _ in range(3)])


def _hints(t, which, on_gpu):
    """the hint objects of a case, bound to the native modules (on_gpu) or to the oracle ones"""
    dev = DEV if on_gpu else "cpu"
    img = [i.to(dev) for i in t.images]
    fuser = t.fuser if on_gpu else t.oracle_fuser
    out = []
    if "style" in which:
        out.append(StyleHint(t.style if on_gpu else t.oracle_style, img[2], t.clip, t.fe, weight=2.5, cfg_only=True, clip_layer="penultimate"))
    if "pair" in which:
        a = (t.sketch, t.depth) if on_gpu else t.oracle_adapters
        out.append(CoAdapterHint(a[0], img[0], fuser, weight=0.8))
        out.append(CoAdapterHint(a[1], img[1], fuser, weight=0.7, soft_injection=True))
    if "costyle" in which:
        out.append(StyleHint(t.costyle if on_gpu else t.oracle_costyle, img[2], t.clip, t.fe, fuser=fuser, weight=0.9, clip_layer=3))
    return out


def _kw(t, rows=77, **extra):
    return dict(seeds=[5, 6], text_embeddings=t.text[:, :rows].contiguous(), uncond_embeddings=t.unc[:, :rows].contiguous(), height=128,
                width=128, num_inference_steps=4, sampler="euler", **extra)


def _against_oracle(t, which, label, **kw):
    got = t.pipe(t2i_hints=_hints(t, which, True), **kw).cpu()
    ref = t.ref_pipe(t2i_hints=_hints(t, which, False), **kw)
    plain = t.pipe(**kw).cpu()
    p, moved = PR.psnr(got, ref), PR.psnr(got, plain)
    print(f"[parity] tiny txt2img + {label}: PSNR {p:.1f} dB vs oracle; {moved:.1f} dB vs the un-hinted run")
    assert p >= GATE
    assert not torch.equal(got, plain) and moved < p                  # the hints matter
    return got


@pytest.mark.parametrize("rows", [77, 154])
def test_style_hint_extends_the_context(tiny, rows):
    _against_oracle(tiny, ("style",), f"style hint, context {rows} + 3", **_kw(tiny, rows))


def test_coadapter_pair_with_its_fuser(tiny):
    _against_oracle(tiny, ("pair",), "co-adapter pair", **_kw(tiny))


@pytest.mark.parametrize("cfg_execution", ["parallel", "sequential"])
def test_coadapters_and_styles_together(tiny, cfg_execution):
    _against_oracle(tiny, ("style", "pair", "costyle"), f"style + co-adapter pair + style co-adapter, {cfg_execution} CFG",
                    **_kw(tiny, cfg_execution=cfg_execution))


def test_without_cfg_and_refusals(tiny):
    one = tiny.pipe(t2i_hints=_hints(tiny, ("style", "pair"), True), guidance_scale=1.0, output_type="latent", **_kw(tiny))
    assert bool(torch.isfinite(one).all())
    with pytest.raises(NotImplementedError):                        # hires fix: the natural-size leaf would need its own states
        big = 2 * 8 * getattr(tiny.ucfg, "sample_size", 64)
        tiny.pipe(t2i_hints=_hints(tiny, ("style",), True), hires_fix=True, **{**_kw(tiny), "height": big, "width": big})
    wide = tiny.text[:, :77, :32].contiguous()
    with pytest.raises(NotImplementedError):                        # a context of another width (SDXL: 2048): refused, not padded
        tiny.pipe(t2i_hints=_hints(tiny, ("style",), True), **{**_kw(tiny), "text_embeddings": wide, "uncond_embeddings": wide})


def test_engine_route_and_nothing_stays_cached(tiny):
    from test_gpu_engine import build_engine, generators, sample_euler_ancestral, wrapper_kwargs
    sets = {"sketch": {"sketch": tiny.sketch, "fuser": tiny.fuser}, "depth": {"depth": tiny.depth, "fuser": tiny.fuser},
            "style": {"style": tiny.style, "clip_model": tiny.clip, "feature_extractor": tiny.fe, "fuser": None}}
    manager = SimpleNamespace(for_type=lambda t, default=None: sets.get(t, default))
    _, _, eng = build_engine(tiny.ucfg, tiny.vcfg, hintset_manager=manager)
    eng.scheduler = sample_euler_ancestral
    seeds, prompt = [7, 8], ["a lighthouse", "a cat"]
    mk = lambda i, kind, w, pr, layer=None: SimpleNamespace(image=tiny.images[i], hint_type=kind, weight=w, priority=pr, clip_layer=layer)
    hint_images = [mk(0, "sketch", 0.8, "balanced"), mk(1, "depth", 0.7, "prompt"), mk(2, "style", 0.9, "hint", "penultimate")]
    args = wrapper_kwargs(prompt=prompt, negative_prompt=None, generator=generators(seeds), width=128, height=128, num_inference_steps=4)
    before, _ = eng(**{**args, "generator": generators(seeds)})
    images, nsfw = eng(**{**args, "hint_images": hint_images})
    assert images.shape == (2, 3, 128, 128) and nsfw == [False, False]
    cond, unc = eng._embed(prompt, None, 2, 1, True, 3)
    img = [i.to(DEV) for i in tiny.images]
    direct = GyrePipeline(eng.unet, eng.vae, None, device=eng.execution_device)(
        generators=generators(seeds), text_embeddings=cond, uncond_embeddings=unc, height=128, width=128, num_inference_steps=4,
        sampler="euler_a",
        t2i_hints=[CoAdapterHint(tiny.sketch, img[0], tiny.fuser, weight=0.8), CoAdapterHint(tiny.depth, img[1], tiny.fuser, weight=0.7, soft_injection=True),
                   StyleHint(tiny.style, img[2], tiny.clip, tiny.fe, weight=0.9, soft_injection=False, cfg_only=True, clip_layer="penultimate")])
    assert torch.equal(images, direct.float().cpu())
    assert not torch.equal(images, before)
    # the next request without hints: what a fresh engine gives, and what this engine gave before the hinted request
    after, _ = eng(**{**args, "generator": generators(seeds)})
    _, _, fresh = build_engine(tiny.ucfg, tiny.vcfg)
    fresh.scheduler = sample_euler_ancestral
    clean, _ = fresh(**{**args, "generator": generators(seeds)})
    assert torch.equal(after, before) and torch.equal(after, clean)
    with pytest.raises(ValueError):                                 # a co-adapter hintset without its fuser
        eng.hintset_manager = SimpleNamespace(for_type=lambda t, default=None: {"sketch": tiny.sketch})
        eng(**{**args, "hint_images": hint_images[:1]})
    with pytest.raises(ValueError):                                 # a style hintset without its CLIP model
        eng.hintset_manager = SimpleNamespace(for_type=lambda t, default=None: {"style": tiny.style})
        eng(**{**args, "hint_images": hint_images[2:]})
