"""Host self-tests of tests/t2i_seq_ref.py (no GPU): the fp32 emulation of every kernel of kernels_seq.hip meets its element-wise bound,
every seeded mistake fails it, the float64 attention equals torch's own nn.MultiheadAttention arithmetic, and the C ABI names are
declared."""
import os

import pytest
import torch
import torch.nn.functional as F

import t2i_seq_ref as R
from gyre_amd import _lib

SDTS = [torch.bfloat16, torch.float16]
SIDS = ["bf16", "f16"]
# a case on which each seeded attention mistake changes the result: padding keys need L off the 32-key tile, the row order N, L > 1,
# the neighbouring head more than one head
MISTAKE_CASES = {"scale_dropped": (1, 2, 12, 96), "q_against_next_head": (1, 2, 12, 96), "k_v_swapped": (2, 1, 63, 64),
                 "padded_keys_in_softmax": (1, 1, 65, 128), "n_l_swapped": (2, 2, 4, 32)}


def _worst(got, v, bd):
    return float(((got.double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=["-".join(map(str, c)) for c in R.ATTN_CASES])
def test_attention_emulation_meets_the_bound(case, sdt):
    c = R.attn_case(sdt, *case)
    worst, rest = R.verdict(c, R.emulate(c))
    print(f"[t2i_seq] emulated seq_attn {sdt} {case}: worst ratio {worst:.3f}")
    assert rest and worst <= 1.0


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
@pytest.mark.parametrize("mistake", R.MISTAKES["attn"])
def test_every_seeded_attention_mistake_fails_the_bound(mistake, sdt):
    assert set(MISTAKE_CASES) == set(R.MISTAKES["attn"])
    c = R.attn_case(sdt, *MISTAKE_CASES[mistake])
    worst, _ = R.verdict(c, R.emulate(c, mistake))
    print(f"[t2i_seq] {mistake} {sdt}: worst ratio {worst:.1f}")
    assert worst > 1.0


@pytest.mark.parametrize("case", [(2, 2, 4, 32), (3, 2, 12, 96), (2, 1, 65, 128)])
def test_value64_is_multi_head_attention_on_the_packed_projection(case):
    """torch's F.multi_head_attention_forward on [L, N, E] with identity projections: the packed columns and the sample-major rows of
    the call are the reference's q, k, v (nn.MultiheadAttention inside ResidualAttentionBlock, adapter.py:155-165)"""
    N, nh, L, D = case
    c = R.attn_case(torch.float16, *case)
    W = nh * D
    x = c["qkv"][:N * L, :3 * W].double().view(N, L, 3 * W).transpose(0, 1)                       # [L, N, 3 W]
    q, k, v = x[..., :W], x[..., W:2 * W], x[..., 2 * W:]
    eye = torch.eye(W, dtype=torch.float64)
    want, _ = F.multi_head_attention_forward(q, k, v, W, nh, None, None, None, None, False, 0.0, eye, None, need_weights=False,
                                             use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye)
    got, _ = R.value64(c)
    # (value64 scales by the fp32 constant the kernel uses: relative 2^-24 of a logit)
    assert torch.allclose(got.view(N, L, W).transpose(0, 1), want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
def test_quick_gelu_emulation_and_its_mistake(sdt):
    x = torch.cat([R.quick_gelu_points(sdt), torch.randn(4096, generator=torch.Generator().manual_seed(3)).mul(3).to(sdt)])
    v, bd = R.quick_gelu_ref(x)
    assert _worst(R.quick_gelu_emulate(x), v, bd) <= 1.0
    assert _worst(R.quick_gelu_emulate(x, "erf_gelu"), v, bd) > 1.0
    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 65536.0


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=["-".join(map(str, c)) for c in R.POOL_CASES])
def test_pool_emulation_and_its_mistake(case, sdt):
    x = R.pool_case(sdt, *case)
    v, bd = R.pool_ref(x)
    assert _worst(R.pool_emulate(x), v, bd) <= 1.0
    # (8 x 8 fills the 64 lanes exactly: there the padded count is the pixel count and the seeded mistake is no mistake)
    assert (_worst(R.pool_emulate(x, "padded_pixel_count"), v, bd) > 1.0) == bool(case[2] * case[3] % 64)
    want = F.silu(x.double().mean((2, 3)))                                         # adapter.py:299-300: mean, then the mapping's SiLU
    assert torch.allclose(v, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
def test_gain_expression_and_its_mistake(sdt):
    x, out = R.pool_case(sdt, 2, 32, 3, 5), R.pool_case(sdt, 2, 32, 3, 5, seed=1)
    alpha = torch.randn((2, 32), generator=torch.Generator().manual_seed(5)) * 0.5
    want = x.double() * (alpha.double()[:, :, None, None] + 1)                     # adapter.py:331-333
    got = R.gain_expr(x, alpha)
    u = R.U[sdt]
    assert bool(((got.double() - want).abs() <= 1.01 * u * want.abs() + R.FL[sdt]).all())
    assert not bool(((R.gain_expr(x, alpha, mistake="alpha_without_one").double() - want).abs() <= 1.01 * u * want.abs() + R.FL[sdt]).all())
    acc = R.gain_expr(x, alpha, out=out)                                           # adapter.py:337: the sum over co-adapters of a type
    assert bool(((acc.double() - (out.double() + want)).abs() <= 1.01 * u * (out.double() + want).abs() + 2 * R.E * want.abs() + R.FL[sdt]).all())
    assert torch.equal(R.bits(R.gain_expr(x, torch.zeros((2, 32)))), R.bits(x))    # zero_module's initial state: the input, bit for bit


def test_max_len_is_what_fits_160_kib():
    for D, L in R.MAX_LEN.items():
        lds = lambda lp: lp * (D + 8) * 2 + D * (lp + 4) * 2
        assert L % 32 == 0 and lds(L) <= 160 * 1024 < lds(L + 32)
    assert R.MAX_LEN[128] >= 257 + 8                                               # the style adapter on CLIP ViT-L/14, 8 tokens


def test_export_names_and_header():
    names = ["gyre_op_seq_attn", "gyre_op_seq_attn_max_len", "gyre_op_quick_gelu", "gyre_op_fuser_pool", "gyre_op_fuser_gain"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gyre_hip.h")).read()
    assert all(f" {n}(" in header for n in names)
    for path in _lib.LIB_PATHS.values():
        if os.path.exists(path):
            blob = open(path, "rb").read()
            assert all(n.encode() + b"\0" in blob for n in names), f"{path} lacks a token-sequence entry"


# ------------------------------------------------------------------------------------------------------------------ the networks
import json

import numpy as np

from gyre_amd import config as gcfg, weights
from gyre_amd import t2i as T

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "t2i_seq_vectors.npz")


def _gold():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 256 * 1024
    return g


def _nets():
    g = _gold()
    scfg, fcfg = gcfg.tiny_t2i_style(), gcfg.tiny_t2i_fuser()
    assert json.loads(str(g["style.cfg"])) == dict(scfg) and json.loads(str(g["fuser.cfg"])) == {**fcfg, "unet_channels": list(fcfg["unet_channels"])}
    ssd = weights.synthetic_state_dict(weights.t2i_style_param_shapes(scfg), int(g["style.seed"]))
    fsd = weights.synthetic_state_dict(weights.t2i_fuser_param_shapes(fcfg), int(g["fuser.seed"]))
    return g, scfg, ssd, fcfg, fsd


def test_restated_networks_equal_what_the_reference_computed():
    """tests/golden/t2i_seq_vectors.npz holds what the reference's own StyleAdapter / CoAdapterFuser computed
    (tests/golden/make_t2i_seq_golden.py); style_net / fuser_net restate them with explicit attention (fp32 ATen on both sides)."""
    g, scfg, ssd, fcfg, fsd = _nets()
    for N, S in R.STYLE_CASES:
        got, want = R.style_net(ssd, scfg, R.style_input(N, S, scfg["width"])), torch.from_numpy(g[f"style.{N}x{S}.out"])
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-5, atol=1e-5), (N, S)
    for name, spec in R.FUSER_CASES.items():
        assert json.loads(str(g[f"fuser.{name}.spec"])) == [list(s) for s in spec]
        maps, seq = R.fuser_net(fsd, fcfg, R.fuser_inputs(spec, fcfg))
        assert (maps is None) == (f"fuser.{name}.map0" not in g.files) and (seq is None) == (f"fuser.{name}.seq" not in g.files)
        for i, m in enumerate(maps or []):
            assert torch.allclose(m, torch.from_numpy(g[f"fuser.{name}.map{i}"]), rtol=1e-5, atol=1e-5), (name, i)
        if seq is not None:
            assert torch.allclose(seq, torch.from_numpy(g[f"fuser.{name}.seq"]), rtol=1e-5, atol=1e-5), name


def test_key_sets_and_shapes_equal_the_reference():
    g = _gold()
    for name, shapes in (("style_default", weights.t2i_style_param_shapes(gcfg.t2i_style_config())),
                         ("fuser_default", weights.t2i_fuser_param_shapes(gcfg.t2i_fuser_config())),
                         ("style", weights.t2i_style_param_shapes(gcfg.tiny_t2i_style())),
                         ("fuser", weights.t2i_fuser_param_shapes(gcfg.tiny_t2i_fuser()))):
        assert list(shapes) == [str(k) for k in g[f"{name}.keys"]], name                    # names AND registration order
        if f"{name}.shapes" in g.files:
            assert [list(v) for v in shapes.values()] == json.loads(str(g[f"{name}.shapes"]))
    assert gcfg.EXTRA_CONDITION == R.EXTRA_CONDITION == dict(sketch=0, keypose=1, seg=2, depth=3, canny=4, style=5, color=6, openpose=7)


@pytest.mark.parametrize("sdt", SDTS, ids=SIDS)
def test_every_seeded_network_mistake_leaves_the_emulation_distance(sdt):
    """the storage emulation stays close to the float64 net; each seeded mistake is at least ten times farther on some output"""
    g, scfg, ssd, fcfg, fsd = _nets()
    x = R.style_input(3, 5, scfg["width"])
    ref = R.style_net(ssd, scfg, x, compute=torch.float64)
    base = R.rel_l2(R.style_net(ssd, scfg, x, store=sdt), ref)
    assert base < 0.05
    for mistake in ("first_rows_instead_of_last",):
        assert R.rel_l2(R.style_net(ssd, scfg, x, store=sdt, mistake=mistake), ref) > 10 * base, mistake
    feats = R.fuser_inputs(R.FUSER_CASES["two_spatial_one_style"], fcfg)
    flat = lambda out: torch.cat([t.reshape(-1).double() for t in out[0]] + [out[1].reshape(-1).double()])
    ref = flat(R.fuser_net(fsd, fcfg, feats, compute=torch.float64))
    base = R.rel_l2(flat(R.fuser_net(fsd, fcfg, feats, store=sdt)), ref)
    assert base < 0.05
    for mistake in ("task_index_off_by_one", "positional_embedding_dropped", "alpha_without_one"):
        assert R.rel_l2(flat(R.fuser_net(fsd, fcfg, feats, store=sdt, mistake=mistake)), ref) > 10 * base, mistake
    assert set(R.NET_MISTAKES) == {"task_index_off_by_one", "positional_embedding_dropped", "first_rows_instead_of_last", "alpha_without_one"}


def test_loader_round_trips_all_four_types_and_loads_strictly(tmp_path):
    cases = {"main": (gcfg.tiny_t2i("main"), weights.t2i_param_shapes, T.GyreHipT2IAdapter),
             "light": (gcfg.tiny_t2i("light"), weights.t2i_param_shapes, T.GyreHipT2IAdapter),
             "style": (gcfg.tiny_t2i_style(), weights.t2i_style_param_shapes, T.GyreHipT2IStyleAdapter),
             "fuser": (gcfg.tiny_t2i_fuser(), weights.t2i_fuser_param_shapes, T.GyreHipT2IFuser)}
    for kind, (cfg, shapes, cls) in cases.items():
        d = tmp_path / kind
        d.mkdir()
        sd = weights.synthetic_state_dict(shapes(cfg), 5)
        torch.save(sd, d / "model.pth")
        kw = {k: v for k, v in cfg.items() if k != "type"}
        m = T.T2iAdapter.from_state_dict(str(d), torch_dtype=torch.float16, type=kind, coadapter="style" if kind == "style" else False, **kw)
        assert type(m) is cls and m._coadapter_type == ("style" if kind == "style" else False) and not m.training
        assert m.dtype == torch.float16 and list(m.state_dict()) == list(sd)
        assert all(torch.equal(v, sd[k].half()) for k, v in m.state_dict().items())
        bad = dict(sd)
        bad.pop(next(iter(bad)))
        with pytest.raises(RuntimeError):
            cls(cfg).load_state_dict(bad)                                                   # strict: a missing key is an error
        with pytest.raises(RuntimeError):
            cls(cfg).load_state_dict({**sd, "extra.weight": torch.zeros(1)})
    with pytest.raises(ValueError):
        T.T2iAdapter.from_state_dict(str(tmp_path / "main"), type="nonsense")
    with pytest.raises(RuntimeError):
        (tmp_path / "empty").mkdir()
        T.T2iAdapter.from_state_dict(str(tmp_path / "empty"), type="style")


def test_pinned_refusals_still_hold_and_new_ones_fail_closed():
    with pytest.raises(NotImplementedError):
        T.GyreHipT2IAdapter.from_state_dict("/nonexistent", type="style")
    with pytest.raises(NotImplementedError):
        T.GyreHipT2IAdapter.from_state_dict("/nonexistent", type="fuser")
    with pytest.raises(NotImplementedError):
        gcfg.t2i_config("style")
    with pytest.raises(NotImplementedError):
        gcfg.t2i_style_config(width=80, num_head=2)                                         # head dim 40 is not built
    with pytest.raises(NotImplementedError):
        gcfg.t2i_fuser_config(unet_channels=(30, 64, 128, 128))
    with pytest.raises(TypeError):
        gcfg.t2i_style_config(depth=3)
    m = T.GyreHipT2IStyleAdapter(gcfg.tiny_t2i_style())
    with pytest.raises(_lib.GyreError):
        m(torch.zeros((1, 4, 64)))                                                          # no CPU fallback


def test_handle_symbols_are_declared():
    names = ["gyre_t2i_seq_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes")]
    names += ["gyre_t2i_style_forward", "gyre_t2i_fuser_forward"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gyre_hip.h")).read()
    assert all(n in _lib.EXPORTED_SYMBOLS and f" {n}(" in header for n in names)
    for path in _lib.LIB_PATHS.values():
        if os.path.exists(path):
            blob = open(path, "rb").read()
            assert all(n.encode() + b"\0" in blob for n in names), f"{path} lacks a gyre_t2i_seq entry"


# ---------------------------------------------------------------------------------------------------------------- the hint layer
from types import SimpleNamespace

from gyre_amd import hints as H


class _FakeHint:
    def __init__(self, fuser, cfg, cotype, kind, T, seed, cfg_only):
        self.cotype, self.cfg_only, self.fuser = cotype, cfg_only, fuser if cotype else None
        self.state = R.hint_states(kind, T, seed, cfg)

    def coadapter_type(self):
        return self.cotype

    def __call__(self):
        return self.state


def test_conditioning_and_context_extension_equal_the_reference_on_every_case():
    """build_t2i_conditioning / extend_style_context against what UNetWithT2I.__init__ / __call__ computed over the same fake hints
    (tests/golden/make_t2i_seq_golden.py), the reference's fuser there and its restatement here"""
    g, _, _, fcfg, fsd = _nets()
    fuser = lambda feats: R.fuser_net(fsd, fcfg, list(feats.items()))
    close = lambda a, key: torch.allclose(a, torch.from_numpy(g[key]), rtol=1e-5, atol=1e-5)
    for name, spec in R.HINT_CASES.items():
        assert json.loads(str(g[f"cond.{name}.spec"])) == [list(h) for h in spec]
        states, style = H.build_t2i_conditioning([_FakeHint(fuser, fcfg, *h) for h in spec])
        assert (states is None) == (f"cond.{name}.g0" not in g.files) and (style is None) == (f"cond.{name}.style" not in g.files), name
        if states is not None:
            assert all(close(t, f"cond.{name}.{side}{i}") for side in ("u", "g", "f") for i, t in enumerate(states[side])), name
        if style is not None:
            assert close(style, f"cond.{name}.style"), name
            for side in ("u", "g", "f"):
                ctx = R.hint_context(style.shape[0] * (2 if side == "f" else 1), fcfg["width"])
                got = H.extend_style_context(ctx, style, side)
                assert got.shape[1] == ctx.shape[1] + style.shape[1] and close(got, f"cond.{name}.ctx_{side}"), (name, side)
    assert H.build_t2i_conditioning([]) == (None, None)
    ctx = R.hint_context(2, 64)
    assert H.extend_style_context(ctx, None, "f") is ctx
    mixed = g["cond.mixed_cfg_only.u0"], g["cond.mixed_cfg_only.g0"]                        # the two-pass branch really ran: the sides differ
    assert not np.allclose(mixed[0], mixed[1])


def test_style_hint_and_coadapter_hint():
    hidden = [torch.randn((1, 5, 64), generator=torch.Generator().manual_seed(80 + i)) for i in range(5)]
    seen = {}

    def vision_model(image, output_hidden_states=False, return_dict=True):
        seen["image"], seen["all"] = image, output_hidden_states
        return SimpleNamespace(last_hidden_state=hidden[-1] + 1, hidden_states=hidden if output_hidden_states else None)

    clip = SimpleNamespace(vision_model=vision_model)
    fe = SimpleNamespace(image_mean=[0.5, 0.4, 0.3], image_std=[0.2, 0.3, 0.4], size={"shortest_edge": 8})
    calls = []

    class Model:
        dtype, _coadapter_type = torch.float32, False

        def __call__(self, x):
            calls.append(x)
            return x[:, -3:] * 2

    image = torch.rand((1, 4, 12, 20), generator=torch.Generator().manual_seed(1))
    for layer, want in (("final", hidden[-1] + 1), (None, hidden[-1] + 1), ("penultimate", hidden[-2]), (2, hidden[-2]), (3, hidden[-3]), (-3, hidden[-3])):
        with pytest.warns(UserWarning):
            h = H.StyleHint(Model(), image, clip, fe, mask=torch.ones(1, 1, 12, 20), soft_injection=True, weight=0.5, clip_layer=layer)
        got = h()
        assert torch.equal(calls[-1], want) and torch.equal(got, want[:, -3:] * 2 * 0.5)
        assert seen["all"] == (H.normalise_clip_layer(layer, "final") != "final") and tuple(seen["image"].shape) == (1, 3, 8, 8)
        assert not h.soft_injection and not h.coadapter_type()
    # the preprocessing: cover-rescale to the extractor's size, then (x - mean) / std per channel
    from gyre_amd.images import rescale
    mean, std = torch.tensor(fe.image_mean).view(1, 3, 1, 1), torch.tensor(fe.image_std).view(1, 3, 1, 1)
    assert torch.allclose(seen["image"], (rescale(image[:, :3], 8, 8, "cover") - mean) / std)
    with pytest.raises(ValueError):
        H.StyleHint(Model(), image, None, fe)
    with pytest.raises(ValueError):
        H.StyleHint(Model(), image, clip, None)
    co = Model()
    co._coadapter_type = "style"
    with pytest.raises(ValueError):
        H.StyleHint(co, image, clip, fe)                                                    # a co-adapter without its fuser
    assert H.StyleHint(co, image, clip, fe, fuser=object()).coadapter_type() == "style"

    class Adapter:
        config = gcfg.tiny_t2i("main")
        _coadapter_type = "sketch"

        def __call__(self, x):
            return [x[:, :, ::2 ** i, ::2 ** i] for i in range(4)]

    a = Adapter()
    with pytest.raises(ValueError):
        H.CoAdapterHint(a, image[:, :3], None)
    plain = Adapter()
    plain._coadapter_type = False
    with pytest.raises(ValueError):
        H.CoAdapterHint(plain, image[:, :3], object())
    with pytest.raises(NotImplementedError):
        H.T2IHint(a, image[:, :3])                                                          # the pinned refusal, unchanged
    with pytest.raises(NotImplementedError):
        H.CoAdapterHint(a, image[:, :3], object(), mask=torch.zeros(1, 1, 12, 20))          # masked co-adapter hints fail closed
    h = H.CoAdapterHint(a, image[:, :3], "fuser", weight=0.5, soft_injection=True)
    assert h.coadapter_type() == "sketch" and h.fuser == "fuser" and a._coadapter_type == "sketch"
    lw = torch.logspace(-0.25, 0, 4)
    assert all(torch.equal(s, t * 0.5 * w) for s, t, w in zip(h(), a(image[:, :3]), lw))


def test_style_and_coadapter_hints_fail_closed_in_the_pipeline():
    """what the request route still refuses, before any model runs: CLIP guidance, grafted inpaint, hires fix, a context of another
    width than the style tokens (SDXL's 2048), and a style hint that is no tensor of the request's batch"""
    from gyre_amd.pipeline import GyrePipeline
    from test_host_pipeline import OracleVAE
    ucfg, vcfg = gcfg.tiny_unet(), gcfg.tiny_vae()
    unet = SimpleNamespace(config=ucfg)
    vae = OracleVAE(weights.synthetic_state_dict(weights.vae_param_shapes(vcfg)), vcfg)

    class Style(H.StyleHint):
        def __init__(self, width=ucfg.cross_attention_dim, cotype=False):
            self.cfg_only, self.width, self.cotype, self.fuser = False, width, cotype, None

        def coadapter_type(self):
            return self.cotype

        def __call__(self):
            return torch.zeros((1, 3, self.width))

    text = torch.zeros((1, 77, ucfg.cross_attention_dim))
    kw = dict(seeds=[1], text_embeddings=text, uncond_embeddings=text, height=128, width=128, num_inference_steps=2, sampler="euler")
    with pytest.raises(NotImplementedError, match="CLIP guidance"):
        GyrePipeline(unet, vae, device="cpu", clip_model=object(), feature_extractor=object())(t2i_hints=[Style()], clip_guidance_scale=1.0, **kw)
    with pytest.raises(NotImplementedError, match="grafted inpaint"):
        GyrePipeline(unet, vae, device="cpu", inpaint_unet=SimpleNamespace(config=ucfg), grafted_inpaint=True)(
            t2i_hints=[Style()], image=torch.zeros(1, 3, 128, 128), mask_image=torch.zeros(1, 1, 128, 128), **kw)
    big = 2 * 8 * getattr(ucfg, "sample_size", 64)
    with pytest.raises(NotImplementedError, match="hires fix"):
        GyrePipeline(unet, vae, device="cpu")(t2i_hints=[Style()], hires_fix=True, **{**kw, "height": big, "width": big})
    with pytest.raises(NotImplementedError, match="style tokens of width"):
        GyrePipeline(unet, vae, device="cpu")(t2i_hints=[Style(width=2048)], **kw)
    with pytest.raises(ValueError, match="fuser is missing"):
        GyrePipeline(unet, vae, device="cpu")(t2i_hints=[Style(cotype="style")], **kw)


def test_style_hint_equals_the_reference_style_call_at_three_clip_layers():
    """what UnifiedPipelineHint_T2i.style_call returned over the same fake vision model and the reference's own StyleAdapter
    (tests/golden/make_t2i_seq_golden.py): the layer choice, whether all hidden states are asked for, the model call, x weight.  The
    image the vision model saw is compared as well; its rescale and Normalize are restatements on both sides and stay unpinned."""
    g, scfg, ssd, _, _ = _nets()

    class Model:
        dtype, _coadapter_type = torch.float32, False

        def __call__(self, x):
            return R.style_net(ssd, scfg, x)

    for layer in R.STYLE_LAYERS:
        vision = R.FakeVision(scfg["width"])
        h = H.StyleHint(Model(), R.style_hint_image(), SimpleNamespace(vision_model=vision), SimpleNamespace(**R.STYLE_EXTRACTOR),
                        weight=R.STYLE_HINT_WEIGHT, clip_layer=layer)
        got = h()
        assert torch.allclose(got, torch.from_numpy(g[f"stylehint.{layer}.out"]), rtol=1e-5, atol=1e-5), layer
        assert vision.asked_all == bool(g[f"stylehint.{layer}.all_layers"]) == (layer != "final")
        assert torch.allclose(vision.seen, torch.from_numpy(g[f"stylehint.{layer}.seen"]), rtol=1e-6, atol=1e-6)
    outs = [g[f"stylehint.{layer}.out"] for layer in R.STYLE_LAYERS]
    assert not np.allclose(outs[0], outs[1]) and not np.allclose(outs[1], outs[2])              # three different layers were read


def test_stored_emulation_figures_are_what_the_emulation_gives():
    """tests/test_gpu_t2i_seq_model.EMULATION sets the GPU gates (twice these figures).  Recomputed here on the CPU: within a factor of
    1.5 either way of the stored value (another torch build may add in another order and move a rounding), so neither a looser
    emulation nor a stale table goes unnoticed."""
    import test_gpu_t2i_seq_model as G
    seen = set()

    def hold(label, emu, ref):
        ma, rl = G.emulation_distance(emu, ref)
        sma, srl = G.EMULATION[label]
        print(f"[t2i_seq] emulation {label}: max-abs {ma:.3e} (stored {sma:.3e}), rel-L2 {rl:.3e} (stored {srl:.3e})")
        assert sma / 1.5 <= ma <= 1.5 * sma and srl / 1.5 <= rl <= 1.5 * srl, label
        seen.add(label)

    for sdt in SDTS:
        for size, N, S in G.STYLE_SHAPES:
            cfg, sd = G.state_dict("style", size, sdt)
            x = R.style_input(N, S, cfg["width"])
            hold(f"style {size} N={N} S={S} {sdt}", R.style_net(sd, cfg, x, store=sdt), R.style_net(sd, cfg, x, compute=torch.float64))
        cases = [("tiny", name, R.fuser_inputs(spec, gcfg.tiny_t2i_fuser())) for name, spec in R.FUSER_CASES.items()]
        cases.append(("default", "default", R.fuser_inputs(G.DEFAULT_FUSER_SPEC, gcfg.t2i_fuser_config(), N=1, hw=G.DEFAULT_HW)))
        for size, name, feats in cases:
            cfg, sd = G.state_dict("fuser", size, sdt)
            st = G.stored(feats, sdt)
            ref, emu = R.fuser_net(sd, cfg, st, compute=torch.float64), R.fuser_net(sd, cfg, st, store=sdt)
            for i, (e, r) in enumerate(zip(emu[0] or [], ref[0] or [])):
                hold(f"fuser {name} {sdt} maps[{i}]", e, r)
            if emu[1] is not None:
                hold(f"fuser {name} {sdt} tokens[0]", emu[1], ref[1])
    assert seen == set(G.EMULATION)
