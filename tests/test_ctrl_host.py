"""ControlNet hint conditioning, host side (no GPU): the state-dict surface of the shell against the reference's constructor (parsed,
never imported or copied), the fp32 restatement tests/ctrl_ref.py against the oracle's own UNet walk, the error models of the two
kernels against seeded mistakes, the hint arithmetic (scales, cfg_only placement, buffer reuse), the engine's routing and every
combination that fails closed."""
import ast
import os
from types import SimpleNamespace

import pytest
import torch

import ctrl_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.engine import GyreUnifiedPipeline
from gyre_amd.hints import ControlNetHint
from gyre_amd.pipeline import GyrePipeline
from gyre_amd.schedulers import UNetWithControlnet
from oracle import models_ref as M

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


# ---- shell ---------------------------------------------------------------------------------------------------------------------------
def test_sd15_state_dict_names_and_shapes():
    cfg = gcfg.sd15_controlnet()
    shapes = weights.controlnet_param_shapes(cfg)
    unet = weights.unet_param_shapes(gcfg.sd15_unet())
    own = [k for k in shapes if k.startswith("controlnet_")]
    shared = [k for k in shapes if not k.startswith("controlnet_")]
    assert shared and all(shapes[k] == unet[k] for k in shared)                      # the UNet shell's own entries, same shapes
    assert sorted(shared) == sorted(k for k in unet if k.split(".")[0] in ("conv_in", "time_embedding", "down_blocks", "mid_block"))
    emb = sorted({k.rsplit(".", 1)[0] for k in own if k.startswith("controlnet_cond_embedding.")})
    assert len(emb) == 8 and shapes["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert [shapes[f"controlnet_cond_embedding.blocks.{i}.weight"][:2] for i in range(6)] == [(16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96)]
    assert shapes["controlnet_cond_embedding.conv_out.weight"] == (320, 256, 3, 3)
    down = [k for k in own if k.startswith("controlnet_down_blocks.") and k.endswith(".weight")]
    assert len(down) == 12 == cfg.n_residuals
    assert [shapes[f"controlnet_down_blocks.{k}.weight"] for k in range(12)] == [(c, c, 1, 1) for c in (320,) * 4 + (640,) * 3 + (1280,) * 5]
    assert shapes["controlnet_mid_block.weight"] == (1280, 1280, 1, 1) and shapes["controlnet_mid_block.bias"] == (1280,)
    tiny = GyreHipControlNet(gcfg.tiny_controlnet())
    tshapes = weights.controlnet_param_shapes(tiny.config)
    assert {k: tuple(v.shape) for k, v in tiny.state_dict().items()} == dict(tshapes)
    tiny.load_state_dict(weights.synthetic_state_dict(tshapes, 3))                  # strict: the diffusers key space loads as it is
    assert tiny.config.get("global_pool_conditions", False) is False and tiny.config.get("nothing", 5) == 5
    assert len(tiny.residual_shapes(16, 24)) == 13 and tiny.residual_shapes(9, 8)[-1] == (128, 2, 1)
    with pytest.raises(NotImplementedError):
        GyreHipControlNet._config_from_json({"class_embed_type": "timestep"})
    with pytest.raises(NotImplementedError):
        GyreHipControlNet._config_from_json({"num_class_embeds": 10})
    cfg2 = GyreHipControlNet._config_from_json({"controlnet_conditioning_channel_order": "bgr", "global_pool_conditions": True})
    assert cfg2.controlnet_conditioning_channel_order == "bgr" and cfg2.get("global_pool_conditions", False) is True
    assert cfg2.block_out_channels == (320, 640, 1280, 1280) and cfg2.conditioning_embedding_out_channels == (16, 32, 96, 256)


def _ctor(path, cls):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == cls:
            return next(fn for fn in node.body if isinstance(fn, ast.FunctionDef) and fn.name == "__init__")
    raise AssertionError(f"{cls}.__init__ not found in {path}")


def _defaults(fn):
    args, vals, out = fn.args.args[1:], fn.args.defaults, {}
    for a, d in zip(args[len(args) - len(vals):], vals):
        try:
            out[a.arg] = ast.literal_eval(d)
        except ValueError:
            out[a.arg] = ast.unparse(d)
    return out


@needs_reference
def test_constructor_defaults_and_module_counts_match_the_reference():
    path = "gyre/pipeline/controlnet/models.py"
    model, emb = _ctor(path, "ControlNetModel"), _ctor(path, "ControlNetConditioningEmbedding")
    d, cfg = _defaults(model), gcfg.sd15_controlnet()
    assert tuple(d["block_out_channels"]) == cfg.block_out_channels and d["layers_per_block"] == cfg.layers_per_block
    assert d["in_channels"] == cfg.in_channels and d["cross_attention_dim"] in (cfg.cross_attention_dim, 1280)
    assert tuple(d["conditioning_embedding_out_channels"]) == cfg.conditioning_embedding_out_channels
    assert d["flip_sin_to_cos"] == cfg.flip_sin_to_cos and d["freq_shift"] == cfg.freq_shift and d["norm_num_groups"] == cfg.norm_num_groups
    assert d["controlnet_conditioning_channel_order"] == cfg.controlnet_conditioning_channel_order
    assert tuple("CrossAttn" in t for t in d["down_block_types"]) == cfg.attn_levels
    e = _defaults(emb)
    assert e["conditioning_channels"] == cfg.conditioning_channels and tuple(e["block_out_channels"]) == (16, 32, 96, 256)
    src = ast.unparse(emb)
    assert src.count("self.blocks.append") == 2 and "stride=2" in src and "range(len(block_out_channels) - 1)" in src
    msrc = ast.unparse(model)
    # one zero convolution for conv_in, one per layer, one per downsampler of a non-final block, one for the mid block
    assert msrc.count("self.controlnet_down_blocks.append") == 3 and "self.controlnet_mid_block" in msrc
    assert "for _ in range(layers_per_block)" in msrc and "if not is_final_block" in msrc


# ---- restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = gcfg.tiny_controlnet()
    sd = weights.synthetic_state_dict(weights.controlnet_param_shapes(cfg), 1)
    g = torch.Generator().manual_seed(2)
    x, ctx = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 5, cfg.cross_attention_dim, generator=g)
    return SimpleNamespace(cfg=cfg, sd=sd, x=x, ctx=ctx, img=torch.rand(2, 3, 128, 128, generator=g), t=torch.tensor([981, 17]))


def test_zeroed_zero_convolutions_give_zero_residuals(tiny):
    sd = {k: (torch.zeros_like(v) if k.startswith(("controlnet_down_blocks", "controlnet_mid_block")) else v) for k, v in tiny.sd.items()}
    out = R.ctrl_forward(sd, tiny.cfg, tiny.x, tiny.t, tiny.ctx, tiny.img)
    assert len(out) == 13 and all(bool((o == 0).all()) for o in out)
    assert all(float(o.norm()) > 0 for o in R.ctrl_forward(tiny.sd, tiny.cfg, tiny.x, tiny.t, tiny.ctx, tiny.img))


def test_walk_collects_what_the_oracle_unet_exposes(tiny):
    """with conv_out of the conditioning embedding zeroed the control model's encoder IS the UNet's: same weights, same tensors"""
    ucfg = gcfg.tiny_unet()
    usd = weights.synthetic_state_dict(weights.unet_param_shapes(ucfg))
    sd = dict(tiny.sd)
    sd.update({k: v for k, v in usd.items() if k in sd})
    for k in ("controlnet_cond_embedding.conv_out.weight", "controlnet_cond_embedding.conv_out.bias"):
        sd[k] = torch.zeros_like(sd[k])
    taps, utaps = {}, {}
    R.ctrl_forward(sd, tiny.cfg, tiny.x, tiny.t, tiny.ctx, tiny.img, taps=taps)
    M.unet_forward(usd, ucfg, tiny.x, tiny.t, tiny.ctx, taps=utaps)
    skips = taps["skips"]
    assert len(skips) == 12
    # the oracle taps the last tensor of every level: skip 3, 6, 9 (downsampler outputs) and 11
    for lvl, k in enumerate((3, 6, 9, 11)):
        assert torch.equal(skips[k], utaps[f"down{lvl}"])
    assert torch.equal(taps["mid"], utaps["mid"])


# ---- error models --------------------------------------------------------------------------------------------------------------------
EMIT_SHAPES = [(2, 32, 32, 6), (3, 20, 24, 35), (1, 320, 320, 64), (2, 1280, 1280, 1)]
MISTAKES = {False: ("scale_dropped", "wrong_offset", "lower_not_zeroed"),
            True: ("scale_dropped", "rounded_before_accumulate", "wrong_offset", "lower_clobbered")}


def _emit_ratio(f, C_, scale, acc, old, b0, odt, mistake=None):
    got = R.emit_host(f, C_, scale, acc, old, b0, mistake)
    exact, mag = R.emit_exact(f, C_, scale, acc, old, b0)
    return float(((got.double() - exact).abs() / R.emit_bound(exact, mag, odt, acc).clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", EMIT_SHAPES)
def test_emit_error_model_accepts_the_emulation_and_catches_seeded_mistakes(sdt, shape):
    B, C_, Cpad, HW = shape
    g = torch.Generator().manual_seed(HW * 7 + C_)
    f = torch.randn((B, HW, Cpad), generator=g).to(sdt)
    soft = 0.8 * float(torch.logspace(-1, 0, 13)[3])
    for odt in (torch.float32, sdt):
        for acc in (False, True):
            old = torch.randn((B + 2, C_, HW), generator=g).to(odt) if acc else torch.full((2 * B, C_, HW), float("nan"), dtype=odt)
            b0 = 1 if acc else B
            for scale in (-1.7, soft):
                assert _emit_ratio(f, C_, scale, acc, old, b0, odt) <= 1.0
                for m in MISTAKES[acc]:
                    assert _emit_ratio(f, C_, scale, acc, old, b0, odt, m) > 1.0, (m, odt, acc, scale)


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [8, 8 * 1031])
def test_silu_error_model_accepts_the_emulation(sdt, n):
    x = R.silu_inputs(n, sdt, seed=n)
    ratio, nan_kept, finite = R.silu_check(x, R.silu_host(x))
    assert ratio <= 1.0 and nan_kept and finite
    bad = (x.float() * torch.sigmoid(x.float())).to(sdt).float()
    assert R.silu_check(x, (bad * 1.02).to(sdt))[0] > 1.0                          # 2 % off is far outside
    assert not R.silu_check(x, torch.nan_to_num(R.silu_host(x), nan=0.0))[1]        # a swallowed NaN is seen


# ---- hint arithmetic -----------------------------------------------------------------------------------------------------------------
class StubControlNet:
    """records the calls ControlNetHint / UNetWithControlnet make; the residual of output k is the constant k + 1"""

    def __init__(self, global_pool=False):
        self.config = gcfg.tiny_controlnet(global_pool_conditions=global_pool)
        self._bound, self.binds, self.calls = None, [], []

    def bind(self, image, ctx):
        self._bound = (image, ctx)
        self.binds.append((tuple(image.shape), tuple(ctx.shape)))

    def new_outputs(self, B, H, W, device, dtype=None):
        return [torch.full((B, ch, h, w), float("nan")) for ch, h, w in GyreHipControlNet.residual_shapes(self, H, W)]

    def __call__(self, x, t, *, scales, out, accumulate=False, out_batch=None, out_offset=0):
        B = x.shape[0]
        self.calls.append(dict(B=B, t=t, accumulate=accumulate, out_batch=out_batch, out_offset=out_offset, ctx=self._bound[1]))
        for k, (o, s) in enumerate(zip(out, scales)):
            if not accumulate:
                o.zero_()
                o[out_offset:out_offset + B] = (k + 1) * s
            else:
                o[out_offset:out_offset + B] += (k + 1) * s
        return out


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("cfg_only", [False, True])
@pytest.mark.parametrize("global_pool", [False, True])
def test_hint_scales_and_flags(soft, cfg_only, global_pool):
    hint = ControlNetHint(StubControlNet(global_pool), torch.rand(3, 16, 16), weight=0.8, soft_injection=soft, cfg_only=cfg_only)
    assert hint.image.shape == (1, 3, 16, 16)
    if global_pool:
        assert hint.cfg_only is True and hint.soft_injection is False
    else:
        assert hint.cfg_only is cfg_only and hint.soft_injection is soft
    sc = hint.scales()
    assert len(sc) == 13 and sc == R.hint_scales(0.8, hint.soft_injection, 13)
    if hint.soft_injection:
        assert sc[0] == pytest.approx(0.08) and sc[-1] == pytest.approx(0.8) and sc[-1] == sc[12] and sorted(sc) == sc
    else:
        assert sc == [0.8] * 13


def test_masked_hints_fail_closed():
    with pytest.raises(NotImplementedError, match="mask"):
        ControlNetHint(StubControlNet(), torch.rand(1, 3, 16, 16), mask=torch.rand(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="mask"):
        ControlNetHint(StubControlNet(), torch.rand(1, 4, 16, 16))                # an alpha plane is a mask
    assert ControlNetHint(StubControlNet(), torch.cat([torch.rand(1, 3, 8, 8), torch.ones(1, 1, 8, 8)], 1)).image.shape[1] == 3
    assert ControlNetHint(StubControlNet(True), torch.rand(1, 4, 8, 8), mask=torch.rand(1, 1, 8, 8)).image.shape[1] == 3


class StubUNet:
    config = gcfg.tiny_unet()

    def __init__(self):
        self.calls = []

    def __call__(self, latents, t, **kw):
        self.calls.append({k: ([r.clone() for r in v] if isinstance(v, list) else v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()})
        return SimpleNamespace(sample=latents)


def test_unet_with_controlnet_sums_two_hints_in_one_set_of_buffers():
    a, b = StubControlNet(), StubControlNet()
    img = torch.rand(1, 3, 64, 64)
    h1 = ControlNetHint(a, img, weight=0.5)                                        # full
    h2 = ControlNetHint(b, img, weight=2.0, soft_injection=True, cfg_only=True)    # guided half only
    lat, ctx, t = torch.randn(4, 4, 8, 8), torch.randn(4, 5, 64), torch.tensor([9, 9, 9, 9])
    unet = StubUNet()
    f = UNetWithControlnet(unet, [h1, h2], "f")
    for _ in range(2):                                                             # two steps: one bind each, the same buffers
        f(lat, t, encoder_hidden_states=ctx)
    assert a.binds == [((1, 3, 64, 64), (4, 5, 64))] and b.binds == [((1, 3, 64, 64), (2, 5, 64))]
    assert torch.equal(b.calls[0]["ctx"], ctx.chunk(2)[-1])
    assert [c["B"] for c in a.calls] == [4, 4] and [(c["B"], c["out_batch"], c["out_offset"], c["accumulate"]) for c in b.calls] == [(2, 4, 2, True)] * 2
    assert [c["accumulate"] for c in a.calls] == [False, False] and b.calls[0]["t"].shape == (2,)
    sc1, sc2 = R.hint_scales(0.5, False, 13), R.hint_scales(2.0, True, 13)
    for call in unet.calls:
        res = call["down_block_additional_residuals"] + [call["mid_block_additional_residual"]]
        assert len(res) == 13
        for k, r in enumerate(res):
            want = R.place([torch.full_like(r[:2], (k + 1) * sc2[k])], "f", True)[0] + (k + 1) * sc1[k]
            torch.testing.assert_close(r, want, rtol=1e-6, atol=0)
    bufs = [o.data_ptr() for o in f._bufs[1]]
    f(lat, t, encoder_hidden_states=ctx)
    assert bufs == [o.data_ptr() for o in f._bufs[1]]                              # allocated once, reused by every step
    # the unconditional side: a cfg_only hint contributes nothing and is never run
    u = UNetWithControlnet(StubUNet(), [h2], "u")
    n = len(b.calls)
    u(lat[:2], 9, encoder_hidden_states=ctx[:2])
    assert len(b.calls) == n and "down_block_additional_residuals" not in u.unet.calls[0]
    # the guided side of a sequential run: the model is bound again for the other context, and runs in full
    g = UNetWithControlnet(StubUNet(), [h2], "g")
    g(lat[:2], 9, encoder_hidden_states=ctx[2:])
    assert len(b.binds) == 2 and b.calls[-1]["out_offset"] == 0 and b.calls[-1]["accumulate"] is False
    assert R.place([torch.ones(2, 1)], "u", True) is None and R.place([torch.ones(2, 1)], "u", False)[0].shape == (2, 1)
    with pytest.raises(NotImplementedError, match="9-channel"):
        h1.run("g", torch.randn(1, 9, 8, 8), 3, ctx[:1], None, False)


# ---- engine routing and refusals -----------------------------------------------------------------------------------------------------
def test_library_exports_the_controlnet_symbols():
    names = ["gyre_ctrl_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "bind_workspace_bytes",
                                        "bind", "workspace_bytes", "forward")] + ["gyre_op_silu", "gyre_op_ctrl_emit"]
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS
        for L in _lib.all_libs():
            assert hasattr(L, n)
    assert all(L.gyre_abi_version() == 1 for L in _lib.all_libs())


def _engine(manager, **kw):
    unet = torch.nn.Linear(1, 1)                 # (execution_device reads a parameter; nothing runs)
    unet.config = gcfg.tiny_unet()
    return GyreUnifiedPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler="euler", hintset_manager=manager, **kw)


def _hint(hint_type="canny", **kw):
    return SimpleNamespace(**{"image": torch.rand(1, 3, 128, 128), "hint_type": hint_type, "weight": None, "priority": "balanced",
                              "clip_layer": None, **kw})


def test_engine_routes_a_controlnet_handler_to_a_controlnet_hint():
    ctrl = GyreHipControlNet(gcfg.tiny_controlnet())
    table = {"canny": {"controlnet": ctrl}, "other": {"model": torch.nn.Linear(1, 1)}}
    manager = SimpleNamespace(for_type=lambda t, default=None: table.get(t, default))
    eng = _engine(manager)
    hints = eng._hints([_hint(weight=0.8, priority="prompt"), _hint(priority="hint"), _hint()], None)
    assert all(isinstance(h, ControlNetHint) and h.model is ctrl for h in hints)
    assert [(h.weight, h.soft_injection, h.cfg_only) for h in hints] == [(0.8, True, False), (1.0, True, True), (1.0, False, False)]
    with pytest.raises(NotImplementedError):                      # a foreign handler keeps raising
        eng._hints([_hint("other")], None)
    with pytest.raises(NotImplementedError, match="mask"):
        eng._hints([_hint()], torch.zeros(1, 1, 128, 128))
    eng._shard_devices = [torch.device("cpu"), torch.device("cpu")]
    with pytest.raises(NotImplementedError, match="shard_devices"):
        eng(prompt="x", hint_images=[_hint()])


class _NoDeviceUNet:
    def __init__(self, in_channels=4):
        self.config = gcfg.tiny_unet(in_channels)

    def __call__(self, *a, **k):
        raise AssertionError("no UNet call may happen before the refusal")


def test_unsupported_combinations_fail_closed_without_a_gpu():
    hint = ControlNetHint(StubControlNet(), torch.rand(1, 3, 128, 128))
    text = torch.zeros(1, 77, 64)
    kw = dict(seeds=[1], text_embeddings=text, uncond_embeddings=text, height=128, width=128, num_inference_steps=2,
              sampler="euler", controlnet_hints=[hint])
    vae = SimpleNamespace(config=gcfg.tiny_vae())
    pipe = GyrePipeline(_NoDeviceUNet(), vae, device="cpu")
    with pytest.raises(NotImplementedError, match="hires"):
        pipe(**{**kw, "height": 256, "width": 256})
    with pytest.raises(NotImplementedError, match="mask"):
        pipe(**kw, image=torch.zeros(1, 3, 128, 128), mask_image=torch.zeros(1, 1, 128, 128))
    with pytest.raises(NotImplementedError, match="9-channel"):
        GyrePipeline(_NoDeviceUNet(9), vae, device="cpu")(**kw)
    graft = GyrePipeline(_NoDeviceUNet(), vae, device="cpu", inpaint_unet=_NoDeviceUNet(9), grafted_inpaint=True)
    with pytest.raises(NotImplementedError, match="grafted"):
        graft(**kw, image=torch.zeros(1, 3, 128, 128), mask_image=torch.zeros(1, 1, 128, 128))
    clip = GyrePipeline(_NoDeviceUNet(), vae, device="cpu", clip_model=object(), feature_extractor=SimpleNamespace(size=224))
    with pytest.raises(NotImplementedError, match="CLIP"):
        clip(**kw, clip_guidance_scale=0.3, clip_text_embeddings=torch.zeros(1, 8))
    with pytest.raises(ValueError, match="hint image"):
        pipe(**{**kw, "controlnet_hints": [ControlNetHint(StubControlNet(), torch.rand(1, 3, 64, 64))]})
