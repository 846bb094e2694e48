"""T2I-adapter hint conditioning, host side (no GPU): the fp32 restatement tests/t2i_ref.py and the hint arithmetic of
gyre_amd/hints.py against arrays the reference's own classes produced (tests/golden/t2i_vectors.npz, written by
tests/golden/make_t2i_golden.py), the shell's state-dict surface, and every combination that fails closed."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import t2i_ref
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.engine import GyreUnifiedPipeline
from gyre_amd.hints import T2IHint, combine_t2i_states
from gyre_amd.pipeline import GyrePipeline
from gyre_amd.t2i import GyreHipT2IAdapter

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "t2i_vectors.npz"))
CASES = ("main_default", "main_conv", "light")


def case(name):
    cfg = json.loads(str(GOLD[f"{name}.cfg"]))
    cfg = gcfg.t2i_config(cfg.pop("type"), **cfg)
    sd = weights.synthetic_state_dict(weights.t2i_param_shapes(cfg), int(GOLD[f"{name}.seed"]))
    return cfg, sd, torch.from_numpy(GOLD[f"{name}.image_u8"]).float() / 255


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_adapters(name):
    """both sides are the same fp32 ATen ops: the margin covers the convolution algorithm choice only"""
    cfg, sd, img = case(name)
    feats = t2i_ref.t2i_forward(sd, cfg, img)
    assert len(feats) == 4
    for i, f in enumerate(feats):
        ref = torch.from_numpy(GOLD[f"{name}.f{i}"])
        assert f.shape == ref.shape
        torch.testing.assert_close(f, ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_equal_the_reference(name):
    cfg, sd, _ = case(name)
    net = GyreHipT2IAdapter(cfg)
    assert sorted(net.state_dict().keys()) == [str(k) for k in GOLD[f"{name}.keys"]]
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == dict(weights.t2i_param_shapes(cfg))
    assert "cin" in net.config and net.config.cin == cfg["cin"] and net._coadapter_type is False
    net.load_state_dict(sd)                  # strict: the reference's key space loads as it is


class FakeModel:
    config = {}

    def __init__(self, seed):
        self.states = [torch.from_numpy(GOLD[f"states.{seed}.{i}"]) for i in range(4)]

    def __call__(self, image):
        assert image.shape[1] == 3
        return [s.clone() for s in self.states]


@pytest.mark.parametrize("name", ["balanced", "soft", "soft_cfg_only_two"])
def test_hint_weighting_and_cfg_sums_match_the_reference(name):
    spec = json.loads(str(GOLD[f"hint.{name}.spec"]))
    hints = [T2IHint(FakeModel(seed), torch.zeros(3, 8, 8), weight=w, soft_injection=soft, cfg_only=only)
             for w, soft, only, seed in spec]
    got = combine_t2i_states(hints)
    for side in ("u", "g", "f"):
        for i in range(4):
            torch.testing.assert_close(got[side][i], torch.from_numpy(GOLD[f"hint.{name}.{side}{i}"]), rtol=1e-6, atol=0)
    if name == "soft_cfg_only_two":          # the cfg_only hint is absent from the unconditional side
        assert not torch.equal(got["u"][0], got["g"][0])
    assert combine_t2i_states([]) is None


def test_hint_image_normalisation_and_masks():
    m = FakeModel(21)
    h = T2IHint(m, torch.rand(1, 8, 8))                        # grey -> three channels, batch axis added
    assert h.image.shape == (1, 3, 8, 8)
    rgba = torch.cat([torch.rand(1, 3, 8, 8), torch.ones(1, 1, 8, 8)], dim=1)
    assert T2IHint(m, rgba).image.shape == (1, 3, 8, 8)         # an alpha channel of ones is dropped
    rgba[:, 3, 0, 0] = 0.5
    with pytest.raises(NotImplementedError):
        T2IHint(m, rgba)
    sketch = SimpleNamespace(config=gcfg.T2IConfig(cin=64), _coadapter_type=False)
    assert T2IHint(sketch, torch.rand(1, 3, 8, 8)).image.shape == (1, 1, 8, 8)
    with pytest.raises(NotImplementedError):
        T2IHint(SimpleNamespace(config={}, _coadapter_type="sketch"), torch.rand(1, 3, 8, 8))


def test_from_state_dict_round_trip(tmp_path):
    cfg, sd, _ = case("light")
    torch.save(sd, tmp_path / "t2iadapter_light.pth")
    net = GyreHipT2IAdapter.from_state_dict(str(tmp_path), torch_dtype=torch.float16, type="light", channels=cfg["channels"])
    assert net.dtype == torch.float16 and net._storage() == _lib.F16 and not net.training
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k].half())
    main = gcfg.t2i_config("main")                                # the reference's defaults (models.py:82-89, 187-191)
    assert (main.cin, main.channels, main.nums_rb, main.ksize, main.sk, main.use_conv) == (192, (320, 640, 1280, 1280), 2, 1, True, False)
    assert gcfg.t2i_config("light").nums_rb == 4
    for t in ("style", "fuser"):
        with pytest.raises(NotImplementedError):
            GyreHipT2IAdapter.from_state_dict(str(tmp_path), type=t)
    with pytest.raises(RuntimeError):
        GyreHipT2IAdapter.from_state_dict(str(tmp_path / "nothing"))
    with pytest.raises(NotImplementedError):                      # the reference's own block cannot change width without sk
        GyreHipT2IAdapter(gcfg.tiny_t2i("main", sk=False))
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 60, 64))                            # H not a multiple of 8: refused before any device work


def test_library_exports_the_t2i_symbols():
    names = ["gyre_t2i_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    names += ["gyre_op_pixel_unshuffle8", "gyre_op_avgpool2", "gyre_op_relu"]
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS
        for L in _lib.all_libs():
            assert hasattr(L, n)


class _NoDeviceUNet:
    config = gcfg.tiny_unet()

    def __call__(self, *a, **k):
        raise AssertionError("no UNet call may happen before the refusal")


def test_unsupported_combinations_fail_closed_without_a_gpu():
    hint = T2IHint(FakeModel(21), torch.rand(1, 3, 128, 128))
    text = torch.zeros(1, 77, 64)
    kw = dict(seeds=[1], text_embeddings=text, uncond_embeddings=text, height=128, width=128, num_inference_steps=2,
              sampler="euler", t2i_hints=[hint])
    pipe = GyrePipeline(_NoDeviceUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu")
    with pytest.raises(NotImplementedError, match="hires"):
        pipe(**{**kw, "height": 256, "width": 256})
    graft = GyrePipeline(_NoDeviceUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu", inpaint_unet=_NoDeviceUNet(),
                         grafted_inpaint=True)
    with pytest.raises(NotImplementedError, match="grafted"):
        graft(**kw, image=torch.zeros(1, 3, 128, 128), mask_image=torch.zeros(1, 1, 128, 128))
    clip = GyrePipeline(_NoDeviceUNet(), SimpleNamespace(config=gcfg.tiny_vae()), device="cpu", clip_model=object(),
                        feature_extractor=SimpleNamespace(size=224))
    with pytest.raises(NotImplementedError, match="CLIP"):
        clip(**kw, clip_guidance_scale=0.3, clip_text_embeddings=torch.zeros(1, 8))


def _engine(manager, **kw):
    unet = torch.nn.Linear(1, 1)                 # (execution_device reads a parameter; nothing runs)
    unet.config = gcfg.tiny_unet()
    eng = GyreUnifiedPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, scheduler="euler", hintset_manager=manager, **kw)
    return eng


def _hint(hint_type="sketch", **kw):
    return SimpleNamespace(**{"image": torch.rand(1, 3, 128, 128), "hint_type": hint_type, "weight": None, "priority": "balanced",
                              "clip_layer": None, **kw})


def test_engine_hint_routing_fails_closed():
    adapter = GyreHipT2IAdapter(gcfg.tiny_t2i("main"))
    table = {"sketch": {"model": adapter, "clip_model": object(), "fuser": None}, "canny": {"controlnet": torch.nn.Linear(1, 1)}}
    manager = SimpleNamespace(for_type=lambda t, default=None: table.get(t, default))
    eng = _engine(manager)
    hints = eng._hints([_hint(weight=0.8, priority="prompt"), _hint(priority="hint")], None)
    assert [(h.weight, h.soft_injection, h.cfg_only) for h in hints] == [(0.8, True, False), (1.0, True, True)]
    assert hints[0].model is adapter and eng._hints(None, None) == []
    with pytest.raises(NotImplementedError):                      # a ControlNet-like handler
        eng(prompt="x", hint_images=[_hint("canny")])
    with pytest.raises(EnvironmentError, match="doesn't know how to handle hint image of type pose"):
        eng(prompt="x", hint_images=[_hint("pose")])
    with pytest.raises(EnvironmentError):
        _engine(None)(prompt="x", hint_images=[_hint()])
    with pytest.raises(NotImplementedError):
        eng(prompt="x", depth_map=torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError):                      # depth hints go to the depth UNet when there is one
        _engine(manager, depth_unet=object())(prompt="x", hint_images=[_hint("depth")])
    eng._shard_devices = [torch.device("cpu"), torch.device("cpu")]
    with pytest.raises(NotImplementedError, match="shard_devices"):
        eng(prompt="x", hint_images=[_hint()])
