"""The line-art pipeline on the GPU (-m gpu; gyre_amd.hinters.GyreInformativeDrawingPipeline over the native generator): host inputs of
1 and 4 channels come back on the host in their dtype, equal to 1 - clamp(module); and one chain: the pipeline's drawing of a 64 x 64
photo goes in as the hint image of a tiny ControlNet request on the engine class - no host model between the image and the latents."""
from types import SimpleNamespace

import pytest
import torch

import lineart_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.hinters import GyreHipDrawingGenerator, GyreInformativeDrawingPipeline
from gpu_util import DEV
from test_gpu_engine import build_engine, generators, wrapper_kwargs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    cfg, sd, _ = R.model_case("shipped")
    m = GyreHipDrawingGenerator(cfg.input_nc, cfg.output_nc, cfg.n_residual_blocks, cfg.sigmoid)
    m.load_state_dict(sd)
    p = GyreInformativeDrawingPipeline(m.to(torch.float16))
    p.to(DEV)
    assert p.pipeline_modules() == [("module", p.module)] and next(p.module.parameters()).is_cuda
    return p


@pytest.mark.parametrize("channels", [1, 4])
def test_pipeline_on_host_images(pipe, channels):
    x = torch.rand((2, channels, 24, 20), generator=torch.Generator().manual_seed(channels))
    got = pipe(x)
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (2, 1, 24, 20)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    x3 = x[:, [0, 0, 0]] if channels == 1 else x[:, :3]
    want = (1 - pipe.module(x3.to(DEV, torch.float16)).clamp(0, 1)).to("cpu", torch.float32)
    assert torch.equal(got, want)
    assert torch.equal(pipe(x[0]), got[:1])                       # [C, H, W] gains its batch axis


def test_drawing_feeds_a_controlnet_request(pipe):
    photo = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(21))
    drawing = pipe(photo)
    assert tuple(drawing.shape) == (1, 1, 64, 64)
    ucfg, vcfg, ccfg = gcfg.tiny_unet(), gcfg.tiny_vae(), gcfg.tiny_controlnet()
    ctrl = GyreHipControlNet(ccfg)
    ctrl.load_state_dict(weights.synthetic_state_dict(weights.controlnet_param_shapes(ccfg), 1))
    table = {"lineart": {"lineart": ctrl.to(DEV)}}
    manager = SimpleNamespace(for_type=lambda t, default=None: table.get(t, default))
    _, _, eng = build_engine(ucfg, vcfg, hintset_manager=manager)
    eng.scheduler = "euler"

    def request(hints):
        images, nsfw = eng(**wrapper_kwargs(prompt=["a lighthouse"], negative_prompt=None, generator=generators([7]), width=64, height=64,
                                            num_inference_steps=2, hint_images=hints))
        assert tuple(images.shape) == (1, 3, 64, 64) and nsfw == [False]
        return images
    hint = SimpleNamespace(image=drawing, hint_type="lineart", weight=0.8, priority="balanced", clip_layer=None)
    got = request([hint])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, request([hint])), "two requests differ"
    assert not torch.equal(got, request([])), "the hint did not reach the latents"
