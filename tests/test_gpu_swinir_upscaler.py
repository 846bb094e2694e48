"""Loader -> GyreUpscalerPipeline on a tiny SwinIR (-m gpu): a folder with a checkpoint and a yaml goes through
GyreHipUpscalerLoader.swinir, the pipeline tiles a 100 x 90 image 4 x 3 at tile_size=64 (with feather=8: the reference's own rule
refuses a 64-pixel tile with the default 32-pixel feather, tests/test_gpu_upscaler.py), stacked batches are bit-equal to tile by tile,
RGB and RGBA inputs, output shape and range."""
import os

import pytest
import torch

import swinir_ref as R
from gyre_amd import upscaler as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    from safetensors.torch import save_file
    cfg, sd, _ = R.model_case("tiny")
    d = tmp_path_factory.mktemp("swinir")
    full = U.GyreHipSwinIR(cfg).state_dict()                                   # the buffers ride along, as in a real checkpoint
    full.update(sd)
    save_file({k: v.contiguous() for k, v in full.items()}, str(d / "model.safetensors"))
    (d / "config.yaml").write_text("depths: [2, 2]\nnum_heads: [2, 2]\nembed_dim: 60\nimg_size: 16\n")
    m = U.GyreHipUpscalerLoader.swinir(str(d), torch_dtype=torch.float16)
    assert m.config.embed_dim == 60 and m._scale == 4 and m._window_size == 8
    return U.GyreUpscalerPipeline(m).to(DEV), cfg, sd


def test_tiled_pipeline_stacked_equals_tile_by_tile(pipe):
    p, cfg, sd = pipe
    img = torch.rand((1, 3, 100, 90), generator=torch.Generator().manual_seed(2))
    (a,) = p(img.to(DEV), tile_size=64, feather=8)
    (b,) = p(img.to(DEV), tile_size=64, feather=8, stacked=False)
    assert tuple(a.shape) == (1, 3, 400, 360) and a.dtype == img.dtype
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and bool(torch.isfinite(a).all())
    assert torch.equal(a.cpu(), b.cpu()), "stacked tiles differ from tile by tile"
    assert float(a.std()) > 0.01


def test_untiled_rgb_and_rgba(pipe):
    p, cfg, sd = pipe
    img = torch.rand((1, 4, 24, 40), generator=torch.Generator().manual_seed(3))
    (rgb,) = p(img[:, :3].to(DEV))
    (rgba,) = p(img.to(DEV))
    assert tuple(rgb.shape) == (1, 3, 96, 160) and tuple(rgba.shape) == (1, 4, 96, 160)
    assert torch.equal(rgb.cpu(), rgba[:, :3].cpu())
    assert float(rgba.min()) >= 0.0 and float(rgba.max()) <= 1.0
    want = R.net(sd, cfg, img[:, :3]).clamp(0, 1)
    d = R.rel_l2(rgb.float().cpu(), want)
    print(f"[swinir] pipeline 24x40 fp16: rel-L2 against the fp32 net {d:.3e}")
    assert d <= 2 * 5.073e-04                                                   # the model gate of tests/test_gpu_swinir_model.py (tiny, fp16)
    (sized,) = p(img[:, :3].to(DEV), width=100, height=60)
    assert tuple(sized.shape) == (1, 3, 60, 100)
