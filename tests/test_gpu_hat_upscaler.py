"""Loader -> GyreUpscalerPipeline on a tiny HAT (-m gpu): a folder with a checkpoint and a yaml goes through GyreHipUpscalerLoader.hat,
the pipeline tiles a 48 x 80 image 5 x 6 at tile_size=32 (with feather=8: the reference's own rule refuses a 32-pixel tile with the
default 32-pixel feather), and the result is held to the same tiling over the fp32 restatement of the net (tests/hat_ref.py)."""
import pytest
import torch

import hat_ref as R
from gyre_amd import upscaler as U
from gpu_util import DEV
from test_hat_ref_host import EMULATION

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    from safetensors.torch import save_file
    cfg, sd, _ = R.model_case("tiny")
    d = tmp_path_factory.mktemp("hat")
    full = U.GyreHipHAT(cfg).state_dict()                                      # the buffers ride along, as in a real checkpoint
    full.update(sd)
    save_file({k: v.contiguous() for k, v in full.items()}, str(d / "model.safetensors"))
    (d / "config.yaml").write_text("depths: [2, 2]\nnum_heads: [2, 2]\nembed_dim: 60\n")
    m = U.GyreHipUpscalerLoader.hat(str(d), torch_dtype=torch.float16)
    assert isinstance(m, U.GyreHipHAT) and m.config.embed_dim == 60 and m._scale == 4 and m._window_size == 16
    return U.GyreUpscalerPipeline(m).to(DEV), cfg, sd


def test_tiled_pipeline_against_tiling_over_the_fp32_net(pipe):
    p, cfg, sd = pipe
    img = torch.rand((1, 3, 48, 80), generator=torch.Generator().manual_seed(2)).half().float()      # (the pipeline casts to the model's dtype)
    (a,) = p(img.to(DEV), tile_size=32, feather=8)
    (b,) = p(img.to(DEV), tile_size=32, feather=8, stacked=False)
    assert tuple(a.shape) == (1, 3, 192, 320) and a.dtype == img.dtype
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and bool(torch.isfinite(a).all())
    assert torch.equal(a.cpu(), b.cpu()), "stacked tiles differ from tile by tile"
    want = U.tile(img, lambda t: R.net(sd, cfg, t), 4, 32, feather=8).clamp(0, 1)
    d = R.rel_l2(a.float().cpu(), want)
    print(f"[hat] tiled pipeline 48x80 fp16: rel-L2 against tile() over the fp32 net {d:.3e}")
    assert d <= 2 * EMULATION[("tiny", torch.float16)]                         # the model gate of tests/test_gpu_hat_model.py (tiny, fp16)
