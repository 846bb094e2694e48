"""The upscaler pipeline end to end on the GPU (-m gpu): GyreUpscalerPipeline over the native RRDBNet against the same host tile
logic driven by the fp32 restatement of the net (tests/rrdb_ref.py), stacked against tile-by-tile calls, alpha handling, a final
rescale, and the loader's round trip through a .safetensors folder."""
import os

import pytest
import torch

import rrdb_ref as R
from gyre_amd import config as gcfg, images, weights
from gyre_amd.upscaler import GyreHipRRDBNet, GyreHipUpscalerLoader, GyreUpscalerPipeline
from gpu_util import DEV

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
# The image of the request: 100 x 90 with a fourth, non-constant plane.  tile_size = 64 tiles it 4 x 3 (padded 164 x 154).  The
# reference's own rule refuses a 64-pixel tile with the default 32-pixel feather (a quarter of the tile must cover it), so the
# request passes feather = 8: the widest band the guaranteed 16-pixel overlap blends without loss.
TILE = dict(tile_size=64, feather=8)
# rel-L2 of the colour planes of the SAME pipeline on the CPU over the emulation that rounds every stored tensor (and the
# pipeline's own tensors: image, tiles, blend) to the storage type, against the fp32 pipeline over the fp32 net - measured by
# _emulation_distance() below on the build machine; the gate is twice that.
EMULATION = {torch.bfloat16: 1.285e-02, torch.float16: 1.185e-03}
_SHARED = {}


class HostNet(torch.nn.Module):
    """the CPU restatement behind the module surface the pipeline drives"""

    def __init__(self, sd, cfg, dtype=torch.float32, store=None):
        super().__init__()
        self.sd, self.cfg, self.store, self._scale = sd, cfg, store, cfg["scale"]
        self.p = torch.nn.Parameter(torch.zeros(1, dtype=dtype), requires_grad=False)

    def forward(self, x):
        return R.net(self.sd, self.cfg, x, store=self.store).to(self.p.dtype)


def _shared():
    if not _SHARED:
        cfg = gcfg.tiny_rrdb()
        sd = weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))
        g = torch.Generator().manual_seed(11)
        rgb = torch.rand((1, 3, 100, 90), generator=g)
        alpha = (torch.linspace(0, 1, 90)[None, :] * torch.linspace(1, 0.5, 100)[:, None])[None, None]
        image = torch.cat([rgb, alpha], 1)
        (ref,) = GyreUpscalerPipeline(HostNet(sd, cfg))(image, **TILE)
        _SHARED.update(cfg=cfg, sd=sd, image=image, ref=ref)
    return _SHARED


def _emulation_distance(sdt):
    s = _shared()
    (emu,) = GyreUpscalerPipeline(HostNet(s["sd"], s["cfg"], dtype=sdt, store=sdt))(s["image"], **TILE)
    return R.rel_l2(emu[:, :3], s["ref"][:, :3])


def _native(sdt, path="auto"):
    s = _shared()
    m = GyreHipRRDBNet(s["cfg"])
    m.load_state_dict(s["sd"])
    m = m.to(sdt).to(DEV)
    m.set_path(path)
    return m


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("path", ["generic", "fused"])
def test_pipeline_against_host_tiling_over_the_fp32_net(path, sdt):
    s = _shared()
    pipe = GyreUpscalerPipeline(_native(sdt, path))
    (got,) = pipe(s["image"].to(DEV), **TILE)
    assert got.shape == (1, 4, 400, 360) and got.dtype == torch.float32 and got.device.type == "cuda"
    got = got.cpu()
    d, gate = R.rel_l2(got[:, :3], s["ref"][:, :3]), 2 * EMULATION[sdt]
    print(f"[upscaler] {path} {sdt}: colour rel-L2 against the fp32 host pipeline {d:.3e} (emulation {EMULATION[sdt]:.3e}, gate {gate:.3e})")
    assert d <= gate
    assert float(got[:, :3].min()) >= 0 and float(got[:, :3].max()) <= 1
    # the alpha plane never meets the model: lanczos3 of the plane rounded to the storage type, rounded again
    u = 2.0 ** -8 if sdt == torch.bfloat16 else 2.0 ** -11
    assert float((got[:, 3] - s["ref"][:, 3]).abs().max()) <= 4 * u
    with pytest.raises(ValueError, match="feather"):
        pipe(s["image"].to(DEV), tile_size=64)                      # the reference's rule: a 16-pixel overlap cannot carry a 32-pixel feather


@pytest.mark.parametrize("sdt", SDTS)
def test_stacked_batch_equals_tile_by_tile(sdt):
    s = _shared()
    pipe = GyreUpscalerPipeline(_native(sdt))
    x = s["image"][:, :3].to(DEV)
    (a,) = pipe(x, **TILE)
    (b,) = pipe(x, stacked=False, **TILE)
    assert torch.equal(a, b)


def test_constant_alpha_and_requested_size():
    s = _shared()
    pipe = GyreUpscalerPipeline(_native(torch.float16))
    image = s["image"].clone()
    image[:, 3] = 0.75
    (out,) = pipe(image.to(DEV), width=300, height=380, **TILE)
    assert out.shape == (1, 4, 380, 300)                            # 400 x 360 scaled by 0.95 ("cover"), 42 columns cropped
    (full,) = pipe(image.to(DEV), **TILE)
    assert bool((full[:, 3] == 0.75).all())
    want = images.rescale(full, 380, 300, "cover")                  # (the pipeline resamples the fp16 result and rounds it once more)
    assert float((out - want).abs().max()) <= 2.0 ** -10
    (small,) = pipe(image[..., :64, :48].to(DEV))                   # fits one tile: the module sees the image itself
    m = pipe.module
    assert torch.equal(small[:, :3], m(image[:, :3, :64, :48].to(DEV).half()).clamp(0, 1).float())


def test_loader_round_trip(tmp_path):
    from safetensors.torch import save_file
    s = _shared()
    save_file(s["sd"], str(tmp_path / "net.safetensors"))
    (tmp_path / "config.yaml").write_text("num_block: 2\n")
    m = GyreHipUpscalerLoader.realesrgan(str(tmp_path), torch_dtype=torch.float16).to(DEV)
    x = s["image"][:, :3, :32, :40].to(DEV)
    assert torch.equal(m(x), _native(torch.float16)(x))
    assert os.path.samefile(m._source, tmp_path)
