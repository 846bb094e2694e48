"""Host side of the upscaler path (CPU only): tile geometry and blend over toy torch modules, the pipeline's alpha and rescale
handling, the loader's defaults, old-format key conversion and refusals, the Gaussian blur and lanczos3 restatements, export names."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from gyre_amd import _lib, config as gcfg, images, resize, weights
from gyre_amd import upscaler as U


class Up(torch.nn.Module):
    """nearest-neighbour upscaling: a module whose tiled result is known in closed form"""

    def __init__(self, scale):
        super().__init__()
        self.scale, self.calls, self.w = scale, [], torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        return F.interpolate(x, scale_factor=self.scale, mode="nearest")


class Conv(torch.nn.Module):
    """a batch-independent module with a receptive field: 3x3 convolution, then nearest 2x"""

    def __init__(self):
        super().__init__()
        self.c = torch.nn.Conv2d(3, 3, 3, padding=1)
        self._scale = 2

    def forward(self, x):
        return F.interpolate(torch.stack([self.c(s[None])[0] for s in x]), scale_factor=2, mode="nearest")


def test_tile_plan_of_the_headline_request():
    # 512 x 512 at tile 256: 576 padded, three tiles per axis overlapping by 96 >= 64 -> the 9 tiles of one request
    ts, pad, half, ys, xs = U.tile_plan(512, 512, 4, 256)
    assert (ts, pad, half, ys, xs) == (256, 32, 64, [0, 160, 320], [0, 160, 320])
    # the tile shrinks to the largest multiple of the window inside the image, each axis gets its own count
    with pytest.raises(ValueError, match="feather"):           # a quarter of a 64-pixel tile is less than the default 32-pixel feather
        U.tile_plan(100, 90, 4, 64)
    ts, pad, half, ys, xs = U.tile_plan(100, 90, 4, 64, feather=8)
    assert ts == 64 and half == 16 and len(ys) == 4 and len(xs) == 3 and ys[0] == 0 and ys[-1] == 164 - 64 and xs[-1] == 154 - 64
    for offs, padded in ((ys, 164), (xs, 154)):
        steps = [b - a for a, b in zip(offs, offs[1:])]
        assert all(64 - s >= 16 for s in steps) and max(steps) - min(steps) <= 1           # overlap >= 25 %, evenly spread
    with pytest.raises(ValueError):
        U.tile_plan(100, 100, 4, 48)
    with pytest.raises(ValueError):
        U.tile_plan(300, 300, 4, 256, feather=40)


def test_feather_map_shape_and_profile():
    fm = U.feather_map(256, 64, torch.zeros(1))
    assert fm.shape == (1, 1, 256, 256) and float(fm.max()) <= 1.0 + 1e-6 and float(fm.min()) >= 0.0
    assert abs(float(fm[0, 0, 128, 64]) - 0.5) < 0.02           # half way across the edge of the white square
    assert float(fm[0, 0, 128, 0]) < 5e-3 and float(fm[0, 0, 128, 127]) > 1 - 5e-3
    assert float((fm - fm.flip(-1)).abs().max()) < 1e-5 and float((fm - fm.transpose(-1, -2)).abs().max()) < 1e-5
    assert U.feather_map(256, 0, torch.zeros(1)) is None


@pytest.mark.parametrize("scale", [1, 2, 4])
def test_tiled_pointwise_module_reproduces_the_untiled_result(scale):
    x = torch.rand((2, 3, 100, 90), generator=torch.Generator().manual_seed(scale))
    m = Up(scale)
    got = U.tile(x, m, scale, 64, feather=8)
    want = F.interpolate(x, scale_factor=scale, mode="nearest")
    assert got.shape == want.shape
    # every output pixel is a feathered mix of tiles that agree on it.  The sequential blend keeps a value only where the feather bands
    # of two overlapping tiles do not meet, i.e. feather <= overlap / 2: 8 against the 16 pixels a 64-pixel tile guarantees (the
    # defaults have the same margin: 32 against 64).  The band itself is within 0.05 % of 0 / 1 at its ends.
    assert float((got - want).abs().max()) < 1e-2
    assert len(m.calls) == 1 and m.calls[0] == (2 * 12, 3, 64, 64)        # 4 x 3 tiles as ONE stacked batch
    m2 = Up(scale)
    seq = U.tile(x, m2, scale, 64, feather=8, stacked=False)
    assert len(m2.calls) == 12 and all(c == (2, 3, 64, 64) for c in m2.calls)
    assert torch.equal(got, seq)


def test_stacked_equals_tile_by_tile_with_a_receptive_field():
    torch.manual_seed(0)
    m = Conv()
    x = torch.rand((2, 3, 70, 100))
    with torch.no_grad():
        a, b = U.tile(x, m, 2, 64, feather=8), U.tile(x, m, 2, 64, feather=8, stacked=False)
        assert a.shape == (2, 3, 140, 200) and torch.equal(a, b)
        # away from the image border the reflect padding plays no part and a tile's interior equals the untiled module
        whole = m(x)
        assert float((a - whole)[..., 8:-8, 8:-8].abs().max()) < 1e-2 * float(whole.abs().max())


def test_stack_is_capped_and_the_result_does_not_depend_on_it():
    x = torch.rand((2, 3, 100, 90), generator=torch.Generator().manual_seed(9))
    whole, capped = Up(2), Up(2)
    a = U.tile(x, whole, 2, 64, feather=8)
    b = U.tile(x, capped, 2, 64, feather=8, max_stack=5)                # 12 tiles: 5 + 5 + 2
    assert torch.equal(a, b) and [c[0] for c in capped.calls] == [10, 10, 4] and len(whole.calls) == 1
    many = Up(1)
    U.tile(torch.rand(1, 3, 40, 200), many, 1, 32, feather=8)           # the default cap: 16 tiles per call
    _, _, _, ys, xs = U.tile_plan(40, 200, 1, 32, feather=8)
    n = len(ys) * len(xs)
    assert n > 32 and n % 16 and [c[0] for c in many.calls] == [16] * (n // 16) + [n % 16]


def test_untiled_shortcut():
    m = Up(4)
    x = torch.rand((1, 3, 64, 48))
    assert torch.equal(U.tile(x, m, 4, 64), F.interpolate(x, scale_factor=4, mode="nearest")) and m.calls == [(1, 3, 64, 48)]


def test_pipeline_alpha_and_rescale():
    m = Up(2)
    m._scale = 2
    pipe = U.GyreUpscalerPipeline(m)
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand((1, 3, 40, 36), generator=g) * 1.4 - 0.2                  # leaves [0, 1]: the result is clamped
    const = torch.cat([rgb, torch.full((1, 1, 40, 36), 0.25)], 1)
    (out,) = pipe(const)
    assert out.shape == (1, 4, 80, 72) and float(out[:, :3].min()) >= 0 and float(out[:, :3].max()) <= 1
    assert bool((out[:, 3] == 0.25).all())                                     # constant alpha: replicated, not resampled
    ramp = torch.linspace(0, 1, 36).expand(1, 1, 40, 36)
    (out,) = pipe(torch.cat([rgb, ramp], 1))
    assert out.shape == (1, 4, 80, 72)
    assert torch.equal(out[:, [3]], images.resize(ramp, 2))                    # lanczos3, antialias, reflect, clamped
    assert float((out[0, 3, :, 1:] - out[0, 3, :, :-1]).min()) > -1e-3        # still a ramp
    (out,) = pipe(rgb, width=36, height=40)                                    # the input's own size: ignored
    assert out.shape == (1, 3, 80, 72)
    (out,) = pipe(rgb, width=60, height=80)                                    # "cover": scale by the larger factor, crop the centre
    assert out.shape == (1, 3, 80, 60)
    with pytest.raises(ValueError):
        pipe(None)
    from PIL import Image                                                      # a PIL image is taken as the reference takes it
    u8 = (torch.rand((40, 36, 4), generator=g) * 255).to(torch.uint8)
    (out,) = pipe(Image.fromarray(u8.numpy(), "RGBA"))
    (want,) = pipe((u8.float() / 255).permute(2, 0, 1)[None])
    assert out.shape == (1, 4, 80, 72) and torch.equal(out, want)


def test_rescale_fits():
    x = torch.rand((1, 3, 20, 30), generator=torch.Generator().manual_seed(1))
    assert images.rescale(x, 40, 40, "cover").shape == (1, 3, 40, 40)
    c = images.rescale(x, 40, 40, "contain")
    assert c.shape == (1, 3, 40, 40) and bool((c[..., :6, :] == 0).all()) and bool((c[..., -6:, :] == 0).all())
    assert images.rescale(x, 10, 45, "strict").shape == (1, 3, 10, 45)
    assert images.scale_shape((1, 3, 5, 7), 2.5) == (1, 3, 12, 18)
    # odd differences: the surplus is cut one pixel deeper in front, the shortfall padded one pixel more behind; a shortfall of one stays
    assert [images._fit_axis(h, 10) for h in (13, 12, 10, 7, 6, 9)] == [(2, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 2), (0, 2, 2), (0, 0, 0)]
    ramp = torch.arange(8.0).expand(1, 1, 8, 8) / 8
    cov = images.rescale(ramp, 8, 5, "cover")                                 # factor 1: the resize is the identity, columns 2 .. 6 stay
    assert cov.shape == (1, 1, 8, 5) and float((cov - ramp[..., 2:7]).abs().max()) < 1e-6
    assert images.rescale(ramp, 16).shape == (1, 1, 16, 16)
    with pytest.raises(ValueError):
        images.resize(x, (1, 2, 3))
    with pytest.raises(NotImplementedError):
        images.resize(x, 0.5, sharpness=0)


def test_gaussian_blur_restatement():
    x = torch.rand((2, 3, 17, 23), generator=torch.Generator().manual_seed(2))
    sigma = 1.3                                                                # kernel ceil(7.8) = 8 -> 9 taps
    k = torch.exp(-0.5 * (torch.arange(-4, 5).float() / sigma) ** 2)
    k = k / k.sum()
    rows = F.conv2d(F.pad(x, (4, 4, 0, 0), mode="reflect").reshape(6, 1, 17, 31), k.view(1, 1, 1, 9))
    want = F.conv2d(F.pad(rows, (0, 0, 4, 4), mode="reflect"), k.view(1, 1, 9, 1)).reshape(2, 3, 17, 23)
    got = images.gaussianblur(x, sigma)
    assert got.shape == x.shape and float((got - want).abs().max()) < 1e-6
    assert abs(float(images.gaussianblur(torch.ones(1, 1, 9, 9), 0.7).mean()) - 1) < 1e-6


def test_lanczos3_kernel():
    t = torch.tensor([0.0, 0.5, 1.0, 2.0, 2.5, 3.0, 3.5], dtype=torch.float64)
    want = torch.where(t.abs() < 3, torch.sinc(t) * torch.sinc(t / 3), torch.zeros_like(t))
    assert float((resize.lanczos3(t) - want).abs().max()) < 1e-6
    m = resize._weight_matrix_general(10, 20, 2.0, "lanczos3", True, "reflect")
    assert m.shape == (20, 10) and float((m.sum(1) - 1).abs().max()) < 1e-6
    ramp = torch.arange(10.0)[None, None, None, :].expand(1, 1, 4, 10)
    up = resize.resize_right(ramp, scale_factors=(1.0, 2.0), interp_method="lanczos3", pad_mode="reflect")
    assert up.shape == (1, 1, 4, 20) and float((up[0, 0, 0, 6:14] - (torch.arange(6, 14) / 2 - 0.25)).abs().max()) < 0.03      # (lanczos ripples on a ramp)


# ---- loader ----------------------------------------------------------------------------------------------------------------------------
def test_loader_default_configurations():
    assert U.DEFAULT_CONFIGS["esrgan"] == dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=23, num_grow_ch=32, scale=4)
    assert U.DEFAULT_CONFIGS["esrgan-plus"] == U.DEFAULT_CONFIGS["esrgan"]
    assert U.DEFAULT_CONFIGS["esrgan-6B"] == dict(U.DEFAULT_CONFIGS["esrgan"], num_block=6)
    for name in ("esrgan", "esrgan_old", "esrgan_plus", "realesrgan", "realesrgan_6B", "swinir", "hat", "load"):
        assert callable(getattr(U.GyreHipUpscalerLoader, name))


def _old_format(sd, num_block):
    return {("module." if i % 2 else "") + U.old_esrgan_key(k, num_block): v for i, (k, v) in enumerate(sd.items())}


def test_old_format_key_conversion():
    assert U.old_esrgan_key("body.7.rdb2.conv3.weight", 23) == "model.1.sub.7.RDB2.conv3.0.weight"
    assert U.old_esrgan_key("body.0.rdb1.conv1x1.weight", 23) == "model.1.sub.0.RDB1.conv1x1.weight"
    assert U.old_esrgan_key("conv_body.bias", 23) == "model.1.sub.23.bias"
    assert [U.old_esrgan_key(k + ".weight", 23) for k in ("conv_first", "conv_up1", "conv_up2", "conv_hr", "conv_last")] == \
        [f"model.{i}.weight" for i in (0, 3, 6, 8, 10)]
    cfg = gcfg.tiny_rrdb(plus=True)
    shapes = weights.rrdb_param_shapes(cfg)
    sd = weights.synthetic_state_dict(shapes)
    old = _old_format(sd, cfg.num_block)
    old["body.0.rdb1.conv1x1.weight"] = old.pop("model.1.sub.0.RDB1.conv1x1.weight")      # already under its new name: taken as it is
    back = U.convert_old_esrgan(old, shapes, cfg.num_block)
    assert list(back) == list(shapes) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="Missing tensor"):
        U.convert_old_esrgan({k: v for k, v in old.items() if "model.8." not in k}, shapes, cfg.num_block)
    with pytest.raises(ValueError, match="Unconverted"):
        U.convert_old_esrgan(dict(old, extra=torch.zeros(1)), shapes, cfg.num_block)


def test_loader_round_trips_and_refusals(tmp_path):
    from safetensors.torch import save_file
    cfg = gcfg.tiny_rrdb()
    sd = weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))
    new_dir, old_dir, ema_dir = tmp_path / "new", tmp_path / "old", tmp_path / "ema"
    for d in (new_dir, old_dir, ema_dir):
        os.makedirs(d)
    save_file(sd, str(new_dir / "model.safetensors"))
    (new_dir / "config.yaml").write_text("num_block: 2\n")
    m = U.GyreHipUpscalerLoader.realesrgan(str(new_dir), torch_dtype=torch.float16)
    assert m.config.num_block == 2 and m._scale == 4 and m._window_size == 32 and m.dtype == torch.float16 and not m.training
    assert all(torch.equal(v, sd[k].half()) for k, v in m.state_dict().items())
    torch.save(_old_format(sd, 2), str(old_dir / "old.pth"))
    (old_dir / "config.yaml").write_text("num_block: 2\n")
    m = U.GyreHipUpscalerLoader.esrgan_old(str(old_dir))
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    torch.save({"params_ema": sd, "params": {}}, str(ema_dir / "net.pt"))
    (ema_dir / "config.yaml").write_text("num_block: 2\n")
    m = U.GyreHipUpscalerLoader.esrgan(str(ema_dir))
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.swinir(str(new_dir))
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.load(str(new_dir), network="hat")
    with pytest.raises(ValueError):
        U.GyreHipUpscalerLoader.load(str(new_dir), network="bsrgan")
    with pytest.raises(FileNotFoundError):
        U.GyreHipUpscalerLoader.esrgan(str(tmp_path))
    (new_dir / "config.yaml").write_text("num_block: 2\nnum_feat: 48\n")
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.esrgan(str(new_dir))                          # a width the native path lacks
    with pytest.raises(NotImplementedError):
        gcfg.rrdb_config(num_grow_ch=16)
    with pytest.raises(NotImplementedError):
        gcfg.rrdb_config(scale=8)


def test_model_shell():
    m = U.GyreHipRRDBNet(gcfg.tiny_rrdb(plus=True))
    keys = list(m.state_dict())
    assert keys == list(weights.rrdb_param_shapes(m.config)) and "body.1.rdb3.conv1x1.weight" in keys and keys[0] == "conv_first.weight"
    assert m._scale == 4 and m._window_size == 32 and m.out_shape((2, 3, 24, 20)) == (2, 3, 96, 80)
    assert weights.rrdb_param_shapes(gcfg.tiny_rrdb(scale=1))["conv_first.weight"] == (64, 48, 3, 3)
    n = sum(math.prod(s) for s in weights.rrdb_param_shapes(gcfg.rrdb_config()).values())
    assert n == 16_697_987                                                   # RRDBNet x4, 23 blocks: the published parameter count
    with pytest.raises(_lib.GyreError):
        m(torch.rand(1, 3, 8, 8))                                             # CPU tensors: no fallback
    with pytest.raises(ValueError):
        m(torch.rand(1, 4, 8, 8))
    with pytest.raises(ValueError):
        m.set_path("fast")


def test_export_names():
    names = ["gyre_rrdb_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward", "set_path")]
    names += ["gyre_op_rdb_conv", "gyre_op_rdb_epilogue", "gyre_op_pixel_unshuffle", "gyre_op_rdb_tile"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
