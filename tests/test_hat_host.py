"""Host side of the HAT upscaler (gyre_amd.config / weights / upscaler), no GPU: configuration refusals, the module shell and its
buffers, loader round trips, the stored outputs of the reference's own HAT against tests/hat_ref.py, the ABI exports."""
import math
import os

import numpy as np
import pytest
import torch

import hat_ref as R
from gyre_amd import _lib, config as gcfg, upscaler as U, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hat_vectors.npz")


def test_default_tables_and_entry_points():
    assert U.DEFAULT_CONFIGS["hat"] == gcfg.HAT_DEFAULTS["hat"] and U.DEFAULT_CONFIGS["hat-l"] == gcfg.HAT_DEFAULTS["hat-l"]
    s, l = gcfg.HAT_DEFAULTS["hat"], gcfg.HAT_DEFAULTS["hat-l"]
    assert (s["embed_dim"], s["num_heads"], s["depths"]) == (180, [6] * 6, [6] * 6)
    assert (l["embed_dim"], l["num_heads"], l["depths"]) == (180, [6] * 12, [6] * 12)
    for t in (s, l):
        assert (t["window_size"], t["mlp_ratio"], t["upsampler"], t["upscale"], t["img_size"], t["img_range"], t["resi_connection"]) == \
            (16, 2, "pixelshuffle", 4, 64, 1.0, "1conv")
        assert (t["compress_ratio"], t["squeeze_factor"], t["conv_scale"], t["overlap_ratio"]) == (3, 30, 0.01, 0.5)
    assert U.ENTRY_POINTS["hat"] == dict(network="hat") and U.ENTRY_POINTS["hat_l"] == dict(network="hat", config="hat-l")
    gcfg.hat_config(**s), gcfg.hat_config(**l)


@pytest.mark.parametrize("kw", [dict(window_size=8), dict(window_size=7), dict(upsampler="nearest+conv"), dict(upsampler="pixelshuffledirect"),
                                dict(upsampler=""), dict(upscale=3), dict(upscale=8), dict(embed_dim=96), dict(num_heads=[2, 4]),
                                dict(embed_dim=270, num_heads=[9, 9]), dict(mlp_ratio=2.05), dict(ape=True), dict(patch_norm=False),
                                dict(qkv_bias=False), dict(in_chans=1), dict(resi_connection="identity"), dict(resi_connection="3conv"),
                                dict(depths=[2]), dict(overlap_ratio=0.25), dict(compress_ratio=4), dict(squeeze_factor=16),
                                dict(num_block=2), dict(scale=4), dict(qk_scale=0.5)])
def test_config_refusals(kw):
    with pytest.raises(NotImplementedError):
        gcfg.tiny_hat(**kw)


def test_constructor_defaults_are_outside_the_built_list():
    with pytest.raises(NotImplementedError):
        gcfg.hat_config()                                                        # HAT(): window 7, no upsampler


def test_model_shell_and_buffers():
    m = U.GyreHipHAT(gcfg.tiny_hat())
    shapes = weights.hat_param_shapes(m.config)
    sd = m.state_dict()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert m._scale == 4 and m._window_size == 16 and m.out_shape((2, 3, 16, 32)) == (2, 3, 64, 128)
    assert sd["relative_position_index_SA"].shape == (256, 256) and sd["relative_position_index_OCA"].shape == (256, 576)
    assert sd["relative_position_index_SA"].dtype == torch.long
    params = dict(m.named_parameters())
    assert not any(weights.hat_is_buffer(k) for k in params) and len(params) + 2 == len(sd)
    big = weights.hat_param_shapes(gcfg.hat_config(**gcfg.HAT_DEFAULTS["hat"]))
    assert big["layers.5.residual_group.overlap_attn.relative_position_bias_table"] == (1521, 6)
    assert big["layers.0.residual_group.blocks.0.conv_block.cab.3.attention.1.weight"] == (6, 180, 1, 1)
    assert big["upsample.2.weight"] == (256, 64, 3, 3)
    n = sum(math.prod(s) for k, s in big.items() if not weights.hat_is_buffer(k))
    assert n == 20_772_507                                                       # HAT x4: 20.8 M parameters
    x2 = weights.hat_param_shapes(gcfg.tiny_hat(upscale=2))
    assert "upsample.0.weight" in x2 and "upsample.2.weight" not in x2
    with pytest.raises(_lib.GyreError):
        m(torch.rand(1, 3, 16, 16))                                              # CPU tensors: no fallback
    with pytest.raises(ValueError):
        m(torch.rand(1, 4, 16, 16))
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 24, 16))                                              # no host padding: multiples of 16 only


def test_loader_round_trips(tmp_path):
    from safetensors.torch import save_file
    cfg = gcfg.hat_config(**{**gcfg.HAT_DEFAULTS["hat"], "depths": [2], "num_heads": [6]})
    shapes = weights.hat_param_shapes(cfg)
    sd = weights.synthetic_state_dict(shapes)
    sd = {k: (torch.zeros(shapes[k], dtype=torch.long) if weights.hat_is_buffer(k) else v) for k, v in sd.items()}
    params = {k: v for k, v in sd.items() if not weights.hat_is_buffer(k)}
    m_dir, l_dir = tmp_path / "m", tmp_path / "l"
    for d in (m_dir, l_dir):
        os.makedirs(d)
    save_file(sd, str(m_dir / "model.safetensors"))                              # a full checkpoint, buffers present: strict load
    (m_dir / "config.yaml").write_text("depths: [2]\nnum_heads: [6]\n")
    m = U.GyreHipUpscalerLoader.hat(str(m_dir), torch_dtype=torch.float16)
    assert isinstance(m, U.GyreHipHAT) and m.config.depths == [2] and m.config.embed_dim == 180 and m.dtype == torch.float16
    assert m._scale == 4 and m._window_size == 16 and not m.training
    assert all(torch.equal(v, params[k].half()) for k, v in m.state_dict().items() if k in params)
    with pytest.raises(RuntimeError):                                            # the buffers are part of the strict key set
        U.GyreHipHAT(cfg).load_state_dict(params)
    lcfg = gcfg.hat_config(**{**gcfg.HAT_DEFAULTS["hat-l"], "depths": [1, 1], "num_heads": [6, 6]})
    lsd = weights.synthetic_state_dict(weights.hat_param_shapes(lcfg))
    lsd = {k: (v.long() if weights.hat_is_buffer(k) else v) for k, v in lsd.items()}
    torch.save({"params_ema": lsd, "params": {}}, str(l_dir / "net.pth"))
    (l_dir / "config.yaml").write_text("depths: [1, 1]\nnum_heads: [6, 6]\n")
    m = U.GyreHipUpscalerLoader.hat_l(str(l_dir))
    assert m.config.embed_dim == 180 and m.config.depths == [1, 1] and m.dtype == torch.float32
    assert all(torch.equal(v, lsd[k]) for k, v in m.state_dict().items())
    assert len(U.GyreHipUpscalerLoader.load(str(l_dir), network="hat", config="hat-l").config.depths) == 2
    (l_dir / "config.yaml").write_text("depths: [1, 1]\nnum_heads: [6, 6]\nupsampler: nearest+conv\n")
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.hat_l(str(l_dir))
    os.remove(l_dir / "config.yaml")                                             # no yaml: the default table alone (12 RHAGs) meets a 2-RHAG file
    with pytest.raises(RuntimeError):
        U.GyreHipUpscalerLoader.hat_l(str(l_dir))


def test_stored_reference_outputs_equal_the_restated_net():
    """tests/golden/hat_vectors.npz holds what the reference's own hat_arch.py computed (tests/golden/make_hat_golden.py); hat_ref.net
    restates it with the same fp32 operations in the same order.  Equal bit for bit where they were made; on another machine's torch
    build the kernels may sum in another order, so the gate there is the fp32 tolerance of tests/test_oracle_model_golden.py (rel-L2
    1e-4)."""
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == ["tiny2_1x3x32x48", "tiny_1x3x16x32"] and os.path.getsize(GOLDEN) < 256 * 1024
    for key in gold.files:
        name, dims = key.split("_")
        shape = tuple(int(v) for v in dims.split("x"))
        cfg, sd, x = R.model_case(name)
        if shape != R.MODEL_CASES[name][1]:
            x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
        got, want = R.net(sd, cfg, x), torch.from_numpy(gold[key])
        d = R.rel_l2(got, want)
        print(f"[hat] golden {key}: rel-L2 {d:.3e}, bit-equal {torch.equal(got, want)}")
        assert got.shape == want.shape and d < 1e-4


def test_export_names():
    names = ["gyre_hat_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    names += ["gyre_op_hat_attn", "gyre_op_chan_pool", "gyre_op_chan_pool_workspace", "gyre_op_chan_gate", "gyre_op_scale_add",
              "gyre_op_pixel_shuffle2"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
