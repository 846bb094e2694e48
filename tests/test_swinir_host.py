"""Host side of the SwinIR upscaler (gyre_amd.config / weights / upscaler), no GPU: configuration refusals, the module shell and its
buffers, loader round trips, the stored outputs of the reference's own SwinIR against tests/swinir_ref.py, the ABI exports."""
import math
import os

import numpy as np
import pytest
import torch

import swinir_ref as R
from gyre_amd import _lib, config as gcfg, upscaler as U, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swinir_vectors.npz")


def test_default_tables_and_entry_points():
    assert U.DEFAULT_CONFIGS["swinir"] == gcfg.SWINIR_DEFAULTS["swinir"] and U.DEFAULT_CONFIGS["swinir-l"] == gcfg.SWINIR_DEFAULTS["swinir-l"]
    s, l = gcfg.SWINIR_DEFAULTS["swinir"], gcfg.SWINIR_DEFAULTS["swinir-l"]
    assert (s["embed_dim"], s["num_heads"], s["depths"], s["resi_connection"]) == (180, [6] * 6, [6] * 6, "1conv")
    assert (l["embed_dim"], l["num_heads"], l["depths"], l["resi_connection"]) == (240, [8] * 9, [6] * 9, "3conv")
    for t in (s, l):
        assert (t["window_size"], t["mlp_ratio"], t["upsampler"], t["upscale"], t["img_size"], t["img_range"]) == (8, 2, "nearest+conv", 4, 64, 1.0)
    assert U.ENTRY_POINTS["swinir"] == dict(network="swinir") and U.ENTRY_POINTS["swinir_l"] == dict(network="swinir", config="swinir-l")
    gcfg.swinir_config(**s), gcfg.swinir_config(**l)


@pytest.mark.parametrize("kw", [dict(window_size=7), dict(upsampler="pixelshuffle"), dict(upsampler="pixelshuffledirect"), dict(upsampler=""),
                                dict(upscale=3), dict(upscale=8), dict(embed_dim=96), dict(num_heads=[2, 4], embed_dim=60),
                                dict(embed_dim=270, num_heads=[9, 9]), dict(mlp_ratio=2.05), dict(ape=True), dict(patch_norm=False),
                                dict(qkv_bias=False), dict(in_chans=1), dict(resi_connection="2conv"), dict(depths=[2]), dict(img_size=8),
                                dict(num_block=2), dict(scale=4), dict(qk_scale=0.5)])
def test_config_refusals(kw):
    with pytest.raises(NotImplementedError):
        gcfg.tiny_swinir(**kw)


def test_constructor_defaults_are_outside_the_built_list():
    with pytest.raises(NotImplementedError):
        gcfg.swinir_config()                                                     # SwinIR(): window 7, no upsampler


def test_model_shell_and_buffers():
    m = U.GyreHipSwinIR(gcfg.tiny_swinir())
    shapes = weights.swinir_param_shapes(m.config)
    sd = m.state_dict()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert m._scale == 4 and m._window_size == 8 and m.out_shape((2, 3, 16, 24)) == (2, 3, 64, 96)
    assert sd["layers.0.residual_group.blocks.0.attn.relative_position_index"].shape == (64, 64)
    assert sd["layers.1.residual_group.blocks.1.attn_mask"].shape == (4, 64, 64)                 # (16 / 8)^2 windows
    assert "layers.0.residual_group.blocks.0.attn_mask" not in sd
    params = dict(m.named_parameters())
    assert not any(weights.swinir_is_buffer(k) for k in params) and len(params) + 6 == len(sd)
    big = weights.swinir_param_shapes(gcfg.swinir_config(**gcfg.SWINIR_DEFAULTS["swinir"]))
    assert big["layers.5.residual_group.blocks.5.attn_mask"] == (64, 64, 64) and big["conv_first.weight"] == (180, 3, 3, 3)
    n = sum(math.prod(s) for k, s in big.items() if not weights.swinir_is_buffer(k))
    assert n == 11_715_559                                                       # SwinIR-M real-world x4 (nearest+conv): 11.7 M parameters
    l3 = weights.swinir_param_shapes(gcfg.swinir_config(**gcfg.SWINIR_DEFAULTS["swinir-l"]))
    assert l3["layers.8.conv.2.weight"] == (60, 60, 1, 1) and l3["conv_after_body.4.weight"] == (240, 60, 3, 3)
    with pytest.raises(_lib.GyreError):
        m(torch.rand(1, 3, 8, 8))                                                # CPU tensors: no fallback
    with pytest.raises(ValueError):
        m(torch.rand(1, 4, 8, 8))
    with pytest.raises(ValueError):
        m(torch.rand(1, 3, 3, 16))                                               # too short to reflect-pad to 8


def test_loader_round_trips(tmp_path):
    from safetensors.torch import save_file
    cfg = gcfg.swinir_config(**{**gcfg.SWINIR_DEFAULTS["swinir"], "depths": [2], "num_heads": [6]})
    shapes = weights.swinir_param_shapes(cfg)
    sd = weights.synthetic_state_dict(shapes)
    sd = {k: (torch.zeros(shapes[k], dtype=torch.long) if k.endswith("relative_position_index") else v) for k, v in sd.items()}
    params = {k: v for k, v in sd.items() if not weights.swinir_is_buffer(k)}
    m_dir, l_dir, ema_dir = tmp_path / "m", tmp_path / "l", tmp_path / "ema"
    for d in (m_dir, l_dir, ema_dir):
        os.makedirs(d)
    save_file(sd, str(m_dir / "model.safetensors"))                              # a full checkpoint, buffers present: strict load
    (m_dir / "config.yaml").write_text("depths: [2]\nnum_heads: [6]\n")
    m = U.GyreHipUpscalerLoader.swinir(str(m_dir), torch_dtype=torch.float16)
    assert isinstance(m, U.GyreHipSwinIR) and m.config.depths == [2] and m.config.embed_dim == 180 and m.dtype == torch.float16
    assert m._scale == 4 and m._window_size == 8 and not m.training
    assert all(torch.equal(v, params[k].half()) for k, v in m.state_dict().items() if k in params)
    with pytest.raises(RuntimeError):                                            # the buffers are part of the strict key set
        U.GyreHipSwinIR(cfg).load_state_dict(params)
    lcfg = gcfg.swinir_config(**{**gcfg.SWINIR_DEFAULTS["swinir-l"], "depths": [2, 2], "num_heads": [8, 8]})
    lsd = weights.synthetic_state_dict(weights.swinir_param_shapes(lcfg))
    lsd = {k: (v.long() if k.endswith("relative_position_index") else v) for k, v in lsd.items()}
    torch.save({"params_ema": lsd, "params": {}}, str(l_dir / "net.pth"))
    (l_dir / "config.yaml").write_text("depths: [2, 2]\nnum_heads: [8, 8]\n")
    m = U.GyreHipUpscalerLoader.swinir_l(str(l_dir))
    assert m.config.embed_dim == 240 and m.config.resi_connection == "3conv" and m.config.depths == [2, 2]
    assert all(torch.equal(v, lsd[k]) for k, v in m.state_dict().items())
    (l_dir / "config.yaml").write_text("depths: [2, 2]\nnum_heads: [8, 8]\nupsampler: pixelshuffle\n")
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.swinir_l(str(l_dir))
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.hat(str(l_dir))
    with pytest.raises(NotImplementedError):
        U.GyreHipUpscalerLoader.hat_l(str(l_dir))


def test_stored_reference_outputs_equal_the_restated_net():
    """tests/golden/swinir_vectors.npz holds what the reference's own network_swinir.py computed (tests/golden/make_swinir_golden.py);
    swinir_ref.net restates it with the same fp32 operations in the same order.  Equal bit for bit where they were made; on another
    machine's torch build the kernels may sum in another order, so the gate there is the fp32 tolerance of
    tests/test_oracle_model_golden.py (rel-L2 1e-4)."""
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == ["tiny3_1x3x13x21", "tiny3_2x3x16x24", "tiny_1x3x13x21", "tiny_2x3x16x24"]
    for key in gold.files:
        name, dims = key.split("_")
        shape = tuple(int(v) for v in dims.split("x"))
        cfg, sd, x = R.model_case(name)
        if shape != R.MODEL_CASES[name][1]:
            x = torch.rand(shape, generator=torch.Generator().manual_seed(1))
        got, want = R.net(sd, cfg, x), torch.from_numpy(gold[key])
        d = R.rel_l2(got, want)
        print(f"[swinir] golden {key}: rel-L2 {d:.3e}, bit-equal {torch.equal(got, want)}")
        assert got.shape == want.shape and d < 1e-4


def test_export_names():
    names = ["gyre_swinir_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    names += ["gyre_op_win_attn", "gyre_op_win_bias", "gyre_op_ln_live", "gyre_op_swin_act", "gyre_op_swin_entry", "gyre_op_swin_exit"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
