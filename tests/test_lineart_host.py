"""Host-side tests of the line-art hinter (no GPU): the stored outputs of the reference's own module against the restated net, the
configuration and its refusals, the module shell, the exported names, and the pipeline's host steps."""
import os

import numpy as np
import pytest
import torch

import lineart_ref as R
from gyre_amd import _lib, config as gcfg, hinters as HN, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lineart_vectors.npz")


def test_stored_reference_outputs_equal_the_restated_net():
    """tests/golden/lineart_vectors.npz holds what the reference's own DrawingGenerator computed (make_lineart_golden.py); the fp32
    rel-L2 gate of tests/test_hat_host.py"""
    stored = np.load(GOLDEN)
    assert set(stored.files) == {"tiny", "odd"} and os.path.getsize(GOLDEN) < 256 * 1024
    for name in stored.files:
        cfg, sd, x = R.model_case(name)
        got, want = R.net(sd, cfg, x), torch.from_numpy(stored[name])
        d = R.rel_l2(got, want)
        print(f"[lineart] golden {name}: rel-L2 {d:.3e}")
        assert got.shape == want.shape and d < 1e-4


def test_output_size_rule():
    assert [R.out_size(h) for h in (5, 6, 8, 9, 12, 13, 18, 512)] == [8, 8, 8, 12, 12, 16, 20, 512]
    m = HN.GyreHipDrawingGenerator(3, 1, 1)
    assert m.out_shape((2, 3, 13, 18)) == (2, 1, 16, 20) and m.out_shape((1, 3, 512, 512)) == (1, 1, 512, 512)


@pytest.mark.parametrize("args,kw", [((1, 1), {}), ((3, 3), {}), ((4, 1), {}), ((3, 1, 0), {}), ((3, 1, 17), {}),
                                     ((3, 1), dict(num_block=6)), ((3, 1), dict(norm="batch"))])
def test_config_refusals(args, kw):
    with pytest.raises(NotImplementedError):
        gcfg.lineart_config(*args, **kw)
    with pytest.raises(NotImplementedError):
        HN.GyreHipDrawingGenerator(*args, **kw)


def test_config_defaults_and_param_shapes():
    cfg = gcfg.lineart_config(3, 1)
    assert dict(cfg) == dict(input_nc=3, output_nc=1, n_residual_blocks=9, sigmoid=True) and cfg.n_residual_blocks == 9
    shapes = weights.lineart_param_shapes(gcfg.lineart_config(3, 1, 3))
    assert list(shapes)[:4] == ["model0.1.weight", "model0.1.bias", "model1.0.weight", "model1.0.bias"] and len(shapes) == 24
    assert shapes["model0.1.weight"] == (64, 3, 7, 7) and shapes["model2.2.conv_block.5.weight"] == (256, 256, 3, 3)
    assert shapes["model3.0.weight"] == (256, 128, 3, 3) and shapes["model3.0.bias"] == (128,)      # ConvTranspose2d: [Cin, Cout, 3, 3]
    assert shapes["model3.3.weight"] == (128, 64, 3, 3) and shapes["model4.1.weight"] == (1, 64, 7, 7)
    assert list(shapes)[-2:] == ["model4.1.weight", "model4.1.bias"]


def test_model_shell():
    cfg, sd, x = R.model_case("tiny")
    m = HN.GyreHipDrawingGenerator(3, 1, 1, False)
    assert list(m.state_dict()) == list(weights.lineart_param_shapes(cfg))
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "model3.3.bias"}, strict=True)
    with pytest.raises(_lib.GyreError):                            # no CPU fallback
        m(x)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 4, 8))
    assert m.to(torch.float16).dtype == torch.float16 and m._kind == "lineart"


class _HostModule(torch.nn.Module):
    """a stand-in generator: one parameter (device and dtype), the mean of the three channels shifted out of [0, 1] on both sides"""

    def __init__(self, dtype):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=dtype), requires_grad=False)
        self.seen = None

    def forward(self, x, cond=None):
        self.seen = x
        return x.mean(1, keepdim=True) * 2 * self.w - 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pipeline_host_semantics(dtype):
    mod = _HostModule(torch.float32)
    pipe = HN.GyreInformativeDrawingPipeline(mod)
    assert pipe.pipeline_modules() == [("module", mod)] and pipe.to("cpu") is None
    g = torch.Generator().manual_seed(1)
    for x, want3 in ((torch.rand((2, 1, 6, 7), generator=g), lambda t: t[:, [0, 0, 0]]),
                     (torch.rand((2, 2, 6, 7), generator=g), lambda t: t[:, [0, 0, 0]]),
                     (torch.rand((1, 3, 6, 7), generator=g), lambda t: t),
                     (torch.rand((1, 5, 6, 7), generator=g), lambda t: t[:, :3]),
                     (torch.rand((3, 6, 7), generator=g), lambda t: t[None])):
        x = x.to(dtype)
        got = pipe(x)
        x3 = want3(x)
        assert torch.equal(mod.seen, x3.to(torch.float32)) and mod.seen.dtype == torch.float32      # the module's own dtype
        want = (1 - (x3.to(torch.float32).mean(1, keepdim=True) * 2 - 0.5).clamp(0, 1)).to(dtype)
        assert got.dtype == dtype and torch.equal(got, want)
        assert float(got.min()) >= 0 and float(got.max()) <= 1 and float(got.min()) == 0.0 and float(got.max()) == 1.0


def test_export_names():
    names = ["gyre_lineart_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    names += ["gyre_op_inorm_workspace", "gyre_op_inorm_stats", "gyre_op_inorm_apply", "gyre_op_tconv_compose", "gyre_op_conv7_in",
              "gyre_op_conv7_out", "gyre_op_conv3x3_valid"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
