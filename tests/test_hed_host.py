"""Host-side tests of the HED edge detector (no GPU): the parameter shapes, the module shell and its refusals, the loader's file
selection, the exported names, and the pipeline's host steps on a stand-in module."""
import os

import pytest
import torch

import hed_ref as R
from gyre_amd import _lib, config as gcfg, hinters as HN, weights


def test_param_shapes():
    shapes = weights.hed_param_shapes()
    assert len(shapes) == 38 and shapes == weights.hed_param_shapes(gcfg.hed_config())
    assert list(shapes)[:4] == ["conv1_1.weight", "conv1_1.bias", "conv1_2.weight", "conv1_2.bias"]
    assert list(shapes)[24:28] == ["conv5_3.weight", "conv5_3.bias", "score_dsn1.weight", "score_dsn1.bias"]
    assert list(shapes)[-2:] == ["score_final.weight", "score_final.bias"]
    assert shapes["conv1_1.weight"] == (64, 3, 3, 3) and shapes["conv3_1.weight"] == (256, 128, 3, 3) and shapes["conv5_1.weight"] == (512, 512, 3, 3)
    assert shapes["score_dsn4.weight"] == (1, 512, 1, 1) and shapes["score_dsn4.bias"] == (1,) and shapes["score_final.weight"] == (1, 5, 1, 1)
    assert not any("deconv" in k for k in shapes)                  # the bilinear buffers are not persistent
    assert gcfg.HED_STAGES == R.STAGES and gcfg.HED_BORDER == R.BORDER
    with pytest.raises(NotImplementedError):
        gcfg.hed_config(n_residual_blocks=3)
    with pytest.raises(NotImplementedError):
        HN.GyreHipHED(input_nc=3)


def test_model_shell():
    sd = R.model_weights()
    m = HN.GyreHipHED()
    assert list(m.state_dict()) == list(weights.hed_param_shapes()) and m._kind == "hed"
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "score_final.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "weight_deconv2": torch.zeros(1, 1, 4, 4)}, strict=True)
    assert m.out_shape((2, 3, 5, 7)) == (12, 1, 5, 7) and m.out_shape((1, 3, 1, 1)) == (6, 1, 1, 1)
    with pytest.raises(_lib.GyreError):                            # no CPU fallback
        m(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(3, 8, 8))
    assert m.to(torch.float16).dtype == torch.float16
    c = m._c_cfg()
    assert isinstance(c, _lib.HedCfg) and c.reserved == 0


def test_loader_file_selection(tmp_path):
    sd = R.model_weights()
    with pytest.raises(FileNotFoundError):
        HN.load_hed(str(tmp_path))
    torch.save(sd, os.path.join(tmp_path, "network-bsds500.pth"))
    m = HN.load_hed(str(tmp_path))
    assert isinstance(m, HN.GyreHipHED) and not m.training and m.dtype == torch.float32
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert HN.load_hed(os.path.join(tmp_path, "network-bsds500.pth"), torch_dtype=torch.float16).dtype == torch.float16
    torch.save(sd, os.path.join(tmp_path, "table5_pidinet.pth"))
    with pytest.raises(FileNotFoundError):
        HN.load_hed(str(tmp_path))
    assert HN.load_hed(str(tmp_path), allow_patterns="network-*").dtype == torch.float32
    assert HN.load_hed(str(tmp_path), ignore_patterns=["table5*"]).dtype == torch.float32
    torch.save({k: v for k, v in sd.items() if k != "conv2_2.bias"}, os.path.join(tmp_path, "short.pt"))
    with pytest.raises(RuntimeError):                              # the load is strict
        HN.load_hed(os.path.join(tmp_path, "short.pt"))


class _HostModule(torch.nn.Module):
    """a stand-in detector: one parameter (device and dtype); six maps of which the last is a ramp of the blue channel it was fed"""

    def __init__(self, dtype):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=dtype), requires_grad=False)
        self.seen = None

    def forward(self, x):
        self.seen = x
        return [x[:, :1] * 0] * 5 + [torch.sigmoid(x[:, :1] * self.w / 64)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pipeline_host_semantics(dtype):
    mod = _HostModule(torch.float32)
    pipe = HN.GyreHedPipeline(mod)
    assert pipe.pipeline_modules() == [("module", mod)] and pipe.to("cpu") is None
    g = torch.Generator().manual_seed(1)
    mean = torch.tensor([0.485, 0.456, 0.406])[None, :, None, None]
    for x, want3 in ((torch.rand((2, 1, 6, 7), generator=g), lambda t: t[:, [0, 0, 0]]),
                     (torch.rand((2, 2, 6, 7), generator=g), lambda t: t[:, [0, 0, 0]]),
                     (torch.rand((1, 3, 6, 7), generator=g), lambda t: t),
                     (torch.rand((1, 5, 6, 7), generator=g), lambda t: t[:, :3]),
                     (torch.rand((3, 6, 7), generator=g), lambda t: t[None])):
        x = x.to(dtype)
        got = pipe(x)
        fed = (want3(x).to(torch.float32) - mean)[:, [2, 1, 0]] * 255           # the module's own dtype; mean off RGB, then BGR x 255
        assert torch.equal(mod.seen, fed) and mod.seen.dtype == torch.float32
        v = torch.sigmoid(fed[:, :1] / 64)
        lo, hi = v.amin((1, 2, 3), keepdim=True), v.amax((1, 2, 3), keepdim=True)
        assert got.dtype == dtype and torch.equal(got, ((v - lo) / (hi - lo)).to(dtype))
        assert torch.equal(got, R.pipeline(mod, x))
        assert all(float(s.min()) == 0.0 and float(s.max()) == 1.0 for s in got)       # per sample, not per batch
    flat = pipe(torch.full((1, 3, 4, 4), 0.5))                       # a constant map divides by zero, as in the reference
    assert bool(torch.isnan(flat).all())


def test_export_names():
    names = ["gyre_hed_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward",
                                       "geometry")]
    names += ["gyre_op_hed_entry", "gyre_op_hed_tail", "gyre_op_hed_fuse"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gyre_hip.h")).read()
    assert all(n + "(" in header for n in names)
    a = _lib.HedFuseArgs()
    assert len(a.so) == 5 and len(a.ox) == 5
