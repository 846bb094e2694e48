"""Host-side tests of the MLSD line detector (no GPU): the parameter shapes and key set, the module shell with its buffers, strict load
and refusals, the loader's file selection, the exported names, and the pipeline - decode and rasteriser against an independent numpy
restatement (tests/mlsd_ref.py) on synthetic maps: a plateau tie, a segment leaving the image, top_k below the number of maxima - and
its host steps on a stand-in module."""
import os

import numpy as np
import pytest
import torch

import mlsd_ref as R
from gyre_amd import _lib, config as gcfg, hinters as HN, weights


def test_param_shapes_and_key_set():
    shapes = weights.mlsd_param_shapes()
    assert len(shapes) == 362 and shapes == weights.mlsd_param_shapes(gcfg.mlsd_config())
    stored = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlsd_vectors.npz"))
    assert stored["keys"].tolist() == list(shapes)                   # the reference's own state_dict() order
    assert list(shapes)[:6] == ["backbone.features.0.0.weight"] + ["backbone.features.0.1." + n for n in
                                                                     ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert list(shapes)[-2:] == ["block23.conv3.weight", "block23.conv3.bias"]
    assert shapes["backbone.features.0.0.weight"] == (32, 4, 3, 3) and "backbone.features.0.0.bias" not in shapes
    assert shapes["backbone.features.1.conv.0.0.weight"] == (32, 1, 3, 3) and shapes["backbone.features.1.conv.1.weight"] == (16, 32, 1, 1)
    assert shapes["backbone.features.2.conv.0.0.weight"] == (96, 16, 1, 1) and shapes["backbone.features.2.conv.1.0.weight"] == (96, 1, 3, 3)
    assert shapes["backbone.features.13.conv.2.weight"] == (96, 576, 1, 1) and shapes["backbone.features.4.conv.1.1.running_var"] == (144,)
    assert shapes["block15.conv1.0.weight"] == (64, 96, 1, 1) and shapes["block21.conv2.0.weight"] == (64, 16, 1, 1)
    assert shapes["block16.conv1.0.weight"] == (128, 128, 3, 3) and shapes["block16.conv1.0.bias"] == (128,)
    assert shapes["block23.conv3.weight"] == (16, 64, 1, 1) and shapes["block23.conv1.1.num_batches_tracked"] == ()
    assert sum(k.endswith("num_batches_tracked") for k in shapes) == 57
    assert gcfg.MLSD_SETTING == R.SETTING
    assert all(gcfg.mlsd_size_ok(n) == R.size_ok(n) for n in range(0, 200))
    assert [n for n in range(40) if gcfg.mlsd_size_ok(n)] == [16, 17, 32, 33]
    with pytest.raises(NotImplementedError):
        gcfg.mlsd_config(pretrained=True)
    with pytest.raises(NotImplementedError):
        HN.GyreHipMLSD(input_nc=4)


def test_model_shell():
    sd = R.model_weights()
    m = HN.GyreHipMLSD()
    assert list(m.state_dict()) == list(weights.mlsd_param_shapes()) and m._kind == "mlsd"
    assert len(list(m.parameters())) == 362 - 3 * 57                 # the BatchNorm statistics and counters are buffers, as in the reference
    assert m.state_dict()["block23.conv1.1.num_batches_tracked"].dtype == torch.long
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "block23.conv3.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({**sd, "backbone.features.14.conv.0.0.weight": torch.zeros(576, 96, 1, 1)}, strict=True)
    assert m.out_shape((2, 4, 17, 49)) == (2, 9, 8, 24) and m.out_shape((1, 4, 512, 512)) == (1, 9, 256, 256)
    with pytest.raises(_lib.GyreError):                            # no CPU fallback
        m(torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(4, 16, 16))
    for H, W in ((15, 16), (16, 18), (20, 16), (16, 34), (8, 8)):    # a size rule refusal comes before any device work
        with pytest.raises(ValueError):
            m(torch.zeros(1, 4, H, W))
    h = m.to(torch.float16)
    assert h.dtype == torch.float16 and h.state_dict()["block23.conv1.1.num_batches_tracked"].dtype == torch.long
    c = m._c_cfg()
    assert isinstance(c, _lib.MlsdCfg) and c.reserved == 0


def test_loader_file_selection(tmp_path):
    sd = R.model_weights()
    with pytest.raises(FileNotFoundError):
        HN.load_mlsd(str(tmp_path))
    torch.save(sd, os.path.join(tmp_path, "mlsd_large_512_fp32.pth"))
    m = HN.load_mlsd(str(tmp_path))
    assert isinstance(m, HN.GyreHipMLSD) and not m.training and m.dtype == torch.float32
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    assert HN.load_mlsd(os.path.join(tmp_path, "mlsd_large_512_fp32.pth"), torch_dtype=torch.float16).dtype == torch.float16
    torch.save(sd, os.path.join(tmp_path, "other.pth"))
    with pytest.raises(FileNotFoundError):
        HN.load_mlsd(str(tmp_path))
    assert HN.load_mlsd(str(tmp_path), allow_patterns="mlsd_*").dtype == torch.float32
    assert HN.load_mlsd(str(tmp_path), ignore_patterns=["other*"]).dtype == torch.float32
    torch.save({k: v for k, v in sd.items() if k != "block15.conv1.1.running_var"}, os.path.join(tmp_path, "short.pt"))
    with pytest.raises(RuntimeError):                              # the load is strict
        HN.load_mlsd(os.path.join(tmp_path, "short.pt"))


def test_export_names():
    names = ["gyre_mlsd_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    names += ["gyre_op_mlsd_fold", "gyre_op_mlsd_entry", "gyre_op_dwconv3", "gyre_op_upsample2_ac", "gyre_op_dconv3_d5", "gyre_op_mlsd_act",
              "gyre_op_mlsd_relu_add", "gyre_op_mlsd_exit"]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gyre_hip.h")).read()
    assert all(n + "(" in header for n in names)
    assert [f[0] for f in _lib.MlsdFoldArgs._fields_][-6:] == ["kind", "O", "I", "taps", "o_pad", "i_pad"]


# ---------------------------------------------------------------------------------------------------------------------------- pipeline
def _synthetic_map(h=16, w=16):
    """tp [2, 9, h, w]: a quiet background (logit -6) with isolated maxima of distinct heights, a two-pixel plateau (a tie: both are
    maxima, equal scores, index order), a centre whose segment leaves the image, and one whose segment is too short"""
    tp = torch.zeros((2, 9, h, w))
    tp[:, 0] = -6.0
    g = torch.Generator().manual_seed(5)
    tp[:, 1:5] = torch.randn((2, 4, h, w), generator=g) * 0.2
    peaks = [(2, 3, 2.0), (5, 9, 1.5), (9, 4, 1.0), (12, 12, 0.5), (7, 13, 0.25), (14, 2, -0.5)]
    for y, x, v in peaks:
        tp[0, 0, y, x] = v
        tp[0, 1:5, y, x] = torch.tensor([-3.3 + 0.1 * y, -1.2, 2.6, 1.9 - 0.1 * x])
    tp[0, 0, 10, 8] = tp[0, 0, 10, 9] = 0.75                        # the plateau
    tp[0, 1:5, 10, 8] = torch.tensor([-2.1, 0.3, 1.7, -0.4])
    tp[0, 1:5, 10, 9] = torch.tensor([-1.1, 2.3, 0.7, -2.4])
    tp[0, 1:5, 2, 3] = torch.tensor([-9.4, -6.3, 4.2, 1.1])         # leaves the image on the left and top
    tp[0, 1:5, 12, 12] = torch.tensor([0.01, 0.02, 0.03, 0.01])     # shorter than the distance threshold
    tp[1, 0, 4, 4], tp[1, 0, 11, 6] = 3.0, -1.0                     # the second sample: one strong, one below a 0.3 threshold
    tp[1, 1:5, 4, 4] = torch.tensor([-2.2, -2.7, 3.1, 2.4])
    return tp


@pytest.mark.parametrize("size", [(32, 32), (45, 70)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("top_k", [200, 4])
def test_decode_and_rasteriser_against_numpy(size, top_k):
    tp = _synthetic_map()
    H, W = size
    for thr in (0.1, 0.3):
        got = HN.mlsd_decode(tp, (H, W), 32, thr, 0.1, top_k)
        want = R.decode_np(tp.numpy(), (H, W), 32, thr, 0.1, top_k)
        assert len(got) == len(want) == 2
        for b in range(2):
            assert got[b].dtype == torch.float32 and tuple(got[b].shape) == want[b].shape
            np.testing.assert_allclose(got[b].numpy(), want[b], rtol=1e-6, atol=1e-6)
            img = HN.mlsd_rasterise(got[b], H, W)
            assert np.array_equal(img.numpy(), R.rasterise_np(want[b], H, W))
            assert set(np.unique(img.numpy()).tolist()) <= {0.0, 1.0}
    full = HN.mlsd_decode(tp, (H, W), 32, 0.1, 0.1, 200)[0]
    # 8 maxima in sample 0; the too-short one is dropped; the plateau's two pixels are both kept, lower index first
    assert full.shape[0] == 7 and bool((full[:-1, 4] >= full[1:, 4]).all())
    tie = (full[:, 4] == torch.sigmoid(torch.tensor(0.75))).nonzero().flatten().tolist()
    assert len(tie) == 2 and tie[1] == tie[0] + 1
    sx = W / 32
    assert abs(float(full[tie[0], 0]) - (8 - 2.1) * 2 * sx) < 1e-4 and abs(float(full[tie[1], 0]) - (9 - 1.1) * 2 * sx) < 1e-4
    assert float(full[0, 0]) < 0 and float(full[0, 1]) < 0           # the strongest segment starts outside the image ...
    assert HN.mlsd_rasterise(full[:1], H, W).sum() > 0               # ... and its inside part is drawn
    few = HN.mlsd_decode(tp, (H, W), 32, 0.1, 0.1, 4)[0]             # top_k below the number of maxima: the four strongest, the plateau's first
    assert few.shape[0] == 4 and torch.equal(few, full[:4])


def test_rasteriser_rounds_half_to_even_and_handles_no_lines():
    assert float(HN.mlsd_rasterise(torch.zeros((0, 5)), 4, 4).sum()) == 0
    img = HN.mlsd_rasterise(torch.tensor([[0.5, 1.5, 2.5, 1.5, 1.0]]), 4, 4)     # round(0.5) = 0, round(2.5) = 2, round(1.5) = 2: three points
    want = np.zeros((4, 4), dtype=np.float32)
    want[2, 0] = want[2, 2] = 1
    want[2, 2] = 1
    mid = int(np.rint(np.float32(0.5) + np.float32(2.0) * (np.float32(1) / np.float32(2))))
    want[2, mid] = 1
    assert np.array_equal(img.numpy(), want) and np.array_equal(want, R.rasterise_np(np.array([[0.5, 1.5, 2.5, 1.5]]), 4, 4))
    one = HN.mlsd_rasterise(torch.tensor([[1.2, 2.9, 1.4, 3.1, 1.0]]), 4, 4)      # both ends round to one pixel: one point, the start
    assert float(one.sum()) == 1 and float(one[3, 1]) == 1


class _HostModule(torch.nn.Module):
    """a stand-in detector: one parameter (device and dtype); returns a fixed synthetic map and remembers what it was fed"""

    def __init__(self, dtype, tp):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1, dtype=dtype), requires_grad=False)
        self.tp, self.seen = tp, None

    def forward(self, x):
        self.seen = x
        return self.tp[:x.shape[0]].to(x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pipeline_host_semantics(dtype):
    tp = _synthetic_map()
    mod = _HostModule(torch.float32, tp)
    pipe = HN.GyreMlsdPipeline(mod, input_size=32)
    assert pipe.pipeline_modules() == [("module", mod)] and pipe.to("cpu") is None
    g = torch.Generator().manual_seed(1)
    for x, want3 in ((torch.rand((2, 1, 32, 32), generator=g), lambda t: t[:, [0, 0, 0]]),
                     (torch.rand((1, 3, 32, 32), generator=g), lambda t: t),
                     (torch.rand((2, 5, 45, 70), generator=g), lambda t: t[:, :3]),
                     (torch.rand((3, 20, 24), generator=g), lambda t: t[None])):
        x = x.to(dtype)
        got = pipe(x)
        rgb = want3(x).to(torch.float32)
        H, W = rgb.shape[2:]
        if (H, W) != (32, 32):
            rgb = torch.nn.functional.interpolate(rgb, size=(32, 32), mode="bilinear", antialias=True, align_corners=False)
        fed = torch.cat([2 * rgb - 1, torch.full_like(rgb[:, :1], 1 / 127.5 - 1)], 1)
        assert torch.equal(mod.seen, fed) and mod.seen.dtype == torch.float32 and mod.seen.shape[1:] == (4, 32, 32)
        B = rgb.shape[0]
        lines = R.decode_np(tp[:B].numpy(), (H, W), 32)
        want = np.stack([R.rasterise_np(l, H, W) for l in lines])[:, None]
        assert got.dtype == dtype and got.shape == (B, 1, H, W) and np.array_equal(got.to(torch.float32).numpy(), want)
        segs = pipe.lines(x)
        assert len(segs) == B and all(s.dtype == torch.float32 and s.shape[1] == 5 for s in segs)
    with pytest.raises(ValueError):
        HN.GyreMlsdPipeline(mod, input_size=100)
    with pytest.raises(ValueError):
        HN.GyreMlsdPipeline(mod, top_k=0)
