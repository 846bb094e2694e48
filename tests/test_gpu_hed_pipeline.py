"""The HED pipeline on the GPU (-m gpu; gyre_amd.hinters.GyreHedPipeline over the native detector) against tests/hed_ref.py's pipeline:
1-, 3- and 4-channel and [C, H, W] host inputs come back on the host in their dtype; the loader from a safetensors file and a folder.

Two references.  hed_ref.pipeline over the SAME native module has the same host steps on the same six maps: equal bits.  hed_ref.pipeline
over the fp64 net is the yardstick: with e the model gate of the fused map (twice EMULATION, max-abs) and R = max - min of the fp64 fused
map of a sample, r = (v - min) / R moves by at most (|dv| + |dmin|) / R + r (|dmax| + |dmin|) / R <= 4 e / R to first order; the assertion
takes 4 e / (R - 2 e)."""
import os

import pytest
import torch

import hed_ref as R
from gyre_amd.hinters import GyreHedPipeline, GyreHipHED, load_hed
from gpu_util import DEV
from test_hed_ref_host import EMULATION

pytestmark = pytest.mark.gpu
CASE = "16x16"


class _Fp64Net(torch.nn.Module):
    """hed_ref.net in fp64 as a module: one parameter names its device and dtype"""

    def __init__(self, sd):
        super().__init__()
        self.sd = sd
        self.w = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64), requires_grad=False)

    def forward(self, x):
        return R.net(self.sd, x, compute=torch.float64)


@pytest.fixture(scope="module")
def pipe():
    m = GyreHipHED()
    m.load_state_dict(R.model_weights())
    p = GyreHedPipeline(m.to(torch.float16))
    p.to(DEV)
    assert p.pipeline_modules() == [("module", p.module)] and next(p.module.parameters()).is_cuda
    return p


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_pipeline_on_host_images(pipe, channels):
    H, W = R.MODEL_CASES[CASE]
    x = torch.rand((2, channels, H, W), generator=torch.Generator().manual_seed(channels))
    got = pipe(x)
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (2, 1, H, W)
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert torch.equal(got, R.pipeline(pipe.module, x))               # the same host steps over the same module
    want = R.pipeline(_Fp64Net(R.model_weights()), x.double())
    fused = R.net(R.model_weights(), _bgr255(x), compute=torch.float64)[-1]
    spread = (fused.amax((1, 2, 3)) - fused.amin((1, 2, 3))).min()
    e = 2 * EMULATION[(CASE, torch.float16)][0][5]
    bound = 4 * e / (float(spread) - 2 * e)
    d = R.max_abs(got, want)
    print(f"[hed] pipeline {channels} channels: max-abs against the fp64 pipeline {d:.3e} (bound {bound:.3e}, fused spread {float(spread):.3f})")
    assert d <= bound
    assert torch.equal(pipe(x[0]), got[:1])                           # [C, H, W] gains its batch axis
    xh = x.to(torch.float16)
    assert pipe(xh).dtype == torch.float16 and pipe(x.to(DEV)).device.type == "cuda"


def _bgr255(x):
    x3 = x[:, [0, 1, 2]] if x.shape[1] >= 3 else x[:, [0, 0, 0]]
    return ((x3.double() - torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)[None, :, None, None])[:, [2, 1, 0]]) * 255


def test_load_hed_from_a_file_and_a_folder(pipe, tmp_path):
    from safetensors.torch import save_file
    sd = {k: v.contiguous() for k, v in R.model_weights().items()}
    file = os.path.join(tmp_path, "network-bsds500.safetensors")
    save_file(sd, file)
    x = R.model_input("5x7").to(DEV)
    want = [g.cpu() for g in pipe.module(x)]
    for path in (file, str(tmp_path)):
        m = load_hed(path, torch_dtype=torch.float16).to(DEV)
        assert all(torch.equal(R.bits(a.cpu()), R.bits(b)) for a, b in zip(m(x), want)), path
    torch.save(sd, os.path.join(tmp_path, "other.pth"))
    with pytest.raises(FileNotFoundError):
        load_hed(str(tmp_path))                                        # two model files: the caller has to choose
    m = load_hed(str(tmp_path), allow_patterns="*.pth")
    assert m.dtype == torch.float32 and torch.equal(m.state_dict()["conv5_3.weight"], sd["conv5_3.weight"])
