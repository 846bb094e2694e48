"""The MLSD pipeline on the GPU (-m gpu; gyre_amd.hinters.GyreMlsdPipeline over the native detector) end to end at input_size 32 and
64, against the restated decode and rasteriser (tests/mlsd_ref.py, numpy) fed with the native module's own output: the segments, the
drawing, host inputs coming back on the host in their dtype; and the loader from a safetensors file and a folder."""
import os

import numpy as np
import pytest
import torch

import mlsd_ref as R
from gyre_amd.hinters import GyreHipMLSD, GyreMlsdPipeline, load_mlsd
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def module():
    m = GyreHipMLSD()
    m.load_state_dict(R.model_weights())
    return m.to(torch.float16).to(DEV)


@pytest.mark.parametrize("input_size,size", [(32, (32, 32)), (64, (64, 64)), (64, (45, 70))], ids=["32", "64", "64-from-45x70"])
def test_pipeline_end_to_end(module, input_size, size):
    # the seeded weights give centre logits near 0 (scores near 0.5) and short offsets: thresholds that keep some and drop some
    pipe = GyreMlsdPipeline(module, input_size=input_size, score_threshold=0.5, distance_threshold=0.05, top_k=50)
    assert pipe.pipeline_modules() == [("module", module)]
    H, W = size
    x = torch.rand((2, 3, H, W), generator=torch.Generator().manual_seed(input_size + H))
    got, lines = pipe(x), pipe.lines(x)
    assert got.device.type == "cpu" and got.dtype == torch.float32 and tuple(got.shape) == (2, 1, H, W)
    # the module's own output on what the pipeline feeds it
    rgb = x.to(DEV)
    if (H, W) != (input_size, input_size):
        rgb = torch.nn.functional.interpolate(rgb, size=(input_size, input_size), mode="bilinear", antialias=True, align_corners=False)
    sample = torch.cat([2 * rgb - 1, torch.full_like(rgb[:, :1], 1 / 127.5 - 1)], 1).to(torch.float16)
    tp = module(sample).float().cpu()
    assert tuple(tp.shape) == (2, 9, input_size // 2, input_size // 2)
    want = R.decode_np(tp.numpy(), (H, W), input_size, 0.5, 0.05, 50)
    counts = [w.shape[0] for w in want]
    print(f"[mlsd] pipeline input_size {input_size} from {H}x{W}: {counts} segments, {int(got.sum())} pixels drawn")
    assert all(0 < c <= 50 for c in counts)
    for b in range(2):
        assert lines[b].dtype == torch.float32 and tuple(lines[b].shape) == want[b].shape
        np.testing.assert_allclose(lines[b].cpu().numpy(), want[b], rtol=1e-5, atol=1e-4)
        assert np.array_equal(got[b, 0].numpy(), R.rasterise_np(lines[b].cpu().numpy(), H, W))    # the drawing of the pipeline's own segments
    assert set(np.unique(got.numpy()).tolist()) == {0.0, 1.0}
    assert torch.equal(pipe(x[0]), got[:1])                            # [C, H, W] gains its batch axis
    assert pipe(x.to(torch.float16)).dtype == torch.float16 and pipe(x.to(DEV)).device.type == "cuda"


def test_load_mlsd_from_a_file_and_a_folder(module, tmp_path):
    from safetensors.torch import save_file
    sd = {k: v.contiguous() for k, v in R.model_weights().items()}
    file = os.path.join(tmp_path, "mlsd_large_512_fp32.safetensors")
    save_file(sd, file)
    x = R.model_input("16x16").to(DEV)
    want = module(x).cpu()
    for path in (file, str(tmp_path)):
        m = load_mlsd(path, torch_dtype=torch.float16).to(DEV)
        assert torch.equal(R.bits(m(x).cpu()), R.bits(want)), path
    torch.save(sd, os.path.join(tmp_path, "other.pth"))
    with pytest.raises(FileNotFoundError):
        load_mlsd(str(tmp_path))                                       # two model files: the caller has to choose
    m = load_mlsd(str(tmp_path), allow_patterns="*.pth")
    assert m.dtype == torch.float32 and torch.equal(m.state_dict()["block23.conv3.weight"], sd["block23.conv3.weight"])
