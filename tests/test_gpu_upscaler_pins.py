"""Launch count and workspace size of one forward of each upscaler family (-m gpu), pinned.  The three graphs share their trunk and
their handle shell (csrc/model_upscaler.h); a change to either shows up here as a deliberate edit of a number.  The numbers were
recorded from the commit before the graphs were moved onto the shared trunk ("The upscaler graphs share one trunk") and
are the same in both storage flavours.  They are those of the FIRST forward of a fresh module: it includes the launches that fill the
derived weight copies (SwinIR's expanded position bias per block, the chunk-ordered weights of RRDB's fused convolutions)."""
import pytest
import torch

import hat_ref
import swinir_ref
from gyre_amd import config as gcfg, weights
from gyre_amd.upscaler import GyreHipHAT, GyreHipRRDBNet, GyreHipSwinIR
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def _swinir():
    cfg, sd, _ = swinir_ref.model_case("tiny")          # tiny_swinir()
    return GyreHipSwinIR(cfg), sd


def _hat():
    cfg, sd, _ = hat_ref.model_case("tiny")             # tiny_hat()
    return GyreHipHAT(cfg), sd


def _rrdb():
    cfg = gcfg.tiny_rrdb()
    return GyreHipRRDBNet(cfg), weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg))


# family: (module and weights, image shape, launches of the first forward, workspace bytes)
PINS = {"swinir": (_swinir, (1, 3, 16, 24), 53, 1818624),
        "hat": (_hat, (1, 3, 32, 48), 91, 8060928),
        "rrdb": (_rrdb, (2, 3, 24, 20), 76, 4423680)}


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("family", list(PINS))
def test_forward_launch_count_and_workspace(family, sdt):
    make, shape, launches, workspace = PINS[family]
    m, sd = make()
    m.load_state_dict(sd, strict=False)                 # (the index / mask buffers of the transformers are not in the synthetic weights)
    m = m.to(sdt).to(DEV)
    out = m(torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(DEV))
    torch.cuda.synchronize()
    got = (int(m._L().gyre_last_launch_count()), m.workspace_bytes(shape[0], shape[2], shape[3], torch.device(DEV)))
    print(f"[pins] {family} {sdt}: {got[0]} launches, {got[1]} workspace bytes, output {tuple(out.shape)}")
    assert got == (launches, workspace)
