"""tests/mlsd_ref.py and gyre_amd against the REFERENCE's own MobileV2_MLSD_Large (gyre/pipeline/hinters/models/mbv2_mlsd_large.py,
executed from /root/reference when it is there): weights.mlsd_param_shapes equal to its state_dict() - keys, order, shapes, 362
entries; a strict load of its state dict into the native module shell; mlsd_ref.net within rtol 1e-5 / atol 1e-6 of its forward in fp32
on every MODEL_CASES entry (the margin tests/test_t2i_host.py gives the same ATen operations); and the size rule: for every side in
2 .. 129 its forward runs exactly when n >= 16 and (n // 2) % 8 == 0.  Build container only."""
import importlib.util
import os

import pytest
import torch

import mlsd_ref as R
from gyre_amd import config as gcfg, hinters as HN, weights

REF = "/root/reference"
FILE = os.path.join(REF, "gyre", "pipeline", "hinters", "models", "mbv2_mlsd_large.py")
pytestmark = pytest.mark.skipif(not os.path.isfile(FILE), reason="reference tree only exists in the build container")


@pytest.fixture(scope="module")
def reference():
    spec = importlib.util.spec_from_file_location("ref_mbv2_mlsd_large", FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.MobileV2_MLSD_Large().eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(R.model_weights(), strict=True)
    return model, shapes


def test_shapes_and_strict_load(reference):
    model, shapes = reference
    mine = weights.mlsd_param_shapes()
    assert len(shapes) == 362 and list(shapes) == list(mine) and all(tuple(mine[k]) == v for k, v in shapes.items())
    shell = HN.GyreHipMLSD()
    r = shell.load_state_dict(model.state_dict(), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in shell.state_dict().items())


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_restatement_equals_the_reference_forward(reference, name):
    sd, x = R.model_case(name)
    with torch.no_grad():
        want = reference[0](x)
    got = R.net(sd, x)
    B, H, W = R.MODEL_CASES[name]
    print(f"[mlsd] reference forward {name}: largest difference {R.max_abs(got, want):.3e}")
    assert got.shape == want.shape == (B, 9, H // 2, W // 2)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


def test_size_rule_is_the_reference_s(reference):
    model = reference[0]
    for n in range(2, 130):
        for shape in ((1, 4, n, 16), (1, 4, 16, n)):
            try:
                with torch.no_grad():
                    out = model(torch.zeros(shape))
                ran = tuple(out.shape) == (1, 9, shape[2] // 2, shape[3] // 2)
            except Exception:
                ran = False
            assert ran == R.size_ok(n) == gcfg.mlsd_size_ok(n), (n, shape)
