"""tests/bae_ref.py and gyre_amd against the REFERENCE's own Decoder (gyre/pipeline/hinters/baenormal/submodules/decoder.py, executed
from /root/reference when it is there, args.architecture = "BN"): weights.bae_param_shapes equal to its state_dict() - keys, order,
shapes; a strict load of its state dict into the native module shell; bae_ref.decoder within rtol 1e-5 / atol 1e-6 of its
forward(mode='test') in fp32 (the margin tests/test_reference_mlsd.py gives the same ATen operations); and the size rule: for every
x_block0 side in 1 .. 40 its forward runs exactly when the side is a multiple of 4.  Build container only."""
import importlib
import os
import sys
import types
from types import SimpleNamespace

import pytest
import torch

import bae_ref as R
from gyre_amd import config as gcfg, hinters as HN, weights

DIR = os.path.join("/root/reference", "gyre", "pipeline", "hinters", "baenormal", "submodules")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(DIR, "decoder.py")), reason="reference tree only exists in the build container")
CFG = gcfg.bae_config()


@pytest.fixture(scope="module")
def reference():
    pkg = types.ModuleType("ref_bae_submodules")                     # (decoder.py imports its sibling relatively)
    pkg.__path__ = [DIR]
    sys.modules["ref_bae_submodules"] = pkg
    mod = importlib.import_module("ref_bae_submodules.decoder")
    model = mod.Decoder(SimpleNamespace(architecture="BN", sampling_ratio=0.4, importance_ratio=0.7)).eval()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(R.seeded_state_dict(weights.bae_param_shapes(CFG)), strict=False)
    return model, shapes


def test_shapes_and_strict_load(reference):
    model, shapes = reference
    mine = weights.bae_param_shapes(CFG)
    assert list(shapes) == list(mine) and all(tuple(mine[k]) == v for k, v in shapes.items())
    shell = HN.GyreHipBaeDecoder("BN")
    r = shell.load_state_dict(model.state_dict(), strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in shell.state_dict().items())


@pytest.mark.parametrize("B,H,W", [(1, 4, 8), (2, 12, 8)])
def test_restatement_equals_the_reference_forward(reference, B, H, W):
    blocks = R.seeded_blocks(CFG, B, H, W)
    with torch.no_grad():
        want, second, third = reference[0](R.features(blocks), mode="test")
    got = R.decoder({k: v for k, v in reference[0].state_dict().items()}, blocks)
    assert second[0] is want[0] and second[1:] == [None] * 3 and third == [None] * 4
    for i, (a, b) in enumerate(zip(got, want)):
        print(f"[bae] reference forward {B}x{H}x{W} map {i}: largest difference {float((a - b).abs().max()):.3e}")
        assert a.shape == b.shape == (B, 4, (H // 4) << i, (W // 4) << i)
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_size_rule_is_the_reference_s(reference):
    shell = HN.GyreHipBaeDecoder("BN")
    for n in range(1, 41):
        for H, W in ((n, 4), (4, n)):
            try:
                with torch.no_grad():
                    out = reference[0](R.features([torch.zeros(s) for s in shell.block_shapes(1, H, W)]), mode="test")[0]
                ran = tuple(out[3].shape) == (1, 4, 2 * H, 2 * W)
            except Exception:
                ran = False
            assert ran == gcfg.bae_size_ok(n), (H, W)
