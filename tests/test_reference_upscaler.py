"""gyre_amd.upscaler against the REFERENCE's own upscaler host logic.

tests/golden/ref_upscaler_probe.py loads gyre/pipeline/upscalers/utils.py and upscaler_loader.py from /root/reference (absent
third-party modules replaced by stand-ins, the Gaussian blur common to both sides) and requires: ``tile`` bit for bit in fp32 over a
toy module - tile by tile and as one stacked batch - the old-format key conversion tensor for tensor, the same refusals, and equal
default configuration tables; ``images.rescale`` / ``resize`` / ``scale_shape`` / ``fromPIL`` of gyre/images.py bit for bit over every fit,
odd surpluses and shortfalls included (the resampling itself is common to both sides).  Build container only."""
import json
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


def test_tile_conversion_and_defaults_match_the_reference():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_upscaler_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0].split("PROBE_JSON ", 1)[1])
    assert len(out["tile"]) >= 6
    for name, c in out["tile"].items():
        assert c["same_shape"] and c["seq_equal"] and c["stacked_equal"], (name, c)
    assert out["tile"]["default_512_x4"]["shape"] == [1, 3, 2048, 2048]
    assert out["tile64_default_feather"] == {"ref": "refused", "mine": "refused"}
    assert len(out["rescale"]) >= 40
    for name, c in out["rescale"].items():
        assert c["equal"], (name, c)
    assert out["rescale"]["400x360->380x300 cover s1"]["shape"] == [1, 3, 380, 300]
    assert all(out["resize_factor_forms"]) and len(out["resize_factor_forms"]) == 5 and all(out["scale_shape"]) and all(out["from_pil"])
    for key in ("convert", "convert_plus"):
        c = out[key]
        assert c["same_keys"] and c["same_tensors"] and c["n"] > 700, (key, c)
        assert c["errors"] == {"missing": ["ValueError", "ValueError"], "leftover": ["ValueError", "ValueError"]}
    for name, c in out["default_configs"].items():
        assert c["ref"] is not None and c["ref"] == c["mine"], (name, c)
    assert all(a and b for a, b in out["loader_surface"].values())
