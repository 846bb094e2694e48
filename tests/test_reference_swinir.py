"""tests/swinir_ref.py and gyre_amd against the REFERENCE's own SwinIR.

tests/golden/ref_swinir_probe.py loads gyre/pipeline/upscalers/models/network_swinir.py from /root/reference (the three ``timm`` names
it imports replaced by stand-ins) and requires: ``weights.swinir_param_shapes`` equal to the reference's ``state_dict()`` - keys, order
and shapes, buffers included - for the two tiny configurations, ``swinir`` and ``swinir-l``; the default tables equal to the reference
loader's; ``swinir_ref.net`` equal to the reference's forward bit for bit (both fp32 torch in one process, the same operations in the
same order) on aligned and unaligned images, 1conv x4 and 3conv x2; and a strict load of the reference's full state dict into the
native module shell.  Build container only."""
import json
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


def test_shapes_defaults_and_forward_match_the_reference():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_swinir_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0].split("PROBE_JSON ", 1)[1])
    assert set(out["shapes"]) == {"tiny", "tiny3", "swinir", "swinir-l"}
    for name, c in out["shapes"].items():
        assert c["same"] and c["same_order"] and c["n"] > 50, (name, c)
    for name, c in out["default_configs"].items():
        assert c["ref"] is not None and c["ref"] == c["mine"] == c["table"], (name, c)
    assert set(out["forward"]) == {"tiny_2x3x16x24", "tiny_1x3x13x21", "tiny3_2x3x16x24", "tiny3_1x3x13x21"}
    for name, c in out["forward"].items():
        print(f"[swinir] reference forward {name}: largest difference {c['max_abs']:.3e} (output up to {c['ref_absmax']:.3f})")
        assert c["equal"], (name, c)
    assert out["forward"]["tiny_1x3x13x21"]["shape"] == [1, 3, 52, 84] and out["forward"]["tiny3_1x3x13x21"]["shape"] == [1, 3, 26, 42]
    assert out["strict_load"] == dict(missing=[], unexpected=[], same=True)
