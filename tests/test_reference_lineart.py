"""tests/lineart_ref.py and gyre_amd against the REFERENCE's own line-art generator and pipeline.

tests/golden/ref_lineart_probe.py loads gyre/pipeline/hinters/models/informative_drawings.py and
gyre/pipeline/hinters/informative_drawing_pipeline.py from /root/reference (the latter's ``kornia`` / ``torchvision`` / ``diffusers``
imports replaced by stand-ins) and requires: ``weights.lineart_param_shapes`` equal to the reference's ``state_dict()`` - keys, order and
shapes - for 1, 3 and 9 residual blocks; ``lineart_ref.net`` equal to the reference's forward bit for bit (both fp32 torch in one
process, the same operations in the same order), an odd size included; a strict load of the reference's state dict into the native
module shell; and the pipeline's host steps equal to the reference pipeline's on 1-, 3- and 4-channel, 3-dimensional and float64
inputs.  Build container only."""
import json
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


def test_shapes_forward_load_and_pipeline_match_the_reference():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_lineart_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0].split("PROBE_JSON ", 1)[1])
    assert set(out["shapes"]) == {"1", "3", "9"}
    for blocks, c in out["shapes"].items():
        assert c["same"] and c["same_order"] and c["n"] == 12 + 4 * int(blocks), (blocks, c)
    assert set(out["forward"]) == {"tiny", "shipped", "odd"}
    for name, c in out["forward"].items():
        print(f"[lineart] reference forward {name}: largest difference {c['max_abs']:.3e} (output up to {c['ref_absmax']:.3f})")
        assert c["equal"], (name, c)
    assert out["forward"]["odd"]["shape"] == [1, 1, 16, 20] and out["forward"]["shipped"]["shape"] == [2, 1, 32, 40]
    assert out["strict_load"] == dict(missing=[], unexpected=[], same=True)
    assert "error" not in out["pipeline"], out["pipeline"]
    assert set(out["pipeline"]) == {"1ch", "3ch", "4ch", "3dim", "f64", "modules"} and out["pipeline"]["modules"]
    for label in ("1ch", "3ch", "4ch", "3dim", "f64"):
        assert out["pipeline"][label]["equal"] and out["pipeline"][label]["same_dtype"], (label, out["pipeline"][label])
