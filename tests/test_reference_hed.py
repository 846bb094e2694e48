"""tests/hed_ref.py and gyre_amd against the REFERENCE's own HED and HedPipeline.

tests/golden/ref_hed_probe.py loads gyre/pipeline/hinters/models/hed.py and gyre/pipeline/hinters/hed_pipeline.py from /root/reference
(the latter's ``kornia`` / ``torchvision`` / ``diffusers`` imports replaced by stand-ins) and requires: ``weights.hed_param_shapes``
equal to the reference's ``state_dict()`` - keys, order and shapes, 38 entries; ``hed_ref``'s stage sizes and crop offsets equal to what
the reference's own layers and ``crop()`` give for sides 1 .. 80; ``hed_ref.net`` equal to ``HED.forward`` bit for bit in fp32 (both
torch in one process, the same operations in the same order) on every MODEL_CASES entry; a strict load of the reference's state dict
into the native module shell; and the pipeline's host steps equal to the reference pipeline's on 1-, 3- and 4-channel, 3-dimensional
and float64 inputs.  Build container only."""
import json
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree only exists in the build container")


def test_shapes_geometry_forward_load_and_pipeline_match_the_reference():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_hed_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0].split("PROBE_JSON ", 1)[1])
    assert out["shapes"] == dict(n=38, same=True, same_order=True)
    assert out["geometry"] == dict(sizes=True, offsets=True)
    assert set(out["forward"]) == {"1x1", "5x7", "16x16", "33x20", "64x47", "13x4"}
    for name, c in out["forward"].items():
        print(f"[hed] reference forward {name}: largest difference {c['max_abs']:.3e}")
        assert c["equal"] and c["n"] == 6, (name, c)
    assert out["forward"]["64x47"]["shape"] == [2, 1, 64, 47] and out["forward"]["1x1"]["shape"] == [2, 1, 1, 1]
    assert out["strict_load"] == dict(missing=[], unexpected=[], same=True)
    assert "error" not in out["pipeline"], out["pipeline"]
    assert set(out["pipeline"]) == {"1ch", "3ch", "4ch", "3dim", "f64", "modules"} and out["pipeline"]["modules"]
    for label in ("1ch", "3ch", "4ch", "3dim", "f64"):
        c = out["pipeline"][label]
        assert c["equal"] and c["same_dtype"] and c["spread"] == 1.0, (label, c)
