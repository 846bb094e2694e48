"""tests/hat_ref.py and gyre_amd against the REFERENCE's own HAT.

tests/golden/ref_hat_probe.py loads gyre/pipeline/upscalers/models/hat_arch.py from /root/reference (the three ``basicsr`` names it
imports replaced by stand-ins) and requires: ``weights.hat_param_shapes`` equal to the reference's ``state_dict()`` - keys, order and
shapes, the two index buffers included - for the two tiny configurations, ``hat`` and ``hat-l``; the default tables equal to the
reference loader's; the closed-form indices and mask of the kernel equal to the reference's buffers and ``calculate_mask``;
``hat_ref.net`` equal to the reference's forward bit for bit (both fp32 torch in one process, the same operations in the same order),
x4 and x2; and a strict load of the reference's full state dict into the native module shell.  Build container only."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "ref_hat_probe.py")], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [l for l in r.stdout.splitlines() if "PROBE_JSON " in l]
    assert r.returncode == 0 and line, (r.stdout + r.stderr)[-3000:]
    out = json.loads(line[0].split("PROBE_JSON ", 1)[1])
    assert set(out["shapes"]) == {"tiny", "tiny2", "hat", "hat-l"}
    for name, c in out["shapes"].items():
        assert c["same"] and c["same_order"] and c["n"] > 50, (name, c)
    for name, c in out["default_configs"].items():
        assert c["ref"] is not None and c["ref"] == c["mine"] == c["table"], (name, c)
    assert out["indices"] == dict(sa=True, sa_closed=True, oca=True, oca_closed=True, mask=True)
    assert set(out["forward"]) == {"tiny_1x3x16x32", "tiny2_1x3x32x48"}
    for name, c in out["forward"].items():
        print(f"[hat] reference forward {name}: largest difference {c['max_abs']:.3e} (output up to {c['ref_absmax']:.3f})")
        assert c["equal"], (name, c)
    assert out["forward"]["tiny_1x3x16x32"]["shape"] == [1, 3, 64, 128] and out["forward"]["tiny2_1x3x32x48"]["shape"] == [1, 3, 64, 96]
    assert out["strict_load"] == dict(missing=[], unexpected=[], same=True)
