"""The LyCORIS operator tests on the fp16-storage flavour of the library: tests/test_gpu_lyco_native.py is written against
``gpu_util.HDT``; this file re-runs its operator tests in a child process with GYRE_STORAGE=f16 (as tests/test_gpu_f16_flavour.py
does for the files it lists), where HDT is torch.float16 and ``_lib.lib()`` is libgyre_hip_f16.so.  Same references, same bounds
(worked out for the storage type under test).  The model tests of that file reach both flavours by themselves (``.to(other)``)."""
import os
import subprocess
import sys

import pytest

from gyre_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(_lib.default_storage() == _lib.F16, reason="already inside the fp16 run")
def test_lycoris_operators_pass_on_the_fp16_flavour():
    env = dict(os.environ, GYRE_STORAGE="f16")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_lyco_native.py", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "operator or lora_terms or zero_terms"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-25:])
    print(tail)
    assert r.returncode == 0, f"fp16 flavour failed:\n{tail}\n{r.stderr[-2000:]}"
