"""The four-parity upsampler tests on the fp16-storage flavour of the library: tests/test_gpu_ups4_conv.py and
tests/test_gpu_ups4_model.py are written against gpu_util.HDT and re-run here in a child process with GYRE_STORAGE=f16, the way
tests/test_gpu_f16_flavour.py re-runs the older operator and model files."""
import os
import subprocess
import sys

import pytest

from gyre_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["tests/test_gpu_ups4_conv.py", "tests/test_gpu_ups4_model.py"]


@pytest.mark.skipif(_lib.default_storage() == _lib.F16, reason="already inside the fp16 run")
def test_ups4_operator_and_model_tests_pass_on_the_fp16_flavour():
    env = dict(os.environ, GYRE_STORAGE="f16")
    r = subprocess.run([sys.executable, "-m", "pytest", *FILES, "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.splitlines()[-60:])
    print(tail)
    assert r.returncode == 0, f"fp16 flavour failed:\n{tail}\n{r.stderr[-2000:]}"
