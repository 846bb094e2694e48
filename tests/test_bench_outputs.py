"""bench.py's plain line and --dump-outputs: what the timed path computed in its last step, written as float32 .npy files that two
builds can be compared by (CPU: the size cap and its fixed sample; -m gpu: a plain run at a tiny size)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_small_outputs_whole_and_samples_large_ones_under_the_cap(tmp_path):
    import bench
    small = {"latents": torch.randn(2, 4, 8, 8, dtype=torch.bfloat16), "images": torch.rand(2, 3, 16, 16)}
    bench.dump_outputs(str(tmp_path / "s"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "s" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v.float().numpy())
    g = torch.Generator().manual_seed(1)
    big = {"latents": torch.randn(64, 4, 64, 64, generator=g), "images": torch.rand(64, 3, 512, 512, generator=g)}   # 200 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    sizes = [os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in big]
    assert sum(sizes) <= 64 << 20 and min(sizes) > 0
    for k, v in big.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)                      # the same sample every time
        assert np.isin(a[:100], v.reshape(-1).numpy()).all()                       # of the array's own elements


@pytest.mark.gpu
def test_plain_line_times_the_steps_asked_for_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_FORCE_DEVICE")}
    outs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--inference-steps", "2",
               "--batch", "1", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout + r.stderr)[-3000:]
        outs.append(json.loads(lines[0]))
    out = outs[0]
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert abs(out["ms_per_step"] - 1e3 / out["value"]) < 0.01 * out["ms_per_step"]     # batch 1: one image per step
    for k in ("roofline", "kernel_classes", "cpu_baseline", "clock_power", "latency_b1_s", "value_checked_attention"):
        assert k not in out, k                                                          # --full only
    lat, img = np.load(tmp_path / "a" / "latents.npy"), np.load(tmp_path / "a" / "images.npy")
    assert lat.shape == (1, 4, 64, 64) and img.shape == (1, 3, 512, 512)
    assert lat.dtype == img.dtype == np.float32 and np.isfinite(lat).all() and np.isfinite(img).all()
    # same arguments, same inputs: the second run's outputs are the first's (bit-identical kernels, fixed seeds)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "latents.npy"), lat)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "images.npy"), img)
