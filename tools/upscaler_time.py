"""Dev tool: the fused dense-block convolution against the generic path of the native RRDBNet (profiles/README.md).  One process,
HIP events, alternating rounds, medians:

  * one stacked 9 x 256 x 256 module call (the tiles of a 512 x 512 request) of the 23-block x4 net: generic, fused, and the fused
    kernel for ONE shape group at a time (the tuning form of gyre_rrdb_set_path) - the per-group differences decide `auto`
  * one 512 x 512 -> 2048 x 2048 pipeline request at batch 1: generic, fused, auto

`python tools/upscaler_time.py [out.json]`; ROUNDS, DTYPE (bf16 | f16), BLOCKS from the environment.  Synthetic weights."""
import json
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import config as gcfg, weights
from gyre_amd.upscaler import GyreHipRRDBNet, GyreUpscalerPipeline

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
BLOCKS = int(os.environ.get("BLOCKS", "23"))
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}[os.environ.get("DTYPE", "bf16")]
GROUPS = ["dense conv1-4 (N=32)", "dense conv5 (N=64, Cin=192)", "conv_up1/2 (nearest 2x)", "conv_last (3 live)", "conv_first/body/hr (N=64)"]


def sclk():
    try:
        o = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
        m = re.search(r"sclk clock level: \S+ \((\d+)Mhz\)", o)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cfg = gcfg.rrdb_config(num_block=BLOCKS)
net = GyreHipRRDBNet(cfg)
net.load_state_dict(weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg)))
net = net.to(DTYPE).to(dev)
g = torch.Generator().manual_seed(0)
tiles = torch.rand((9, 3, 256, 256), generator=g).to(dev)
image = torch.rand((1, 3, 512, 512), generator=g).to(dev)
pipe = GyreUpscalerPipeline(net)

paths = {"generic": "generic", "fused": "fused", **{f"only group {i}": 0x100 | (1 << i) for i in range(5)}}
ms, clocks = {k: [] for k in paths}, []
for k, p in paths.items():                       # warm-up: workspace, derived weight copies, every shape
    net.set_path(p)
    net(tiles)
for _ in range(ROUNDS):
    for k, p in paths.items():
        net.set_path(p)
        ms[k].append(timed(lambda: net(tiles)))
    clocks.append(sclk())
med = {k: statistics.median(v) for k, v in ms.items()}
macs = 9 * 65536 * (BLOCKS * 3 * 9 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64) + 9 * 64 * 64 * (2 + 4 + 16 + 16) + 16 * 9 * 64 * 3)
result = {"dtype": str(DTYPE), "num_block": BLOCKS, "rounds": ROUNDS, "sclk_mhz": [c for c in clocks if c],
          "stacked_9x256x256": {k: {"median_ms": med[k], "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()},
          "tmac": macs / 1e12, "tflops_generic": 2 * macs / med["generic"] / 1e9, "tflops_fused": 2 * macs / med["fused"] / 1e9,
          "groups": [{"group": i, "what": GROUPS[i], "fused_minus_generic_ms": med[f"only group {i}"] - med["generic"],
                      "fused_wins": med[f"only group {i}"] < med["generic"]} for i in range(5)]}
result["auto_mask_measured"] = sum(1 << r["group"] for r in result["groups"] if r["fused_wins"])
print(json.dumps(result["stacked_9x256x256"]), flush=True)
print(json.dumps(result["groups"]), flush=True)

rq = {"generic": [], "fused": [], "auto": []}
for k in rq:
    net.set_path(k)
    pipe(image)
for _ in range(max(2, ROUNDS // 2)):
    for k in rq:
        net.set_path(k)
        rq[k].append(timed(lambda: pipe(image)))
result["request_512_to_2048_batch1"] = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in rq.items()}
print(json.dumps(result["request_512_to_2048_batch1"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
