"""Dev tool: the native line-art generator against the restated reference network in PyTorch (profiles/README.md).  One process, HIP
events, alternating rounds, medians after a warm-up call of each, for the shipped configuration (3 -> 1 channels, 3 residual blocks,
sigmoid) on one 512 x 512 image and on a batch of 8:

  * native   the module call through GyreHipDrawingGenerator, plus ONE more call with per-launch event timing on, which gives the
             split by kernel family (the events serialise the launches, so the split's total is a little above the unprofiled time)
  * torch    the same call through tests/lineart_ref.net in the same 16-bit dtype on the GPU - the reference network's operations as
             PyTorch-ROCm runs them, which is what a server without the native path computes

`python tools/lineart_time.py [out.json]`; ROUNDS, DTYPE (f16 | bf16), BLOCKS from the environment.  Synthetic weights."""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import lineart_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.hinters import GyreHipDrawingGenerator

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
BLOCKS = int(os.environ.get("BLOCKS", "3"))
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}[os.environ.get("DTYPE", "f16")]
SHAPES = {"1x512x512": (1, 3, 512, 512), "8x512x512": (8, 3, 512, 512)}


def flops(blocks, pixels):
    """multiply-adds x 2 of one call: per input pixel the first 7x7, the two stride-2 convolutions (1/4 and 1/16 of the pixels), the
    residual blocks at 1/16, the transposed convolutions as built (4 Cin x 4 Cout per source pixel) and the last 7x7"""
    per = 147 * 64 + 9 * 64 * 128 / 4 + 9 * 128 * 256 / 16 + blocks * 2 * 9 * 256 * 256 / 16 + 1024 * 512 / 16 + 512 * 256 / 4 + 49 * 64
    return 2.0 * pixels * per


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


def family(name):
    if name.startswith("k_gemm") or name == "k_splitk_reduce":
        return "convolutions (3x3)" if name.rstrip(">").endswith(", 1") else "transposed convolutions (linear GEMMs)"
    return {"k_gn_partial+k_gn_finalize": "instance-norm statistics", "k_gn_apply": "instance-norm apply (pad / patch / shuffle)",
            "other": "7x7 convolutions"}.get(name, name)


def profile_split(net, x):
    """{family: ms} of one call with per-launch event timing (the library's profiling scopes)"""
    L = net._L()
    n = L.gyre_prof_num_classes()
    L.gyre_prof_set_mask((1 << n) - 1)
    la, ms, fl, by = (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    torch.cuda.synchronize()
    L.gyre_prof_collect(la, ms, fl, by)                       # drop what earlier calls left
    net(x)
    torch.cuda.synchronize()
    L.gyre_prof_collect(la, ms, fl, by)
    L.gyre_prof_set_mask(0)
    out = {}
    for k in range(n):
        if la[k]:
            f = out.setdefault(family(L.gyre_prof_class_name(k).decode()), dict(launches=0, ms=0.0))
            f["launches"] += int(la[k])
            f["ms"] += float(ms[k])
    # The family names rest on kernel and class names; the graph's own launch counts say whether they still sort the launches right:
    # 2 + 2 BLOCKS planner convolutions, 5 + 2 BLOCKS normalisations (one timed scope per statistics pair and per apply), two 7x7s
    want = {"convolutions (3x3)": 2 + 2 * BLOCKS, "instance-norm statistics": 5 + 2 * BLOCKS,
            "instance-norm apply (pad / patch / shuffle)": 5 + 2 * BLOCKS, "7x7 convolutions": 2}
    have = {k: out.get(k, {}).get("launches", 0) for k in want}
    if have != want or set(out) - set(want) - {"transposed convolutions (linear GEMMs)"}:
        raise SystemExit(f"the split by kernel family no longer matches the graph: launches {out}, expected {want}")
    return out


cfg = gcfg.lineart_config(3, 1, BLOCKS, True)
sd = weights.synthetic_state_dict(weights.lineart_param_shapes(cfg))
net = GyreHipDrawingGenerator(3, 1, BLOCKS, True)
net.load_state_dict(sd)
net = net.to(DTYPE).to(dev)
sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
result = {"dtype": str(DTYPE), "rounds": ROUNDS, "n_residual_blocks": BLOCKS, "shapes": {}}
for label, shape in SHAPES.items():
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(dev)
    xh = x.to(DTYPE)
    torch_call = lambda: R.net(sdg, cfg, xh, compute=DTYPE)
    with torch.no_grad():
        got = net(x)                                          # warm-up: workspace, derived weight copies
        want = torch_call()
        agree = R.rel_l2(got.float().cpu(), want.float().cpu())
        ms, clocks = {"native": [], "torch": []}, []
        for _ in range(ROUNDS):
            ms["native"].append(timed(lambda: net(x)))
            ms["torch"].append(timed(torch_call))
            clocks.append(sclk())
        split = profile_split(net, x)
    med = {k: statistics.median(v) for k, v in ms.items()}
    fl = flops(BLOCKS, shape[0] * shape[2] * shape[3])
    r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
         "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
         "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
         "tflop": fl / 1e12, "native_tflops": fl / med["native"] / 1e9,
         "native_split_ms": split, "native_split_total_ms": sum(f["ms"] for f in split.values()),
         "workspace_gb": net.workspace_bytes(shape[0], shape[2], shape[3], dev) / 2 ** 30, "rel_l2_native_vs_torch": agree,
         "sclk_mhz": [c for c in clocks if c]}
    result["shapes"][label] = r
    print(label, json.dumps(r), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
