"""Dev tool: a native window-transformer upscaler (SwinIR or HAT) against the restated reference network in PyTorch
(profiles/README.md).  One process, HIP events, alternating rounds, medians, for the two default configurations of the family
(swinir, swinir-l / hat, hat-l):

  * native   one stacked 9 x 256 x 256 module call (the tiles of a 512 x 512 request) through GyreHipSwinIR / GyreHipHAT, plus ONE
             more call with per-launch event timing on, which gives the split by kernel family (the events serialise the launches,
             so the split's total is a little above the unprofiled time)
  * torch    the same call through tests/swinir_ref.net / tests/hat_ref.net in the same 16-bit dtype on the GPU - the reference
             network's operations as PyTorch-ROCm runs them, which is what a server without the native path computes

`python tools/window_upscaler_time.py swinir|hat [out.json]`; ROUNDS, DTYPE (f16 | bf16), TILES, CONFIGS from the environment.
Synthetic weights."""
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

from gyre_amd import config as gcfg, upscaler, weights

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
TILES = int(os.environ.get("TILES", "9"))
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}[os.environ.get("DTYPE", "f16")]


def swinir_flops(cfg, tokens):
    """multiply-adds x 2 of one call: the linears and attention per token, the convolutions per pixel"""
    c, hid, blocks = cfg["embed_dim"], int(cfg["embed_dim"] * cfg["mlp_ratio"]), sum(cfg["depths"])
    lin = blocks * (3 * c * c + c * c + 2 * c * hid + 2 * 64 * c)
    resi = 9 * c * c if cfg["resi_connection"] == "1conv" else 2 * 9 * c * (c // 4) + (c // 4) ** 2
    conv = 9 * 3 * c + (len(cfg["depths"]) + 1) * resi + 9 * c * 64 + 9 * 64 * 64 * (4 + 16 + 16) + 16 * 9 * 64 * 3
    return 2.0 * tokens * (lin + conv)


def hat_flops(cfg, tokens):
    c, hid, habs, groups = cfg["embed_dim"], int(cfg["embed_dim"] * cfg["mlp_ratio"]), sum(cfg["depths"]), len(cfg["depths"])
    lin = (habs + groups) * (3 * c * c + c * c + 2 * c * hid) + habs * 2 * 256 * c + groups * 2 * 576 * c
    cab = habs * 2 * 9 * c * (c // 3)
    conv = 9 * 3 * c + (groups + 1) * 9 * c * c + 9 * c * 64 + 9 * 64 * 256 * (1 + 4) + 16 * 9 * 64 * 3
    return 2.0 * tokens * (lin + cab + conv)


# family -> what differs: the names of the default configurations, the config / shape / module entry points, the reference network,
# the flop count and what the profiler's class "other" holds
FAMILIES = {
    "swinir": dict(configs="swinir,swinir-l", defaults=gcfg.SWINIR_DEFAULTS, config=gcfg.swinir_config, shapes=weights.swinir_param_shapes,
                   is_buffer=weights.swinir_is_buffer, module=upscaler.GyreHipSwinIR, ref="swinir_ref", flops=swinir_flops,
                   other="GELU / leaky ReLU passes"),
    "hat": dict(configs="hat,hat-l", defaults=gcfg.HAT_DEFAULTS, config=gcfg.hat_config, shapes=weights.hat_param_shapes,
                is_buffer=weights.hat_is_buffer, module=upscaler.GyreHipHAT, ref="hat_ref", flops=hat_flops,
                other="GELU / leaky ReLU, channel attention, pixel shuffle")}
if len(sys.argv) < 2 or sys.argv[1] not in FAMILIES:
    sys.exit(f"usage: {sys.argv[0]} {' | '.join(FAMILIES)} [out.json]")
F = FAMILIES[sys.argv[1]]
R = __import__(F["ref"])
CONFIGS = os.environ.get("CONFIGS", F["configs"]).split(",")


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
        return "convolutions (3x3)" if name.rstrip(">").endswith(", 1") else "linear GEMMs"
    return {"k_attn": "window attention", "k_layernorm": "LayerNorm", "other": F["other"]}.get(name, name)


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
    return out


result = {"dtype": str(DTYPE), "rounds": ROUNDS, "tiles": TILES, "configs": {}}
x = torch.rand((TILES, 3, 256, 256), generator=torch.Generator().manual_seed(0)).to(dev)
for name in CONFIGS:
    cfg = F["config"](**F["defaults"][name])
    shapes = {k: v for k, v in F["shapes"](cfg).items() if not F["is_buffer"](k)}
    sd = weights.synthetic_state_dict(shapes)
    net = F["module"](cfg)
    net.load_state_dict(sd, strict=False)
    net = net.to(DTYPE).to(dev)
    sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
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
    fl = F["flops"](cfg, TILES * 65536)
    r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
         "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
         "torch_over_native": med["torch"] / med["native"], "tflop": fl / 1e12, "native_tflops": fl / med["native"] / 1e9,
         "native_split_ms": split, "native_split_total_ms": sum(f["ms"] for f in split.values()),
         "workspace_gb": net.workspace_bytes(TILES, 256, 256, dev) / 2 ** 30, "rel_l2_native_vs_torch": agree,
         "sclk_mhz": [c for c in clocks if c]}
    result["configs"][name] = r
    print(name, json.dumps(r), flush=True)
    del net, sdg
    torch.cuda.empty_cache()
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(result, f, indent=1)
