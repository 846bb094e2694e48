"""Dev tool: the native MLSD line detector against the restated reference network in PyTorch (profiles/README.md).  One process, HIP
events, alternating rounds, medians after a warm-up call of each, in fp16, on one 512 x 512 image and on a batch of 8:

  * native   the module call through GyreHipMLSD
  * torch    the same call through tests/mlsd_ref.net in fp16 on the GPU - the reference network's operations (convolution, eval-mode
             BatchNorm, ReLU6, interpolate) as PyTorch-ROCm runs them, which is what a server without the native path computes
  * split    per kernel class of the native call, its time and share: the planner launches from ONE more call with the library's
             per-launch event timing on (the events serialise the launches, so the sum is a little above the unprofiled call); the
             MLSD kernels through their raw-operator hooks on the shapes of the graph, REPS launches between two events; and the
             in-place ReLU6 pass the depthwise kernel's read-side ReLU6 replaces, measured on the same tensors
  * clocks   `rocm-smi --showclocks` before and after, as text (read only)

`python tools/mlsd_time.py [out.json]`; ROUNDS, REPS from the environment; `python tools/mlsd_time.py --calls N B` only runs N native
calls at batch B (the target of a kernel trace).  Seeded weights (tests/mlsd_ref.model_weights)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import mlsd_ref as R
from gyre_amd import _lib
from gyre_amd.hinters import GyreHipMLSD

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REPS = int(os.environ.get("REPS", "10"))
DTYPE = torch.float16
SHAPES = {"1x512x512": (1, 4, 512, 512), "8x512x512": (8, 4, 512, 512)}
pad32 = lambda c: (c + 31) // 32 * 32


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l or "fclk" in l)]
    except Exception as e:                                            # the measurement does not depend on it
        return [f"unavailable: {e}"]


def timed(fn, reps=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def median_ms(fn):
    fn()
    return statistics.median(timed(fn, REPS) for _ in range(ROUNDS))


def planner_ms(net, x):
    """{class: ms} and the launch count of one call with per-launch event timing; the MLSD kernels are 'other'"""
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
    per = {L.gyre_prof_class_name(k).decode(): {"ms": float(ms[k]), "launches": int(la[k])} for k in range(n) if la[k]}
    return per


def hook_split(L, B, H, W):
    """{class: ms} of the kernels that are not planner launches, each through its hook on the graph's shapes (any values)"""
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    p = lambda t: C.c_void_p(t.data_ptr())
    out = {"entry convolution": 0.0, "depthwise": 0.0, "upsample": 0.0, "dilated convolution": 0.0, "in-place ReLU / ReLU-add passes": 0.0, "exit": 0.0,
           "(not in the graph) in-place ReLU6 of the expand outputs": 0.0}
    h, w = H // 2, W // 2
    x = torch.rand((B, 4, H, W), device=dev)
    y = torch.empty((B, h, w, 32), dtype=DTYPE, device=dev)
    w36, b32 = torch.randn((36, 32), device=dev).to(DTYPE), torch.zeros(32, device=dev)
    out["entry convolution"] = median_ms(lambda: _lib.check(L.gyre_op_mlsd_entry(st, p(x), 0, B, H, W, p(w36), p(b32), p(y)), L))
    cin = 32
    for t, c, n, s in R.SETTING:
        for i in range(n):
            stride, hid = (s if i == 0 else 1), pad32(t * cin)
            xi = torch.randn((B, h, w, hid), device=dev).to(DTYPE)
            yo = torch.empty((B, h // stride, w // stride, hid), dtype=DTYPE, device=dev)
            wd, bd = torch.randn((9, hid), device=dev).to(DTYPE), torch.zeros(hid, device=dev)
            out["depthwise"] += median_ms(lambda: _lib.check(L.gyre_op_dwconv3(st, p(xi), B, h, w, hid, p(wd), p(bd), stride, int(t != 1), p(yo)), L))
            if t != 1:
                out["(not in the graph) in-place ReLU6 of the expand outputs"] += median_ms(
                    lambda: _lib.check(L.gyre_op_mlsd_act(st, p(xi), B * h * w, hid, hid, 1), L))
            h, w, cin = h // stride, w // stride, c
    hh, ww = H // 16, W // 16                                         # block15 / 16 at h / 8, then three levels up
    for k in range(4):
        if k:
            bb = torch.randn((B, hh, ww, 64), device=dev).to(DTYPE)
            hh, ww = 2 * hh, 2 * ww
        cat = torch.randn((B, hh, ww, 128), device=dev).to(DTYPE)
        t128 = torch.randn((B, hh, ww, 128), device=dev).to(DTYPE)
        u64 = torch.randn((B, hh, ww, 64), device=dev).to(DTYPE)
        if k:
            out["upsample"] += median_ms(lambda: _lib.check(L.gyre_op_upsample2_ac(st, p(bb), B, hh // 2, ww // 2, 64, 64, 1,
                                                                                   C.c_void_p(cat.data_ptr() + 128), 128), L))
            out["in-place ReLU / ReLU-add passes"] += median_ms(lambda: _lib.check(L.gyre_op_mlsd_act(st, p(cat), B * hh * ww, 64, 128, 0), L))
        else:
            out["in-place ReLU / ReLU-add passes"] += median_ms(lambda: _lib.check(L.gyre_op_mlsd_act(st, p(cat), B * hh * ww, 128, 128, 0), L))
        out["in-place ReLU / ReLU-add passes"] += median_ms(lambda: _lib.check(L.gyre_op_mlsd_relu_add(st, p(t128), p(cat), t128.numel()), L))
        out["in-place ReLU / ReLU-add passes"] += median_ms(lambda: _lib.check(L.gyre_op_mlsd_act(st, p(u64), B * hh * ww, 64, 64, 0), L))
    x64, y64 = torch.randn((B, hh, ww, 64), device=dev).to(DTYPE), torch.empty((B, hh, ww, 64), dtype=DTYPE, device=dev)
    w9, b64 = (torch.randn((64, 9, 64), device=dev) / 24).to(DTYPE), torch.zeros(64, device=dev)
    out["dilated convolution"] = median_ms(lambda: _lib.check(L.gyre_op_dconv3_d5(st, p(x64), B, hh, ww, p(w9), p(b64), p(y64)), L))
    out["in-place ReLU / ReLU-add passes"] += median_ms(lambda: _lib.check(L.gyre_op_mlsd_act(st, p(y64), B * hh * ww, 64, 64, 0), L))
    x16, o9 = torch.randn((B, hh, ww, 16), device=dev).to(DTYPE), torch.empty((B, 9, hh, ww), dtype=DTYPE, device=dev)
    out["exit"] = median_ms(lambda: _lib.check(L.gyre_op_mlsd_exit(st, p(x16), B, hh, ww, p(o9), _lib.F16), L))
    return out


def main():
    sd = R.model_weights()
    net = GyreHipMLSD()
    net.load_state_dict(sd)
    net = net.to(DTYPE).to(dev)
    if len(sys.argv) > 1 and sys.argv[1] == "--calls":
        x = R.model_input("16x16")[:1, :, :1, :1].expand(int(sys.argv[3]), 4, 512, 512).contiguous().to(dev)
        for _ in range(int(sys.argv[2])):
            net(x)
        torch.cuda.synchronize()
        return
    sdg = {k: (v.to(DTYPE) if v.is_floating_point() else v).to(dev) for k, v in sd.items()}
    L = net._L()
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "clocks_before": clocks(), "shapes": {}}
    for label, shape in SHAPES.items():
        B, _, H, W = shape
        g = torch.Generator().manual_seed(0)
        x = torch.cat([2 * torch.rand((B, 3, H, W), generator=g) - 1, torch.full((B, 1, H, W), 1 / 127.5 - 1)], 1).to(dev)
        xh = x.to(DTYPE)
        torch_call = lambda: R.net(sdg, xh, compute=DTYPE)
        with torch.no_grad():
            got = net(xh)                                         # warm-up: workspace, derived weight copies
            want = torch_call()
            agree = R.max_abs(got.float().cpu(), want.float().cpu())
            ms = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                ms["native"].append(timed(lambda: net(xh), REPS))
                ms["torch"].append(timed(torch_call, REPS))
            per = planner_ms(net, xh)
            split = hook_split(L, B, H, W)
        med = {k: statistics.median(v) for k, v in ms.items()}
        planner = {k: v for k, v in per.items() if k != "other"}
        graph_split = {"planner 3x3 convolutions and 1x1 GEMMs": sum(v["ms"] for v in planner.values()),
                       **{k: v for k, v in split.items() if not k.startswith("(")}}
        r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
             "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
             "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
             "gmac": 25.5 * B * (H * W) / 512 ** 2,
             "split_ms": graph_split, "split_share_of_native": {k: v / med["native"] for k, v in graph_split.items()},
             "planner_classes": planner, "mlsd_kernels_in_the_profiled_call": per.get("other"),
             "relu6_on_the_depthwise_reads_replaces_ms": split["(not in the graph) in-place ReLU6 of the expand outputs"],
             "workspace_gb": net.workspace_bytes(B, H, W, dev) / 2 ** 30, "max_abs_native_vs_torch": agree}
        result["shapes"][label] = r
        print(label, json.dumps(r), flush=True)
    result["clocks_after"] = clocks()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
