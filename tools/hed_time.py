"""Dev tool: the native HED edge detector against the restated reference network in PyTorch (profiles/README.md).  One process, HIP
events, alternating rounds, medians after a warm-up call of each, in fp16, on one 512 x 512 image and on a batch of 8:

  * native   the module call through GyreHipHED
  * torch    the same call through tests/hed_ref.net in fp16 on the GPU - the reference network's operations as PyTorch-ROCm runs
             them, which is what a server without the native path computes
  * split    per kernel family, its time and its share of the native call: the planner convolutions from ONE more call with the
             library's per-launch event timing on (the events serialise the launches, so their sum is a little above their share of
             the unprofiled call); the in-place ReLU passes, the entry pass, the five stage tails and the fuse kernel each through its
             raw-operator hook on the shapes of the graph, REPS launches between two events
  * tail     bytes moved (the stage's last convolution read once, the pooled tensor and the fp32 scores written) over its time,
             against the device's streaming rate, measured in the same run as a device copy of 512 MiB (read + write bytes over time).
             The hook is launched REPS times over the same tensors: whatever fits the 256 MiB Infinity Cache is served from it, so the
             rate is an upper bound of what the kernel reaches inside the graph, where its input was just written by a convolution

`python tools/hed_time.py [out.json]`; ROUNDS, REPS from the environment.  Seeded weights (tests/hed_ref.model_weights)."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import hed_ref as R
from gyre_amd import _lib
from gyre_amd.hinters import GyreHipHED

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REPS = int(os.environ.get("REPS", "10"))
DTYPE = torch.float16
SHAPES = {"1x512x512": (1, 3, 512, 512), "8x512x512": (8, 3, 512, 512)}


def flops(B, H, W):
    """multiply-adds x 2 of the thirteen convolutions of one call"""
    hs, ws, total, cin = R.stage_sizes(H), R.stage_sizes(W), 0.0, 3
    for k, (n, width) in enumerate(R.STAGES):
        for _ in range(n):
            total += 2.0 * B * hs[k] * ws[k] * 9 * cin * width
            cin = width
    return total


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
    """(ms, launches) of the GEMM / convolution classes in one call with per-launch event timing; the three HED kernels are 'other'"""
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
    conv = [k for k in range(n) if la[k] and L.gyre_prof_class_name(k).decode() != "other"]
    other = [k for k in range(n) if la[k] and L.gyre_prof_class_name(k).decode() == "other"]
    if sum(int(la[k]) for k in other) != 7:
        raise SystemExit(f"the split no longer matches the graph: {sum(int(la[k]) for k in other)} launches in class 'other', expected entry + 5 tails + fuse")
    return sum(float(ms[k]) for k in conv), sum(int(la[k]) for k in conv), sum(float(ms[k]) for k in other)


def hook_split(L, B, H, W):
    """{family: ms} of the kernels that are not planner convolutions, each through its hook on the graph's shapes (any values)"""
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    hs, ws = R.stage_sizes(H), R.stage_sizes(W)
    out = {"in-place ReLU passes": 0.0, "entry": 0.0, "tail": 0.0, "fuse": 0.0}
    tail_bytes, tails = 0.0, []
    x = torch.rand((B, 3, H, W), device=dev)
    x8 = torch.empty((B, hs[0], ws[0], 8), dtype=DTYPE, device=dev)
    out["entry"] = median_ms(lambda: _lib.check(L.gyre_op_hed_entry(st, C.c_void_p(x.data_ptr()), 0, B, H, W, C.c_void_p(x8.data_ptr())), L))
    so = []
    for k, (n, width) in enumerate(R.STAGES):
        t = torch.randn((B, hs[k], ws[k], width), device=dev).to(DTYPE)
        relu = median_ms(lambda: _lib.check(L.gyre_op_relu(st, C.c_void_p(t.data_ptr()), t.numel()), L))
        out["in-place ReLU passes"] += (n - 1) * relu
        t = torch.randn((B, hs[k], ws[k], width), device=dev).to(DTYPE)
        w, b = torch.randn(width, device=dev) / width ** 0.5, torch.zeros(1, device=dev)
        pool = torch.empty((B, -(-hs[k] // 2), -(-ws[k] // 2), width), dtype=DTYPE, device=dev) if k < 4 else None
        s = torch.empty((B, hs[k], ws[k]), dtype=torch.float32, device=dev)
        ms = median_ms(lambda: _lib.check(L.gyre_op_hed_tail(st, C.c_void_p(t.data_ptr()), B, hs[k], ws[k], width, C.c_void_p(w.data_ptr()),
                                                             C.c_void_p(b.data_ptr()), C.c_void_p(pool.data_ptr()) if k < 4 else None,
                                                             C.c_void_p(s.data_ptr())), L))
        nbytes = t.numel() * 2 + (pool.numel() * 2 if k < 4 else 0) + s.numel() * 4
        tails.append({"stage": k + 1, "ms": ms, "bytes": nbytes, "tb_per_s": nbytes / ms / 1e9})
        out["tail"] += ms
        tail_bytes += nbytes
        so.append(s)
    wf, bf = torch.tensor(R.FUSE_WEIGHTS, device=dev), torch.full((1,), R.FUSE_BIAS, device=dev)
    res = torch.empty((6, B, 1, H, W), dtype=DTYPE, device=dev)
    a = _lib.HedFuseArgs(wf=wf.data_ptr(), bf=bf.data_ptr(), out=res.data_ptr(), out_dtype=_lib.F16, B=B, H=H, W=W)
    oy, ox = R.crop_offsets(H), R.crop_offsets(W)
    for k in range(5):
        a.so[k], a.Hk[k], a.Wk[k], a.oy[k], a.ox[k] = so[k].data_ptr(), hs[k], ws[k], oy[k], ox[k]
    out["fuse"] = median_ms(lambda: _lib.check(L.gyre_op_hed_fuse(st, C.byref(a)), L))
    return out, tails, tail_bytes


def streaming_rate(L):
    """TB/s of a device copy of 512 MiB: bytes read + bytes written over time"""
    n = 512 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    ms = median_ms(lambda: _lib.check(L.gyre_op_copy_probe(st, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n), L))
    return 2.0 * n / ms / 1e9


def main():
    sd = R.model_weights()
    net = GyreHipHED()
    net.load_state_dict(sd)
    net = net.to(DTYPE).to(dev)
    sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
    L = net._L()
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "streaming_tb_per_s": streaming_rate(L), "shapes": {}}
    for label, shape in SHAPES.items():
        B, _, H, W = shape
        x = ((torch.rand(shape, generator=torch.Generator().manual_seed(0)) - 0.45) * 255).to(dev)
        xh = x.to(DTYPE)
        torch_call = lambda: R.net(sdg, xh, compute=DTYPE)
        with torch.no_grad():
            got = net(x)                                          # warm-up: workspace, derived weight copies
            want = torch_call()
            agree = [R.max_abs(a.float().cpu(), b.float().cpu()) for a, b in zip(got, want)]
            ms = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                ms["native"].append(timed(lambda: net(x)))
                ms["torch"].append(timed(torch_call))
            conv_ms, conv_launches, other_ms = planner_ms(net, x)
            split, tails, tail_bytes = hook_split(L, B, H, W)
        med = {k: statistics.median(v) for k, v in ms.items()}
        split = {"planner convolutions": conv_ms, **split}
        fl = flops(B, H, W)
        r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
             "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
             "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
             "tflop": fl / 1e12, "native_tflops": fl / med["native"] / 1e9,
             "split_ms": split, "split_share_of_native": {k: v / med["native"] for k, v in split.items()},
             "planner_launches": conv_launches, "entry_tail_fuse_ms_in_the_profiled_call": other_ms,
             "tail": {"stages": tails, "bytes": tail_bytes, "tb_per_s": tail_bytes / split["tail"] / 1e9,
                      "share_of_streaming_rate": tail_bytes / split["tail"] / 1e9 / result["streaming_tb_per_s"]},
             "workspace_gb": net.workspace_bytes(B, H, W, dev) / 2 ** 30, "max_abs_native_vs_torch_per_map": agree}
        result["shapes"][label] = r
        print(label, json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
