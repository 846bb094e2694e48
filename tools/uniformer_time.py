"""Dev tool: the native UniFormer backbone against the same network restated in fp16 PyTorch (profiles/README.md).  One process, HIP
events, alternating rounds, medians after a warm-up call of each, in fp16, for uniformer_small and uniformer_base on one 512 x 512 image
and a batch of 4:

  * native   the module call through GyreHipUniFormer
  * torch    torch_net below: the reference module's operations in its own NCHW order - conv2d with its own padding, eval-mode
             batch_norm (one op, nothing folded), layer_norm, linear, matmul + softmax, gelu - on fp16 tensors as PyTorch-ROCm runs
             them, which is what a server without the native path computes; nothing but those operations is inside the timed window
  * split    per kernel class of ONE more native call with the library's per-launch event timing on (the events serialise the
             launches, so the sum is a little above the unprofiled call)
  * local    k_uf_local alone (gyre_op_uf_local on the stage-1 and stage-2 maps of the shape, median of REPS launches each) times the
             blocks that launch it, as a share of the kernel-time sum
  * clocks   `rocm-smi --showclocks` before and after, as text (read only); "before" is an idle card, so only "after" shows the clocks
             the card measured at

`python tools/uniformer_time.py [out.json]`; ROUNDS, REPS from the environment.  Seeded weights (tests/uniformer_ref.seeded_state_dict, matrices
scaled by 0.3: the convolutional blocks have no activation-dependent norm, so the test gain would overflow fp16 at the real depths)."""
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
import torch.nn.functional as F

import uniformer_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hinters import GyreHipUniFormer

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REPS = int(os.environ.get("REPS", "50"))                                 # a timed window of 60 - 180 ms native, 0.25 - 0.8 s torch
DTYPE = torch.float16
SHAPES = {"1x512x512": (1, 3, 512, 512), "4x512x512": (4, 3, 512, 512)}
VARIANTS = {"small": [3, 4, 8, 3], "base": [5, 8, 20, 7]}


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


def torch_net(sd, cfg, x):
    """the four maps of the reference's UniFormer.forward(x) (global attention), operation by operation as its modules run them"""
    conv = lambda t, p, **kw: F.conv2d(t, sd[p + ".weight"], sd[p + ".bias"], **kw)
    bn = lambda t, p: F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.1, R.BN_EPS)
    ln = lambda t, p, eps: F.layer_norm(t, t.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], eps)
    lin = lambda t, p: F.linear(t, sd[p + ".weight"], sd[p + ".bias"])
    outs = []
    for i, depth in enumerate(cfg["layers"]):
        p = f"patch_embed{i + 1}"
        x = conv(x, p + ".proj", stride=4 if i == 0 else 2)
        B, C, H, W = x.shape
        x = ln(x.flatten(2).transpose(1, 2), p + ".norm", 1e-5).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        for j in range(depth):
            p = f"blocks{i + 1}.{j}"
            x = x + conv(x, p + ".pos_embed", padding=1, groups=C)
            if i < 2:
                x = x + conv(conv(conv(bn(x, p + ".norm1"), p + ".conv1"), p + ".attn", padding=2, groups=C), p + ".conv2")
                x = x + conv(F.gelu(conv(bn(x, p + ".norm2"), p + ".mlp.fc1")), p + ".mlp.fc2")
            else:
                t = x.flatten(2).transpose(1, 2)
                q, k, v = lin(ln(t, p + ".norm1", 1e-6), p + ".attn.qkv").reshape(B, H * W, 3, C // 64, 64).permute(2, 0, 3, 1, 4)
                a = ((q @ k.transpose(-2, -1)) * 64 ** -0.5).softmax(dim=-1)
                t = t + lin((a @ v).transpose(1, 2).reshape(B, H * W, C), p + ".attn.proj")
                t = t + lin(F.gelu(lin(ln(t, p + ".norm2", 1e-6), p + ".mlp.fc1")), p + ".mlp.fc2")
                x = t.transpose(1, 2).reshape(B, C, H, W)
        outs.append(ln(x.permute(0, 2, 3, 1), f"norm{i + 1}", 1e-6).permute(0, 3, 1, 2).contiguous())
    return outs


def class_ms(net, x):
    """{class: {ms, launches}} of one call with per-launch event timing"""
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
    return {L.gyre_prof_class_name(k).decode(): {"ms": float(ms[k]), "launches": int(la[k])} for k in range(n) if la[k]}


def local_ms(L, B, h, w, Cn):
    """one k_uf_local launch on a [B, h, w, Cn] map, ms"""
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.randn((B, h, w, Cn), device=dev).to(DTYPE)
    y, wm = torch.empty_like(x), (torch.randn((Cn, Cn), device=dev) / Cn ** 0.5).to(DTYPE)
    v = torch.randn(26 * Cn, device=dev)
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    call = lambda: _lib.check(L.gyre_op_uf_local(st, p(x), Cn, p(y), Cn, B, h, w, Cn, p(wm), p(v), p(v), p(v[25 * Cn:]), p(wm), p(v)), L)
    call()
    return statistics.median(timed(call, REPS) for _ in range(ROUNDS))


def main():
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "clocks_before": clocks(), "variants": {}}
    for name, layers in VARIANTS.items():
        cfg = gcfg.uniformer_config(layers=layers)
        sd = R.seeded_state_dict(weights.uniformer_param_shapes(cfg))
        sd = {k: 0.3 * v if v.ndim >= 2 else v for k, v in sd.items()}       # (the test gain of 1.5 per layer leaves fp16 over 18 - 40 blocks)
        net = GyreHipUniFormer(layers=layers)
        net.load_state_dict(sd, strict=False)
        net = net.to(DTYPE).to(dev)
        sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
        out = result["variants"][name] = {"config": f"layers {layers}, embed 64 128 320 512, head dim 64", "shapes": {}}
        for label, shape in SHAPES.items():
            x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(DTYPE).to(dev)
            torch_call = lambda: torch_net(sdg, cfg, x)
            with torch.no_grad():
                got, want = net(x), torch_call()                     # warm-up: workspace, folds
                agree = [R.rel_l2(a.float().cpu(), b.float().cpu()) for a, b in zip(got, want)]
                del got, want
                ms = {"native": [], "torch": []}
                for _ in range(ROUNDS):
                    ms["native"].append(timed(lambda: net(x), REPS))
                    ms["torch"].append(timed(torch_call, REPS))
                per = class_ms(net, x)
                B, H, W = shape[0], shape[2], shape[3]
                loc = {"stage1": local_ms(net._L(), B, H // 4, W // 4, 64), "stage2": local_ms(net._L(), B, H // 8, W // 8, 128)}
            med = {k: statistics.median(v) for k, v in ms.items()}
            total = sum(v["ms"] for v in per.values())
            loc_total = layers[0] * loc["stage1"] + layers[1] * loc["stage2"]
            r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
                 "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
                 "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
                 "kernel_classes": per, "kernel_ms_sum": total, "uf_local_ms_per_launch": loc, "uf_local_ms_per_call": loc_total,
                 "uf_local_share_of_kernel_time": loc_total / total,
                 "workspace_gb": net.workspace_bytes(B, H, W, dev) / 2 ** 30, "rel_l2_native_vs_torch_per_map": agree}
            out["shapes"][label] = r
            print(name, label, json.dumps(r), flush=True)
    result["clocks_after"] = clocks()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
