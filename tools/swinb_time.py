"""Dev tool: the native Swin-B backbone against the same network restated in fp16 PyTorch (profiles/README.md).  One process, HIP events,
alternating rounds, medians after a warm-up call of each, in fp16, at the Swin-B configuration on one 1024 x 1024 image and a batch of 4:

  * native   the module call through GyreHipSwinB
  * torch    torch_net below: the reference's operations (conv2d, layer_norm, pad, roll, the window partition as views, matmul +
             softmax with the gathered bias and the -100 mask, gelu, linear) in fp16 as PyTorch-ROCm runs them
  * split    per kernel class of ONE more native call with the library's per-launch event timing on (the events serialise the
             launches, so the sum is a little above the unprofiled call); k_win12_attn is the only launch of the attention class
  * clocks   `rocm-smi --showclocks` before and after, as text (read only)

`python tools/swinb_time.py [out.json]`; ROUNDS, REPS from the environment.  Seeded weights (tests/swinb_ref.seeded_state_dict)."""
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

import swinb_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.hinters import GyreHipSwinB

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REPS = int(os.environ.get("REPS", "30"))
DTYPE = torch.float16
SHAPES = {"1x1024x1024": (1, 3, 1024, 1024), "4x1024x1024": (4, 3, 1024, 1024)}
WS = 12


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


def torch_net(sd, cfg, x, index):
    """SwinTransformer.forward in the dtype of sd; index: relative_position_index on the device"""
    ln = lambda t, p: F.layer_norm(t, t.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], 1e-5)
    lin = lambda t, p: F.linear(t, sd[p + ".weight"], sd.get(p + ".bias"))
    B, _, H, W = x.shape
    x = F.pad(x, (0, -W % 4, 0, -H % 4))
    t = ln(F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=4).permute(0, 2, 3, 1), "patch_embed.norm")
    outs = [t.permute(0, 3, 1, 2).contiguous()]
    for i, depth in enumerate(cfg["depths"]):
        heads = cfg["num_heads"][i]
        h, w = t.shape[1:3]
        Hp, Wp = -(-h // WS) * WS, -(-w // WS) * WS
        nW = (Hp // WS) * (Wp // WS)
        mask = R.region_mask(Hp, Wp, 6).to(x).unsqueeze(1).unsqueeze(0)
        for j in range(depth):
            p = f"layers.{i}.blocks.{j}"
            shift = 6 if j % 2 else 0
            y = F.pad(ln(t, p + ".norm1"), (0, 0, 0, Wp - w, 0, Hp - h))
            if shift:
                y = torch.roll(y, (-shift, -shift), (1, 2))
            Cc = y.shape[-1]
            yw = y.view(B, Hp // WS, WS, Wp // WS, WS, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, WS * WS, Cc)
            qkv = lin(yw, p + ".attn.qkv").reshape(B * nW, WS * WS, 3, heads, 32).permute(2, 0, 3, 1, 4)
            a = (qkv[0] * 32 ** -0.5) @ qkv[1].transpose(-2, -1)
            a = a + sd[p + ".attn.relative_position_bias_table"][index].view(WS * WS, WS * WS, heads).permute(2, 0, 1).unsqueeze(0)
            if shift:
                a = (a.view(B, nW, heads, WS * WS, WS * WS) + mask).view(-1, heads, WS * WS, WS * WS)
            o = lin((torch.softmax(a, -1) @ qkv[2]).transpose(1, 2).reshape(B * nW, WS * WS, Cc), p + ".attn.proj")
            o = o.view(B, Hp // WS, Wp // WS, WS, WS, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, Cc)
            if shift:
                o = torch.roll(o, (shift, shift), (1, 2))
            t = t + o[:, :h, :w]
            t = t + lin(F.gelu(lin(ln(t, p + ".norm2"), p + ".mlp.fc1")), p + ".mlp.fc2")
        outs.append(ln(t, f"norm{i}").permute(0, 3, 1, 2).contiguous())
        if i < 3:
            t = F.pad(t, (0, 0, 0, w % 2, 0, h % 2))
            t = torch.cat([t[:, 0::2, 0::2], t[:, 1::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 1::2]], -1)
            t = lin(ln(t, f"layers.{i}.downsample.norm"), f"layers.{i}.downsample.reduction")
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


def main():
    cfg = gcfg.swinb_config()
    sd = R.seeded_state_dict(weights.swinb_param_shapes(cfg))
    net = GyreHipSwinB()
    net.load_state_dict(sd, strict=False)
    net = net.to(DTYPE).to(dev)
    sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
    index = R.relative_position_index().view(-1).to(dev)
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "config": "Swin-B: embed 128, depths 2 2 18 2, heads 4 8 16 32, window 12",
              "clocks_before": clocks(), "shapes": {}}
    for label, shape in SHAPES.items():
        x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).to(DTYPE).to(dev)
        torch_call = lambda: torch_net(sdg, cfg, x, index)
        with torch.no_grad():
            got, want = net(x), torch_call()                     # warm-up: workspace, derived weight copies
            agree = [R.rel_l2(a.float().cpu(), b.float().cpu()) for a, b in zip(got, want)]
            del got, want
            ms = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                ms["native"].append(timed(lambda: net(x), REPS))
                ms["torch"].append(timed(torch_call, REPS))
            per = class_ms(net, x)
        med = {k: statistics.median(v) for k, v in ms.items()}
        total = sum(v["ms"] for v in per.values())
        r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
             "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
             "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
             "kernel_classes": per, "kernel_ms_sum": total,
             "win12_attn_share_of_kernel_time": per.get("k_attn", {"ms": 0.0})["ms"] / total,
             "workspace_gb": net.workspace_bytes(shape[0], shape[2], shape[3], dev) / 2 ** 30, "rel_l2_native_vs_torch_per_map": agree}
        result["shapes"][label] = r
        print(label, json.dumps(r), flush=True)
    result["clocks_after"] = clocks()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
