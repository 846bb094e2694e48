"""Dev tool: the native BAE normal-map decoder against the same decoder restated in fp16 PyTorch (profiles/README.md).  One process, HIP
events, alternating rounds, medians after a warm-up call of each, in fp16, at the real widths (num_features 2048, skips 24 40 64 176)
for the feature maps of one 512 x 512 image (x_block0 256 x 256) and of a batch of 4:

  * native   the module call through GyreHipBaeDecoder (the packing of the five maps into one buffer included)
  * torch    tests/bae_ref.decoder - the reference module's operations in its own order: interpolate, cat, conv2d, eval-mode batch_norm
             (one op, nothing folded), leaky_relu, conv1d over every pixel - on fp16 tensors as PyTorch-ROCm runs them
  * split    per kernel class of ONE more native call with the library's per-launch event timing on (the events serialise the
             launches, so the sum is a little above the unprofiled call); "planner" is every class but the one the element-wise and
             fused kernels are booked under
  * refine   k_bae_refine alone (gyre_op_bae_refine on the three stage shapes, median of REPS launches each), as a share of the
             kernel-time sum
  * clocks   `rocm-smi --showclocks` before and after, as text (read only); "before" is an idle card, so only "after" shows the clocks
             the card measured at

`python tools/bae_time.py [out.json]`; ROUNDS, REPS from the environment.  Seeded weights (tests/bae_ref.seeded_state_dict)."""
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

import bae_ref as R
from gyre_amd import _lib, weights
from gyre_amd.hinters import GyreHipBaeDecoder

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
REPS = int(os.environ.get("REPS", "10"))
DTYPE = torch.float16
SHAPES = {"1x512x512": (1, 256, 256), "4x512x512": (4, 256, 256)}          # (B, x_block0 rows, columns)
_p = lambda t: C.c_void_p(t.data_ptr())


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


def class_ms(L, fn):
    """{class: {ms, launches}} of one call with per-launch event timing"""
    n = L.gyre_prof_num_classes()
    L.gyre_prof_set_mask((1 << n) - 1)
    la, ms, fl, by = (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    torch.cuda.synchronize()
    L.gyre_prof_collect(la, ms, fl, by)                       # drop what earlier calls left
    fn()
    torch.cuda.synchronize()
    L.gyre_prof_collect(la, ms, fl, by)
    L.gyre_prof_set_mask(0)
    return {L.gyre_prof_class_name(k).decode(): {"ms": float(ms[k]), "launches": int(la[k])} for k in range(n) if la[k]}


def refine_call(L, B, h, w, CF):
    """a closure that launches k_bae_refine once on a [B, h, w, CF] map"""
    x, pred = torch.randn((B, h, w, CF), device=dev).to(DTYPE), torch.randn((B, 4, h, w), device=dev)
    w1, w2 = (torch.randn((128, CF + 32), device=dev) / CF ** 0.5).to(DTYPE), (torch.randn((128, 128), device=dev) / 11).to(DTYPE)
    v, out = torch.randn(512, device=dev), torch.empty((B, 4, 2 * h, 2 * w), device=dev)
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    keep = (x, pred, w1, w2, v, out)
    return lambda: _lib.check(L.gyre_op_bae_refine(st, _p(x), CF, _p(pred), B, h, w, CF, _p(w1), _p(v), _p(w2), _p(v), _p(w2), _p(v), _p(v),
                                                   _p(v), 1, _p(out)), L) or keep


def main():
    net = GyreHipBaeDecoder("BN")
    cfg = net.config
    sd = R.seeded_state_dict(weights.bae_param_shapes(cfg))
    net.load_state_dict(sd, strict=False)
    net = net.to(DTYPE).to(dev)
    L = net._L()
    sdg = {k: v.to(DTYPE).to(dev) for k, v in sd.items()}
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "clocks_before": clocks(),
              "config": f"num_features {cfg.num_features}, skips {list(cfg.skip_features)}", "shapes": {}}
    for label, (B, H, W) in SHAPES.items():
        blocks = [b.to(DTYPE).to(dev) for b in R.seeded_blocks(cfg, B, H, W)]
        feats = [None] * 12
        for i, b in zip(net.BLOCKS, blocks):
            feats[i] = b
        torch_call = lambda: R.decoder(sdg, blocks)
        with torch.no_grad():
            got, want = net(feats)[0], torch_call()                  # warm-up: workspace, folds
            agree = [R.rel_l2(a.float().cpu(), b.float().cpu()) for a, b in zip(got, want)]
            del got, want
            ms = {"native": [], "torch": []}
            for _ in range(ROUNDS):
                ms["native"].append(timed(lambda: net(feats), REPS))
                ms["torch"].append(timed(torch_call, REPS))
            per = class_ms(L, lambda: net(feats))
            stages = {f"res{8 >> (s + 1)}": refine_call(L, B, (H // 4) << s, (W // 4) << s, cfg.num_features >> (s + 2)) for s in range(3)}
            own = next(iter(class_ms(L, stages["res4"])))                # the class the fused and element-wise kernels are booked under
            ref = {}
            for k, call in stages.items():
                call()
                ref[k] = statistics.median(timed(call, REPS) for _ in range(ROUNDS))
        med = {k: statistics.median(v) for k, v in ms.items()}
        total = sum(v["ms"] for v in per.values())
        planner = total - per.get(own, {"ms": 0.0})["ms"]
        r = {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
             "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
             "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
             "kernel_classes": per, "kernel_ms_sum": total, "planner_ms": planner, "planner_share_of_kernel_time": planner / total,
             "bae_refine_ms_per_launch": ref, "bae_refine_ms_per_call": sum(ref.values()),
             "bae_refine_share_of_kernel_time": sum(ref.values()) / total,
             "workspace_gb": net.workspace_bytes(B, H, W, dev) / 2 ** 30, "rel_l2_native_vs_torch_per_map": agree}
        result["shapes"][label] = r
        print(label, json.dumps(r), flush=True)
    result["clocks_after"] = clocks()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
