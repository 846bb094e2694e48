"""Dev tool: the native T2I style adapter and co-adapter fuser against the restated reference networks in PyTorch (profiles/README.md).
One process, HIP events, alternating rounds, medians after a warm-up call of each, in fp16:

  * style    the default StyleAdapter (width 1024, 8 heads, 3 blocks, 8 tokens) on CLIP ViT-L/14 hidden states [1 and 8][257][1024]
  * fuser    the default CoAdapterFuser (width 768, 8 heads of 96, 3 blocks) on two spatial co-adapters plus one style co-adapter at
             512 x 512 (states of 64 / 32 / 16 / 8 pixels a side, 8 style tokens: a sequence of 16)
  * native   the module call through GyreHipT2IStyleAdapter / GyreHipT2IFuser
  * torch    the same call through tests/t2i_seq_ref.style_net / fuser_net in fp16 on the GPU - the reference network's operations as
             PyTorch-ROCm runs them (explicit attention; the reference itself keeps its style models out of fp16)
  * attn     k_seq_attn through its raw-operator hook on the shape of the graph, REPS launches between two events, times the number
             of blocks: its share of the native call

`python tools/t2i_seq_time.py [out.json]`; ROUNDS, REPS from the environment.  Seeded synthetic weights."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import t2i_seq_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.t2i import GyreHipT2IFuser, GyreHipT2IStyleAdapter

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "7"))
REPS = int(os.environ.get("REPS", "10"))
DTYPE = torch.float16
HW_512 = [(64, 64), (32, 32), (16, 16), (8, 8)]


def timed(fn, reps=1):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def attn_ms(L_, N, seq, heads, D):
    W = heads * D
    qkv = torch.randn((N * seq, 3 * W), device=dev).to(DTYPE)
    o = torch.empty((N * seq, W), dtype=DTYPE, device=dev)
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))
    call = lambda: _lib.check(L_.gyre_op_seq_attn(st, C.c_void_p(qkv.data_ptr()), 3 * W, C.c_void_p(o.data_ptr()), W, N, seq, heads, D), L_)
    call()
    return statistics.median(timed(call, REPS) for _ in range(ROUNDS))


def compare(native, torch_call, flatten):
    with torch.no_grad():
        got, want = flatten(native()), flatten(torch_call())
        ms = {"native": [], "torch": []}
        for _ in range(ROUNDS):
            ms["native"].append(timed(native, REPS))
            ms["torch"].append(timed(torch_call, REPS))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"native_ms": {"median": med["native"], "min": min(ms["native"]), "max": max(ms["native"])},
            "torch_ms": {"median": med["torch"], "min": min(ms["torch"]), "max": max(ms["torch"])},
            "torch_over_native": med["torch"] / med["native"], "native_faster": med["native"] < med["torch"],
            "max_abs_native_vs_torch": float((got.float() - want.float()).abs().max()), "rel_l2_native_vs_torch": R.rel_l2(got, want)}


def main():
    result = {"dtype": str(DTYPE), "rounds": ROUNDS, "reps": REPS, "style": {}, "fuser": {}}
    scfg = gcfg.t2i_style_config()
    ssd = weights.synthetic_state_dict(weights.t2i_style_param_shapes(scfg), 31)
    style = GyreHipT2IStyleAdapter(scfg)
    style.load_state_dict(ssd)
    style = style.to(DTYPE).to(dev)
    ssdg = {k: v.to(DTYPE).to(dev) for k, v in ssd.items()}
    for N in (1, 8):
        x = R.style_input(N, 257, scfg["width"]).to(DTYPE).to(dev)
        r = compare(lambda: style(x), lambda: R.style_net(ssdg, scfg, x, compute=DTYPE), lambda t: t)
        a = attn_ms(style._L(), N, 257 + scfg["num_token"], scfg["num_head"], scfg["width"] // scfg["num_head"])
        r["seq_attn_ms_per_launch"], r["seq_attn_share_of_native"] = a, scfg["n_layes"] * a / r["native_ms"]["median"]
        result["style"][f"{N}x257x{scfg['width']}"] = r
        print("style", N, json.dumps(r), flush=True)
    fcfg = gcfg.t2i_fuser_config()
    fsd = weights.synthetic_state_dict(weights.t2i_fuser_param_shapes(fcfg), 32)
    fuser = GyreHipT2IFuser(fcfg)
    fuser.load_state_dict(fsd)
    fuser = fuser.to(DTYPE).to(dev)
    fsdg = {k: v.to(DTYPE).to(dev) for k, v in fsd.items()}
    spec = [("sketch", "spatial", 0, 51), ("style", "tokens", 8, 52), ("depth", "spatial", 0, 53)]
    for N in (1, 8):
        feats = [(n, [m.to(DTYPE).to(dev) for m in v] if isinstance(v, list) else v.to(DTYPE).to(dev))
                 for n, v in R.fuser_inputs(spec, fcfg, N=N, hw=HW_512)]
        flat = lambda out: torch.cat([t.reshape(-1).float() for t in out[0]] + [out[1].reshape(-1).float()])
        r = compare(lambda: fuser(feats), lambda: R.fuser_net(fsdg, fcfg, feats, compute=DTYPE), flat)
        a = attn_ms(fuser._L(), N, 16, fcfg["num_head"], fcfg["width"] // fcfg["num_head"])
        r["seq_attn_ms_per_launch"], r["seq_attn_share_of_native"] = a, fcfg["n_layes"] * a / r["native_ms"]["median"]
        result["fuser"][f"{N}x(2 spatial + 8 style tokens) at 512x512"] = r
        print("fuser", N, json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
