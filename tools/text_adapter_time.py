"""Request-time cost of a text-encoder LoRA: attach + detach of a rank-32 kohya LoRA over all 72 Linear weights of a CLIP-L-sized
synthetic text encoder (hidden 768, 12 layers), on the device path of gyre_amd/text_adapters.py (one gyre_op_merge_delta per weight,
factors uploaded beforehand) beside the same merge done with torch ops (``W + s * up @ down`` per module, and a copy back).

usage: python tools/text_adapter_time.py [--rank 32] [--reps 20] [--dtype float16] [--out profiles/text_adapter_request_time.json]

Timed with device events around the calls, after two warm-up rounds of each path; the two paths alternate inside one process, the
median and the spread (min, max) of ``reps`` rounds are written.  Needs the GPU: no number is produced without one.  Nothing is
asserted about the time - the paths are checked to give the same weights (lattice-free data: equal within one rounding of the
encoder's dtype) and detach to restore the base bits."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gyre_amd import text_adapters as TA  # noqa: E402
from gyre_amd.text import ClipTextEncoder  # noqa: E402

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", default="float16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_adapter_request_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_adapter_time: needs the GPU (a CPU timing says nothing about it)")
    dev, dtype = torch.device("cuda:0"), getattr(torch, a.dtype)
    te = ClipTextEncoder.synthetic(device=dev, dtype=dtype).model
    tower = getattr(te, "text_model", te)
    g = torch.Generator().manual_seed(0)
    lora, mods = {}, []
    for i, layer in enumerate(tower.encoder.layers):
        for name in LINEARS:
            m = layer
            for part in name.split("."):
                m = getattr(m, part)
            O, I = m.weight.shape
            k = f"lora_te_text_model_encoder_layers_{i}_{name.replace('.', '_')}"
            lora[k + ".lora_up.weight"] = torch.randn(O, a.rank, generator=g) * 0.05
            lora[k + ".lora_down.weight"] = torch.randn(a.rank, I, generator=g) * 0.05
            lora[k + ".alpha"] = torch.tensor(a.rank / 2.0)
            mods.append((m, k))
    base = {m: m.weight.data.clone() for m, _ in mods}
    f = TA.upload_text_factors(te, lora, dev)
    assert len(f) == len(mods) == 72
    pairs = [(m, lora[k + ".lora_up.weight"].to(dev), lora[k + ".lora_down.weight"].to(dev), 0.5 * 0.8) for m, k in mods]

    def native():
        TA.attach(te, [(f, 0.8)])
        TA.detach(te)

    def torch_ops():
        kept = []
        for m, up, down, s in pairs:
            w = m.weight.data
            kept.append((w, w.clone()))
            w.copy_((w.float() + s * (up @ down)).to(w.dtype))
        for w, b in kept:
            w.copy_(b)

    # the two paths give the same weights (within one rounding: torch rounds the fp32 product before the sum), detach restores the bits
    TA.attach(te, [(f, 0.8)])
    got = {m: m.weight.data.clone() for m, _ in mods}
    TA.detach(te)
    restored = all(torch.equal(m.weight.data, base[m]) for m, _ in mods)
    worst = 0.0
    for m, up, down, s in pairs:
        want = (base[m].float() + s * (up @ down)).to(dtype)
        worst = max(worst, float(((got[m].float() - want.float()).abs() / want.float().abs().clamp_min(1e-3)).max()))
    ulp = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}[dtype]
    assert restored, "detach did not restore the base bits"
    agree = worst <= 2 * ulp

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(2):
        native(), torch_ops()
    torch.cuda.synchronize()
    t = {"native": [], "torch_ops": []}
    for _ in range(a.reps):                                               # alternating, same process
        t["native"].append(timed(native))
        t["torch_ops"].append(timed(torch_ops))
    stat = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    flops = sum(2.0 * m.weight.shape[0] * m.weight.shape[1] * a.rank for m, _ in mods)
    result = {"what": "attach + detach of one kohya LoRA over every Linear weight of a synthetic CLIP-L text encoder, device events around the calls",
              "encoder": "hidden 768, 12 layers, 72 Linear weights", "dtype": a.dtype, "rank": a.rank, "reps": a.reps,
              "device": torch.cuda.get_device_name(0), "merge_flop_per_attach": flops,
              "native_merge_delta": stat(t["native"]), "torch_ops": stat(t["torch_ops"]),
              "native_over_torch_median": statistics.median(t["native"]) / statistics.median(t["torch_ops"]),
              "worst_relative_difference_of_the_two_merges": worst, "merges_agree_within_two_ulp": agree, "base_restored_bit_exact": restored}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
