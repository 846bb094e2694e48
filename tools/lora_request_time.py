"""What a per-request LoRA costs around the generation: wall time from "request starts" to "first UNet call returned", for a LoRA
request and for the plain request that follows it, on the host-merge path (lora.apply_lora / remove_lora_from_model) and on the
device path (lora.attach_lora / detach_loras) - same process, same GPU, same SD1.5 UNet with synthetic weights, a kohya-ss LoRA
over every attention, feed-forward and convolution weight.

usage: python tools/lora_request_time.py [--kind lora,loha,lokr,locon_tucker] [--ranks 4,32,128] [--reps 5] [--limit 600]
                                          [--dtype bfloat16] [--no-host] [--out FILE.json]

--kind (one or several, default lora): the same targets and ranks as a LyCORIS file - loha (two low-rank products per weight), lokr
(dense w1 of near-square-root factors, low-rank w2) or locon_tucker (a mid core on every 3 x 3 convolution, plain LoCon elsewhere) -
through lycoris.apply_lycoris / upload_factors / attach_lycoris.  The yardstick of a LyCORIS kind is the LoRA device path of the
SAME run (name lora first).  --no-host skips the host-merge path (device_faster is then not judged).

Per rank and path: one warm-up, then the median of --reps.  A request here is what the engine does before its first UNet call
(gyre_amd/engine.py): strip what the previous request left, apply this request's LoRA, call the UNet (batch 2, 64 x 64 latents,
the CFG pair of one 512 x 512 image).  The tensors mapping stays loaded between requests, as the server's manager keeps it: the
device path uploads its factors once (reported as upload_s), the host path multiplies them out on every request because that
is what it does.  kernel_ms is the fused repack kernels' own time for one attach (gyre_prof_*, HIP events; the median of three
attaches; LyCORIS launches are accounted in the same class).  Every timed step
runs under its own time limit (--limit seconds, SIGALRM): a step that overruns ends the script, nothing more is started.
The alarm is delivered between Python byte codes only: it ends a step that is slow, not one that is blocked inside a native call
(a hung hipStreamSynchronize).  Run the script itself under an outer limit that can kill it, e.g.
``timeout -k 10 900 python tools/lora_request_time.py``.
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gyre_amd import _lib, lora as LR, lycoris as LC
from gyre_amd.modules import GyreHipUNet

DEV = torch.device("cuda:0")


def kohya_all(unet, rank, seed=0):
    g = torch.Generator().manual_seed(seed)
    out, n = {}, 0
    for name, w in unet.named_parameters():
        if not name.endswith(".weight") or not (w.ndim == 4 or (w.ndim == 2 and ".attentions." in name)):
            continue
        k = "lora_unet_" + name[:-len(".weight")].replace(".", "_")
        O, I = w.shape[:2]
        tail = tuple(w.shape[2:])
        out[k + ".lora_down.weight"] = (torch.randn(rank, I, *tail, generator=g) * 0.02).to(torch.float16)
        out[k + ".lora_up.weight"] = (torch.randn(O, rank, *([1, 1] if tail else []), generator=g) * 0.02).to(torch.float16)
        out[k + ".alpha"] = torch.tensor(float(rank) / 2)
        n += 1
    return out, n


def _split(n):
    """n = a * b with a the largest divisor <= sqrt(n) (LyCORIS' default factorization of a LoKr)"""
    a = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return a, n // a


def lyco_all(unet, rank, kind, seed=0):
    """The targets of kohya_all as a LyCORIS file of one kind, fp16 tensors."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: (torch.randn(*s, generator=g) * 0.02).to(torch.float16)
    out, n = {}, 0
    for name, w in unet.named_parameters():
        if not name.endswith(".weight") or not (w.ndim == 4 or (w.ndim == 2 and ".attentions." in name)):
            continue
        k = "lora_unet_" + name[:-len(".weight")].replace(".", "_")
        O, I = w.shape[:2]
        tail = tuple(w.shape[2:])
        kk = w[0, 0].numel()
        if kind == "loha":
            for side in ("1", "2"):
                out[f"{k}.hada_w{side}_a"], out[f"{k}.hada_w{side}_b"] = rn(O, rank) * 8, rn(rank, I * kk) * 8
        elif kind == "lokr":
            (O1, O2), (I1, I2) = _split(O), _split(I)
            out[k + ".lokr_w1"], out[k + ".lokr_w2_a"], out[k + ".lokr_w2_b"] = rn(O1, I1) * 8, rn(O2, rank), rn(rank, I2 * kk)
        elif kk > 1:                                     # locon_tucker
            out[k + ".lora_up.weight"], out[k + ".lora_down.weight"], out[k + ".lora_mid.weight"] = \
                rn(O, rank, 1, 1), rn(rank, I, 1, 1), rn(rank, rank, *tail) * 8
        else:
            out[k + ".lora_up.weight"], out[k + ".lora_down.weight"] = rn(O, rank, *([1, 1] if tail else [])), rn(rank, I, *tail)
        out[k + ".alpha"] = torch.tensor(float(rank) / 2)
        n += 1
    return out, n


class StepLimit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _fire(self, *_):
        raise TimeoutError(f"step '{self.what}' exceeded its {self.seconds} s limit")

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="lora")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--ranks", default="4,32,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dtype = getattr(torch, a.dtype)
    unet = GyreHipUNet().load_synthetic().to(DEV, dtype)
    _lib.set_default_storage(unet._storage())            # the profiler helpers talk to the library this module runs in
    x = torch.randn(2, 4, 64, 64, device=DEV, dtype=dtype)
    t = torch.tensor([500, 500], device=DEV)
    ctx = torch.randn(2, 77, unet.config.cross_attention_dim, device=DEV, dtype=dtype)

    def first_call():
        out = unet(x, t, encoder_hidden_states=ctx).sample
        torch.cuda.synchronize()
        return out

    def timed(what, fn):
        with StepLimit(a.limit, what):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

    with StepLimit(a.limit, "first upload"):
        base = first_call().clone()
    result = {"config": "sd15 unet, synthetic weights", "dtype": a.dtype, "reps": a.reps, "batch": 2, "latent": 64,
              "device": torch.cuda.get_device_name(0), "kinds": {}}
    kinds = a.kind.split(",")
    for kind in kinds:
        if kind not in ("lora", "loha", "lokr", "locon_tucker"):
            ap.error(f"unknown --kind {kind}")
    for kind, rank in [(k, int(r)) for k in kinds for r in a.ranks.split(",")]:
        tensors, nkeys = kohya_all(unet, rank) if kind == "lora" else lyco_all(unet, rank, kind)
        apply, upload = (LR.apply_lora, LR.upload_factors) if kind == "lora" else (LC.apply_lycoris, LC.upload_factors)
        row = {"touched_weights": nkeys}
        # ---- host path (code unchanged): merge on the CPU, re-upload every tensor, twice per LoRA request ----
        def host_lora():
            LR.remove_lora_from_model(unet)
            apply(unet, tensors, "request-0", 1.0)
            return first_call()

        def host_plain():
            LR.remove_lora_from_model(unet)
            return first_call()
        lo, pl = [], []
        for i in range(0 if a.no_host else a.reps + 1):
            tl = timed(f"host {kind} r{rank}", host_lora)
            tp = timed(f"host plain r{rank}", host_plain)
            if i:
                lo.append(tl); pl.append(tp)
        if not a.no_host:
            row["host"] = {"lora_request_s": statistics.median(lo), "next_plain_request_s": statistics.median(pl)}
        # ---- device path: factors uploaded once, touched keys re-issued through the fused repack kernel ----
        with StepLimit(a.limit, f"factor upload r{rank}"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            factors = upload(unet, tensors, DEV)
            torch.cuda.synchronize()
            row["upload_s"] = time.perf_counter() - t0

        def dev_lora():
            LR.detach_loras(unet)
            LR.attach_lora(unet, factors, "request-0", 1.0)
            return first_call()

        def dev_plain():
            LR.detach_loras(unet)
            return first_call()
        lo, pl = [], []
        for i in range(a.reps + 1):
            tl = timed(f"device {kind} r{rank}", dev_lora)
            tp = timed(f"device plain r{rank}", dev_plain)
            if i:
                lo.append(tl); pl.append(tp)
        row["device"] = {"lora_request_s": statistics.median(lo), "next_plain_request_s": statistics.median(pl)}
        with StepLimit(a.limit, f"kernel time r{rank}"):
            ks = []
            for _ in range(3):                           # median of three profiled attaches: a single one can catch a stall
                LR.detach_loras(unet)
                _lib.prof_enable(["k_repack_lora"])
                LR.attach_lora(unet, factors, "request-0", 1.0)
                torch.cuda.synchronize()
                ks.append(_lib.prof_collect().get("k_repack_lora", {"ms": 0.0, "launches": 0, "flops": 0.0}))
                _lib.prof_enable([])
            k = sorted(ks, key=lambda r: r["ms"])[1]
            restored = dev_plain()
        row["device"]["kernel_ms"] = k["ms"]
        row["device"]["kernel_launches"] = k["launches"]
        row["device"]["kernel_tflops"] = k["flops"] / max(k["ms"], 1e-9) / 1e9
        row["device"]["kernel_share_of_lora_request"] = k["ms"] / 1e3 / row["device"]["lora_request_s"]
        row["device_faster"] = None if a.no_host else bool(row["device"]["lora_request_s"] < row["host"]["lora_request_s"]
                                                           and row["device"]["next_plain_request_s"] < row["host"]["next_plain_request_s"])
        row["base_restored_bit_exact"] = bool(torch.equal(restored, base))
        result["kinds"].setdefault(kind, {})[str(rank)] = row
        print(json.dumps({kind: {str(rank): row}}), flush=True)
    if "lora" in result["kinds"]:
        result["ranks"] = result["kinds"]["lora"]            # (the layout of profiles/lora_request_time.json)
    for kind, rows in result["kinds"].items():              # each LyCORIS kind against the LoRA device path of this run
        for rank, row in rows.items():
            ref = result["kinds"].get("lora", {}).get(rank)
            if kind != "lora" and ref:
                row["vs_lora_device"] = {"kernel_ms_ratio": row["device"]["kernel_ms"] / max(ref["device"]["kernel_ms"], 1e-9),
                                         "request_s_ratio": row["device"]["lora_request_s"] / ref["device"]["lora_request_s"]}
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    rows = [r for rows in result["kinds"].values() for r in rows.values()]
    return 0 if all(r["device_faster"] is not False and r["base_restored_bit_exact"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
