"""Dev tool: what one native ControlNet costs next to the UNet it feeds (profiles/README.md, Round 8).  One process, HIP events,
alternating rounds, medians:

  * gyre_ctrl_forward against the UNet forward of the same batch (SD1.5 widths, 64 x 64 latents, batch 16 and 2), the UNet with and
    without the 13 residual inputs (its side of the NCHW hand-off: launch_add_nchw_into_nhwc) and the 13 emits alone on the same
    shapes (the control model's side)
  * the 50-step DPM++2M request (512 x 512, CFG, batch BENCH_B) with and without one ControlNet hint

`python tools/ctrl_time.py [out.json]`; ROUNDS, BENCH_B, STEPS from the environment.  Synthetic N(0, 1/fan_in) weights."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import _lib, config as gcfg
from gyre_amd.controlnet import GyreHipControlNet
from gyre_amd.hints import ControlNetHint
from gyre_amd.modules import GyreHipUNet, GyreHipVAE
from gyre_amd.pipeline import GyrePipeline

dev = "cuda:0"
ROUNDS = int(os.environ.get("ROUNDS", "5"))
BENCH_B = int(os.environ.get("BENCH_B", "8"))
STEPS = int(os.environ.get("STEPS", "50"))


def fill(m):
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.ndim > 1:
                p.copy_(torch.randn(p.shape, device=dev, generator=g, dtype=torch.float32) / p[0].numel() ** 0.5)
            elif k.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    m._invalidate()
    return m


def timeit(fn, iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


unet = fill(GyreHipUNet(gcfg.sd15_unet()).to(torch.bfloat16).to(dev))
vae = fill(GyreHipVAE(gcfg.sd15_vae()).to(torch.bfloat16).to(dev))
ctrl = fill(GyreHipControlNet(gcfg.sd15_controlnet()).to(torch.bfloat16).to(dev))
L = ctrl._L()
result = {"rounds": ROUNDS, "forward": [], "request": {}}

for B in (16, 2):
    x = torch.randn(B, 4, 64, 64, device=dev)
    t = torch.full((B,), 500, device=dev)
    ctx = torch.randn(B, 77, 768, device=dev)
    img = torch.rand(1, 3, 512, 512, device=dev)
    bind_ms = timeit(lambda: ctrl.bind(img, ctx), 2)
    res = [o.clone() for o in ctrl(x, t)]
    feats = [torch.randn(B, o.shape[2] * o.shape[3], o.shape[1], device=dev).to(torch.bfloat16) for o in res]
    st = C.c_void_p(_lib.stream_ptr(torch.device(dev)))

    def emits():
        for f, o in zip(feats, res):
            L.gyre_op_ctrl_emit(st, C.c_void_p(f.data_ptr()), B, o.shape[1], o.shape[2] * o.shape[3], o.shape[1], 0.5, 0,
                                C.c_void_p(o.data_ptr()), _lib.dtype_code(o), B, 0)

    runs = {"ctrl_forward": lambda: ctrl(x, t), "unet_forward": lambda: unet(x, t, encoder_hidden_states=ctx).sample,
            "unet_forward_with_residuals": lambda: unet(x, t, encoder_hidden_states=ctx, down_block_additional_residuals=res[:-1],
                                                        mid_block_additional_residual=res[-1]).sample,
            "emit_x13": emits}
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            ms[k].append(timeit(fn, 5))
    row = {"batch": B, "latents": 64, "bind_ms": bind_ms}
    row.update({k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()})
    result["forward"].append(row)
    print(json.dumps(row), flush=True)

pipe = GyrePipeline(unet, vae, device=dev)
g = torch.Generator().manual_seed(1)
text, unc = torch.randn(BENCH_B, 77, 768, generator=g), torch.randn(BENCH_B, 77, 768, generator=g)
image = torch.rand(1, 3, 512, 512, generator=g)
kw = dict(seeds=list(range(BENCH_B)), text_embeddings=text, uncond_embeddings=unc, height=512, width=512, num_inference_steps=STEPS,
          sampler="dpmpp_2m", hires_fix=False)


def request(hinted):
    hints = [ControlNetHint(ctrl, image.to(dev), weight=1.0, soft_injection=True)] if hinted else None
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    pipe(controlnet_hints=hints, **kw)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


request(False); request(True)                                          # warm-up of every shape
rq = {"plain": [], "one_controlnet_hint": []}
for _ in range(max(2, ROUNDS // 2)):
    rq["plain"].append(request(False))
    rq["one_controlnet_hint"].append(request(True))
result["request"] = {"batch": BENCH_B, "steps": STEPS, "sampler": "dpmpp_2m", "size": 512,
                     **{k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in rq.items()}}
print(json.dumps(result["request"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(result, f, indent=1)
