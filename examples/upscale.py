"""End-to-end upscaler run on random-init weights: a 4-channel image through GyreUpscalerPipeline over the native RRDBNet, SwinIR or HAT.

    python examples/upscale.py [--network esrgan|swinir|swinir-l|hat|hat-l] [--size 512] [--blocks 23] [--dtype f16] [--out upscaled.png]

Synthetic weights make no picture worth looking at; the run shows the call sequence an engine makes (loader-shaped model, pipeline
call, 9 stacked tiles for 512 x 512) and prints its time."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import config as gcfg, weights
from gyre_amd.upscaler import GyreHipHAT, GyreHipRRDBNet, GyreHipSwinIR, GyreUpscalerPipeline

ap = argparse.ArgumentParser()
ap.add_argument("--network", choices=("esrgan", "swinir", "swinir-l", "hat", "hat-l"), default="esrgan")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--blocks", type=int, default=23, help="RRDBs of the esrgan network")
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.network == "esrgan":
    cfg = gcfg.rrdb_config(num_block=a.blocks)
    net = GyreHipRRDBNet(cfg)
    net.load_state_dict(weights.synthetic_state_dict(weights.rrdb_param_shapes(cfg)))
elif a.network in ("hat", "hat-l"):
    cfg = gcfg.hat_config(**gcfg.HAT_DEFAULTS[a.network])
    net = GyreHipHAT(cfg)
    shapes = {k: v for k, v in weights.hat_param_shapes(cfg).items() if not weights.hat_is_buffer(k)}
    net.load_state_dict(weights.synthetic_state_dict(shapes), strict=False)      # (the buffers keep their zeros: they are never read)
else:
    cfg = gcfg.swinir_config(**gcfg.SWINIR_DEFAULTS[a.network])
    net = GyreHipSwinIR(cfg)
    shapes = {k: v for k, v in weights.swinir_param_shapes(cfg).items() if not weights.swinir_is_buffer(k)}
    net.load_state_dict(weights.synthetic_state_dict(shapes), strict=False)      # (the buffers keep their zeros: they are never read)
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).to("cuda:0").eval()
pipe = GyreUpscalerPipeline(net)
image = torch.rand((1, 4, a.size, a.size), generator=torch.Generator().manual_seed(0)).to("cuda:0")
pipe(image)                                        # first call: weight upload, workspace
torch.cuda.synchronize()
t0 = time.time()
(out,) = pipe(image)
torch.cuda.synchronize()
print(f"{a.size} x {a.size} -> {out.shape[-2]} x {out.shape[-1]} ({out.shape[1]} channels) in {(time.time() - t0) * 1e3:.1f} ms")
if a.out:
    from PIL import Image
    Image.fromarray((out[0].permute(1, 2, 0).clamp(0, 1) * 255).round().byte().cpu().numpy()).save(a.out)
