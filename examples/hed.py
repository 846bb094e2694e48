"""End-to-end HED edge-detector run: a photo-shaped tensor through GyreHedPipeline over the native HED.

    python examples/hed.py [--model folder-or-file] [--size 512] [--dtype f16] [--out hed.png]

Without --model the weights are random-init (seeded He-scaled weights make no edge map worth looking at; the run shows the call
sequence an edge_detection engine makes and prints its time).  --model takes a *.pth / *.pt / *.safetensors state dict of HED (the
file of the reference's hinters-hed engines) or a folder holding exactly one."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHedPipeline, GyreHipHED, load_hed

ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.model:
    net = load_hed(a.model)
else:
    net = GyreHipHED()
    g = torch.Generator().manual_seed(0)
    sd = {}
    for key, shape in weights.hed_param_shapes().items():           # He-scaled convolutions, small side scores: maps that are not flat
        fan_in = shape[1] * shape[2] * shape[3] if len(shape) == 4 else 1
        scale = 0.5 if key.endswith(".bias") else (2.0 / fan_in) ** 0.5 / (80 if key.startswith("score_dsn") else 1)
        sd[key] = torch.randn(shape, generator=g) * scale
    sd["score_final.weight"] = torch.tensor([0.31, -0.27, 0.34, -0.29, 0.3]).reshape(1, 5, 1, 1)
    net.load_state_dict(sd)
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).eval()
pipe = GyreHedPipeline(net)
pipe.to("cuda:0")
image = torch.rand((1, 4, a.size, a.size), generator=torch.Generator().manual_seed(0))       # RGBA on the host: the alpha is cut
pipe(image)                                        # first call: weight upload, workspace
torch.cuda.synchronize()
t0 = time.time()
out = pipe(image)
torch.cuda.synchronize()
print(f"{a.size} x {a.size} -> {out.shape[-2]} x {out.shape[-1]} ({out.shape[1]} channel, {out.dtype} on {out.device}, "
      f"range {float(out.min()):.2f} .. {float(out.max()):.2f}) in {(time.time() - t0) * 1e3:.1f} ms")
if a.out:
    from PIL import Image
    Image.fromarray((out[0, 0].clamp(0, 1) * 255).round().byte().cpu().numpy()).save(a.out)
