"""End-to-end line-art hinter run: a photo-shaped tensor through GyreInformativeDrawingPipeline over the native DrawingGenerator.

    python examples/lineart.py [--model folder-or-file] [--size 512] [--blocks 3] [--dtype f16] [--out lineart.png]

Without --model the weights are random-init (synthetic weights make no drawing worth looking at; the run shows the call sequence an
edge_detection engine makes and prints its time).  --model takes a *.pth / *.pt / *.safetensors state dict of the informative-drawings
generator (the files of the reference's hinters-lineart-* engines) or a folder holding exactly one."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHipDrawingGenerator, GyreInformativeDrawingPipeline, load_drawing_generator

ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--blocks", type=int, default=3, help="residual blocks (3: the reference's three engines)")
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.model:
    net = load_drawing_generator(a.model, n_residual_blocks=a.blocks)
else:
    net = GyreHipDrawingGenerator(3, 1, a.blocks)
    net.load_state_dict(weights.synthetic_state_dict(weights.lineart_param_shapes(net.config)))
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).eval()
pipe = GyreInformativeDrawingPipeline(net)
pipe.to("cuda:0")
image = torch.rand((1, 4, a.size, a.size), generator=torch.Generator().manual_seed(0))       # RGBA on the host: the alpha is cut
pipe(image)                                        # first call: weight upload, workspace
torch.cuda.synchronize()
t0 = time.time()
out = pipe(image)
torch.cuda.synchronize()
print(f"{a.size} x {a.size} -> {out.shape[-2]} x {out.shape[-1]} ({out.shape[1]} channel, {out.dtype} on {out.device}) in {(time.time() - t0) * 1e3:.1f} ms")
if a.out:
    from PIL import Image
    Image.fromarray((out[0, 0].clamp(0, 1) * 255).round().byte().cpu().numpy()).save(a.out)
