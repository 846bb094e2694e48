"""End-to-end MLSD line-detector run: a photo-shaped tensor through GyreMlsdPipeline over the native MobileV2_MLSD_Large.

    python examples/mlsd.py [--model folder-or-file] [--size 512] [--input-size 512] [--dtype f16] [--out mlsd.png]

Without --model the weights are random-init (seeded weights find no line worth looking at; the run shows the call sequence a hinter
engine makes and prints its time and the number of segments).  --model takes a *.pth / *.pt / *.safetensors state dict of
MobileV2_MLSD_Large (mlsd_large_512_fp32.pth of the upstream project) or a folder holding exactly one."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHipMLSD, GyreMlsdPipeline, load_mlsd

ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--input-size", type=int, default=512)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
ap.add_argument("--out", default=None)
a = ap.parse_args()

if a.model:
    net = load_mlsd(a.model)
    thresholds = dict(score_threshold=0.1, distance_threshold=0.1)
else:
    net = GyreHipMLSD()
    shapes = weights.mlsd_param_shapes()
    sd = weights.synthetic_state_dict(shapes, seed=0)
    g = torch.Generator().manual_seed(0)
    for key, shape in shapes.items():                              # BatchNorm: gains near 1 (4 in front of a ReLU6), variances near 1
        if key.endswith("running_var"):
            bn = key[:-len(".running_var")]
            sd[bn + ".weight"] = (4.0 if bn.endswith(".0.1") else 0.5) * (0.75 + 0.5 * torch.rand(shape, generator=g))
            sd[key] = 0.5 + torch.rand(shape, generator=g)
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros((), dtype=torch.long)
    net.load_state_dict(sd)
    thresholds = dict(score_threshold=0.0, distance_threshold=0.0)           # random maps: draw the top_k maxima, whatever their score
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).eval()
pipe = GyreMlsdPipeline(net, input_size=a.input_size, **thresholds)
pipe.to("cuda:0")
image = torch.rand((1, 4, a.size, a.size), generator=torch.Generator().manual_seed(0))       # RGBA on the host: the alpha is cut
pipe(image)                                        # first call: weight upload, BatchNorm fold, workspace
torch.cuda.synchronize()
t0 = time.time()
out = pipe(image)
torch.cuda.synchronize()
ms = (time.time() - t0) * 1e3
print(f"{a.size} x {a.size} -> {out.shape[-2]} x {out.shape[-1]} ({out.shape[1]} channel, {out.dtype} on {out.device}), "
      f"{pipe.lines(image)[0].shape[0]} segments, {int(out.sum())} pixels drawn, in {ms:.1f} ms")
if a.out:
    from PIL import Image
    Image.fromarray((out[0, 0].clamp(0, 1) * 255).round().byte().cpu().numpy()).save(a.out)
