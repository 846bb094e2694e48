"""The Swin-B backbone of InSPyReNet on the native path: an image-shaped tensor through GyreHipSwinB, the module the reference's
``InSPyReNet(backbone, in_channels, depth, base_size, ...)`` takes as its first argument.

    python examples/inspyrenet_backbone.py [--model folder-or-file] [--size 1024] [--batch 1] [--dtype f16]

Without --model the weights are random-init (the run shows the call a background-removal engine makes on its backbone and prints the
five map shapes and the time).  --model takes an InSPyReNet checkpoint (*.pth / *.pt / *.safetensors, or a folder holding exactly
one): its ``backbone.`` keys load strictly, the head's keys are the host module's.  The five maps come back in the module's dtype; a
caller that keeps the head in fp32, as the reference does, casts them."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHipSwinB, load_inspyrenet_backbone

ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
a = ap.parse_args()

if a.model:
    net = load_inspyrenet_backbone(a.model)
else:
    net = GyreHipSwinB()
    net.load_state_dict(weights.synthetic_state_dict({k: s for k, s in weights.swinb_param_shapes(net.config).items()
                                                      if not weights.swinb_is_buffer(k)}, seed=0), strict=False)
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).eval().to("cuda:0")
image = torch.rand((a.batch, 3, a.size, a.size), generator=torch.Generator().manual_seed(0)).to("cuda:0")
net(image)                                         # first call: weight upload, bias expansion, workspace
torch.cuda.synchronize()
t0 = time.time()
maps = net(image)
torch.cuda.synchronize()
ms = (time.time() - t0) * 1e3
print(f"{a.batch} x {a.size} x {a.size} -> " + ", ".join("x".join(map(str, m.shape[1:])) for m in maps) + f" ({maps[0].dtype}) in {ms:.1f} ms")
