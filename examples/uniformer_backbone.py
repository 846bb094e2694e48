"""The UniFormer backbone of the segmentation annotator on the native path: an image-shaped tensor through GyreHipUniFormer, the module
the mmseg segmentor behind the reference's ``hinters-uniformer`` engine takes as its backbone.

    python examples/uniformer_backbone.py [--model folder-or-file] [--variant small] [--size 512] [--batch 1] [--dtype f16]

Without --model the weights are random-init (the run shows the call a segmentation engine makes on its backbone and prints the four map
shapes and the time).  --model takes an mmseg segmentor checkpoint (*.pth / *.pt / *.safetensors, or a folder holding exactly one): its
``backbone.`` keys load strictly, the UPerNet head's keys are the host module's.  The four maps come back in the module's dtype."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHipUniFormer, load_uniformer_backbone

LAYERS = {"small": [3, 4, 8, 3], "base": [5, 8, 20, 7]}
ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--variant", choices=tuple(LAYERS), default="small")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
a = ap.parse_args()

if a.model:
    net = load_uniformer_backbone(a.model, layers=LAYERS[a.variant])
else:
    net = GyreHipUniFormer(layers=LAYERS[a.variant])
    sd = weights.synthetic_state_dict({k: s for k, s in weights.uniformer_param_shapes(net.config).items()
                                       if not weights.uniformer_is_buffer(k)}, seed=0)
    sd.update({k: torch.ones_like(v) for k, v in net.state_dict().items() if k.endswith("running_var")})
    net.load_state_dict(sd, strict=False)
net = net.to(torch.float16 if a.dtype == "f16" else torch.bfloat16).eval().to("cuda:0")
image = torch.rand((a.batch, 3, a.size, a.size), generator=torch.Generator().manual_seed(0)).to("cuda:0")
net(image)                                         # first call: weight upload, BatchNorm folds, workspace
torch.cuda.synchronize()
t0 = time.time()
maps = net(image)
torch.cuda.synchronize()
ms = (time.time() - t0) * 1e3
print(f"{a.batch} x {a.size} x {a.size} -> " + " ".join(str(list(m.shape)).replace(" ", "") for m in maps) + f" ({maps[0].dtype}) in {ms:.1f} ms")
