"""The decoder of the BAE surface-normal estimator on the native path: the five feature maps an EfficientNet-B5 encoder produces for an
image, through GyreHipBaeDecoder - the heavy half of the network behind the reference's ``hinters-baenormal`` engine.

    python examples/baenormal_decoder.py [--model folder-or-file] [--size 512] [--batch 1] [--dtype f16]

Without --model the weights are random-init.  --model takes an NNET checkpoint (*.pt / *.pth / *.safetensors, or a folder holding exactly
one): its ``decoder.`` keys load strictly.  Either way the feature maps are random tensors of the encoder's shapes - the encoder is the
host module the caller supplies (gyre_amd.hinters.GyreHipNNET / load_baenormal take it) - so the run shows the call and its time, not a
normal map.  --size is the image's side (a multiple of 8); x_block0 is half of it."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gyre_amd import weights
from gyre_amd.hinters import GyreHipBaeDecoder, _load_weights

ap = argparse.ArgumentParser()
ap.add_argument("--model", default=None)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--dtype", choices=("bf16", "f16"), default="f16")
a = ap.parse_args()

net = GyreHipBaeDecoder("BN")
if a.model:
    net = _load_weights(net, a.model, None, None, None, prefix="decoder", unwrap="model")
else:
    sd = weights.synthetic_state_dict({k: s for k, s in weights.bae_param_shapes(net.config).items() if not weights.bae_is_buffer(k)}, seed=0)
    sd.update({k: torch.ones_like(v) for k, v in net.state_dict().items() if k.endswith("running_var")})
    net.load_state_dict(sd, strict=False)
dtype = torch.float16 if a.dtype == "f16" else torch.bfloat16
net = net.to(dtype).eval().to("cuda:0")
g = torch.Generator().manual_seed(0)
features = [None] * 12
for i, s in zip(net.BLOCKS, net.block_shapes(a.batch, a.size // 2, a.size // 2)):
    features[i] = torch.randn(s, generator=g).to(dtype).to("cuda:0")
net(features)                                      # first call: weight upload, BatchNorm folds, workspace
torch.cuda.synchronize()
t0 = time.time()
maps = net(features)[0]
torch.cuda.synchronize()
ms = (time.time() - t0) * 1e3
print(f"{a.batch} x {a.size} x {a.size} -> " + " ".join(str(list(m.shape)).replace(" ", "") for m in maps) + f" ({maps[0].dtype}) in {ms:.1f} ms")
