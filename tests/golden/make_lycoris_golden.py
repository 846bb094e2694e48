"""Generate tests/golden/lycoris_vectors.npz by running the REFERENCE's own LyCORIS code (gyre/pipeline/lycoris.py: apply_lycoris
and LycorisHook._calc_updown) over a tiny nn.Module tree, with the stubs of make_golden._install().

Runs only in the build container (needs the reference checkout, which does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lycoris_golden.py

For every entry of ENTRIES a one-module file is built from tests/lyco_ref.lattice_fields (seeded lattice tensors: every value the
reference computes from them is exact in fp32, so the recorded deltas must be reproduced bit for bit), applied under its own id
with user scale 0.5, and the delta ``updown * file scale * user scale`` the hook would add is recorded together with the seed, the
keys and the class name of the reference's module object.  tests/test_lycoris_host.py rebuilds the same tensors from the seeds.
"""
import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import lyco_ref as LY  # noqa: E402

USER_SCALE = 0.5
# (module path, form, arguments of lyco_ref.lattice_fields): every supported form on a Linear, a 3x3 and a 1x1 convolution where it
# exists there, and every rule for the file scale
K_LIN, K_CONV = dict(kron=(3, 2)), dict(kron=(2, 2))
ENTRIES = [
    ("lin", "lora", dict(rank=2)),
    ("lin", "lora", dict(rank=2, scale_rule="scale")),
    ("lin", "lora", dict(rank=2, scale_rule="scale0")),
    ("lin", "lora", dict(rank=2, scale_rule="none")),
    ("block.conv1", "lora", dict(rank=3)),
    ("block.proj_in", "lora", dict(rank=2)),
    ("block.conv1", "locon_mid", dict(rank=3)),
    ("block.to_q", "loha", dict(rank=2)),
    ("block.to_q", "loha", dict(rank=3, rank2=2, scale_rule="scale")),
    ("block.conv1", "loha", dict(rank=2)),
    ("block.conv1", "loha_t", dict(rank=3)),
    ("block.proj_in", "loha", dict(rank=2, scale_rule="none")),
    ("lin", "lokr_dense", K_LIN),
    ("lin", "lokr_dense", dict(scale_rule="none", **K_LIN)),
    ("lin", "lokr_lowrank", dict(rank=2, **K_LIN)),
    ("lin", "lokr_w1_lowrank", dict(rank=2, **K_LIN)),
    ("block.conv1", "lokr_dense", K_CONV),
    ("block.conv1", "lokr_lowrank", dict(rank=2, **K_CONV)),
    ("block.conv1", "lokr_t", dict(rank=3, **K_CONV)),
    ("block.proj_in", "lokr_lowrank", dict(rank=2, scale_rule="scale", **K_CONV)),
    ("lin", "full", {}),
    ("block.conv1", "full", {}),
]


def tree():
    """The module tree both sides use: names and shapes only matter."""
    torch.manual_seed(0)
    net = torch.nn.Module()
    net.lin = torch.nn.Linear(8, 12)
    net.block = torch.nn.Module()
    net.block.to_q = torch.nn.Linear(8, 8, bias=False)
    net.block.conv1 = torch.nn.Conv2d(4, 6, 3, padding=1)
    net.block.proj_in = torch.nn.Conv2d(4, 6, 1)
    return net


def entry_file(i):
    """(module key, {file key: tensor}) of ENTRIES[i]"""
    path, form, kw = ENTRIES[i]
    w = dict(tree().named_parameters())[path + ".weight"]
    KH, KW = (w.shape[2], w.shape[3]) if w.ndim == 4 else (1, 1)
    fields = LY.lattice_fields(form, w.shape[0], w.shape[1], KH, KW, seed=100 + i, **kw)
    key = "lora_unet_" + path.replace(".", "_")
    return key, {f"{key}.{k}": torch.from_numpy(np.asarray(v)) for k, v in fields.items()}


class Handle:
    """What the reference reads a file through (safetensors' safe_open object)."""

    def __init__(self, tensors):
        self.tensors = tensors

    def keys(self):
        return self.tensors.keys()

    def get_tensor(self, key):
        return self.tensors[key]


def main():
    from make_golden import _install
    _install()
    from gyre.pipeline import lycoris as ref
    from gyre.pipeline.model_utils import get_hook
    out, meta = {}, []
    for i, (path, form, kw) in enumerate(ENTRIES):
        net = tree()
        key, tensors = entry_file(i)
        ref.apply_lycoris(Handle(tensors), f"g{i}", unet=net)
        module = net.get_submodule(path)
        hook = get_hook(module, ref.LycorisHook)
        hook.set_scale(f"g{i}", USER_SCALE)
        with torch.no_grad():
            delta = hook._calc_updown(f"g{i}", module.weight)
        assert tuple(delta.shape) == tuple(module.weight.shape)
        out[f"delta_{i}"] = delta.detach().to(torch.float32).numpy()
        meta.append(dict(path=path, form=form, kwargs=kw, seed=100 + i, keys=sorted(tensors), cls=type(hook.lycorii[f"g{i}"]).__name__))
    out["meta"] = np.array(json.dumps(dict(user_scale=USER_SCALE, entries=meta)))
    np.savez_compressed(os.path.join(HERE, "lycoris_vectors.npz"), **out)
    print("wrote", len(meta), "entries:", sorted({m["cls"] for m in meta}))


if __name__ == "__main__":
    main()
