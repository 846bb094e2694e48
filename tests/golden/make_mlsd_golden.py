"""Writes tests/golden/mlsd_vectors.npz: what the REFERENCE's own MobileV2_MLSD_Large (gyre/pipeline/hinters/models/mbv2_mlsd_large.py,
loaded from /root/reference) gives on the CPU in fp32 for the two smallest entries of mlsd_ref.MODEL_CASES on the seeded weights - the
inputs, the outputs, and the 362 key names of its state dict in order.  The weights are regenerated from the seed
(mlsd_ref.model_weights), only inputs, names and results are stored.  Build container only:

    python tests/golden/make_mlsd_golden.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mlsd_ref as R  # noqa: E402

CASES = ("16x16", "17x49")


def reference_model(root="/root/reference"):
    spec = importlib.util.spec_from_file_location("ref_mbv2_mlsd_large", os.path.join(root, "gyre/pipeline/hinters/models/mbv2_mlsd_large.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MobileV2_MLSD_Large().eval()


if __name__ == "__main__":
    model = reference_model()
    keys = list(model.state_dict())
    model.load_state_dict(R.model_weights(), strict=True)
    data = {"keys": np.array(keys)}
    with torch.no_grad():
        for name in CASES:
            x = R.model_input(name)
            data["x_" + name], data["y_" + name] = x.numpy(), model(x).numpy()
    np.savez_compressed(os.path.join(HERE, "mlsd_vectors.npz"), **data)
    print(len(keys), {k: v.shape for k, v in data.items()})
