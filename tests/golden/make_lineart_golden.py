"""Writes tests/golden/lineart_vectors.npz: the outputs of the REFERENCE's own DrawingGenerator (loaded from /root/reference by
tests/golden/ref_lineart_probe.py) on the synthetic weights and images of two lineart_ref.MODEL_CASES entries.  Only the outputs are
stored - weights and images are regenerated from the seed (lineart_ref.model_case).  Build container only:

    python tests/golden/make_lineart_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_lineart_probe as P  # noqa: E402

out = {name: t.numpy() for name, t in P.reference_outputs().items()}
np.savez_compressed(os.path.join(HERE, "lineart_vectors.npz"), **out)
print({k: v.shape for k, v in out.items()})
