"""Writes tests/golden/hed_vectors.npz: what the REFERENCE's own HED (loaded from /root/reference by tests/golden/ref_hed_probe.py)
gives - the stage sizes and crop offsets for sides 1 .. 80, read off its own layers and its crop(), and its six fp32 maps for the 5x7
entry of hed_ref.MODEL_CASES on the seeded weights.  Weights and image are regenerated from the seed (hed_ref.model_case), only
results are stored.  Build container only:

    python tests/golden/make_hed_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_hed_probe as P  # noqa: E402

arch = P.reference_model()
sizes, offsets = P.reference_geometry(arch)
maps = torch.stack(P.reference_maps(arch, "5x7")).numpy()
np.savez_compressed(os.path.join(HERE, "hed_vectors.npz"), sides=np.array(P.SIDES, dtype=np.int32), stage_sizes=np.array(sizes, dtype=np.int32),
                    crop_offsets=np.array(offsets, dtype=np.int32), maps_5x7=maps)
print(maps.shape, sizes[0], offsets[0])
