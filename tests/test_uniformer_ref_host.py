"""tests/uniformer_ref.py held to the reference's own UniFormer through vectors recorded from it (tests/golden/
make_uniformer_golden.py), GyreHipUniFormer's parameter names and shapes held to the uniformer_small state dict recorded with them, and
the seeded "bias in the halo" mistake shown to leave the element-wise bound of tests/test_gpu_uniformer.py.  No GPU."""
import os

import numpy as np
import torch

import uniformer_ref as R
from gyre_amd import config as gcfg, weights
from gyre_amd.hinters import GyreHipUniFormer

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uniformer_vectors.npz"))


def test_restatement_matches_the_recorded_reference_outputs():
    sd = R.seeded_state_dict(weights.uniformer_param_shapes(gcfg.uniformer_config(**R.TINY)))
    assert abs(sum(float(v.double().abs().sum()) for v in sd.values()) - float(GOLD["weight_l1"])) <= 1e-9 * float(GOLD["weight_l1"])
    outs = R.net({k: v.double() for k, v in sd.items()}, R.TINY, torch.from_numpy(GOLD["x"]))
    assert len(outs) == 4
    for i, got in enumerate(outs):
        want = torch.from_numpy(GOLD[f"y{i}"])
        d = R.rel_l2(got, want)
        print(f"[uniformer] map {i} {tuple(want.shape)}: rel-L2 of the float64 restatement against the reference's fp32 {d:.3e}")
        assert tuple(got.shape) == tuple(want.shape) and d < 1e-5          # fp32 round-off of the residual stream (Swin-B's gate)


def test_module_state_dict_is_the_reference_uniformer_state_dict():
    sd = GyreHipUniFormer().state_dict()
    assert list(sd) == [str(k) for k in GOLD["keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in GOLD["shapes"]]
    assert sd["blocks1.0.norm1.num_batches_tracked"].dtype == torch.long


def test_bias_in_the_halo_leaves_the_bound():
    ops = R.local_case(64, 9, 17, torch.bfloat16)
    val, bound = R.local_bound(*ops, 2.0 ** -8, 2.0 ** -134)
    wrong = R.local(*ops, halo_bias=True)
    ratio = (wrong - val).abs() / bound
    assert float(ratio[:, 2:-2, 2:-2].max()) == 0.0 and float(ratio[:, 0].median()) > 1.0, "the border, and only the border, sees the mistake"
