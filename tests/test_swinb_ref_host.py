"""tests/swinb_ref.py held to the reference's own SwinTransformer through vectors recorded from it (tests/golden/make_swinb_golden.py),
and GyreHipSwinB's parameter names and shapes held to SwinB()'s state dict recorded with them.  No GPU."""
import os

import numpy as np
import torch

import swinb_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.hinters import GyreHipSwinB

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swinb_vectors.npz"))


def test_restatement_matches_the_recorded_reference_outputs():
    sd = R.seeded_state_dict(weights.swinb_param_shapes(gcfg.swinb_config(**R.TINY)))
    assert abs(sum(float(v.double().abs().sum()) for v in sd.values()) - float(GOLD["weight_l1"])) <= 1e-9 * float(GOLD["weight_l1"])
    outs = R.net({k: v.double() for k, v in sd.items()}, R.TINY, torch.from_numpy(GOLD["x"]))
    assert len(outs) == 5
    for i, got in enumerate(outs):
        want = torch.from_numpy(GOLD[f"y{i}"])
        d = R.rel_l2(got, want)
        print(f"[swinb] map {i} {tuple(want.shape)}: rel-L2 of the float64 restatement against the reference's fp32 {d:.3e}")
        assert tuple(got.shape) == tuple(want.shape) and d < 1e-5          # fp32 round-off of an 8-block residual stream


def test_module_state_dict_is_the_reference_swinb_state_dict():
    sd = GyreHipSwinB().state_dict()
    assert list(sd) == [str(k) for k in GOLD["keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in GOLD["shapes"]]
    assert sd["layers.0.blocks.0.attn.relative_position_index"].dtype == torch.long
    names = ["gyre_swinb_" + n for n in ("create", "destroy", "num_params", "param_key", "set_weight", "finalize", "workspace_bytes", "forward")]
    assert all(n in _lib.EXPORTED_SYMBOLS for n in names + ["gyre_op_win12_attn", "gyre_op_win12_bias"])
