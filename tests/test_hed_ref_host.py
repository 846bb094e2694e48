"""Self-test of the HED references (tests/hed_ref.py), on the host: the test inputs keep every map informative; the restated net and
geometry equal the stored outputs of the reference's own module; the storage-emulation distance of the whole net - the numbers the
GPU model gates are twice of - is measured per (case, flavour, MAP), printed and re-checked; every seeded mistake exceeds the gate of
both flavours on some (case, map); the fp32 emulation of each kernel meets its derived element bound and the kernel-level mistakes
break it.

Distances are per map, never pooled over the six: map 5 has a sixteenth of the others' independent values and its error would vanish
in a pooled norm.  A mistake counts as seen by a flavour when, on one map of one case, the emulation of that flavour WITH the mistake
lies further from the fp64 net than that flavour's gate (twice the emulation's distance) in max-abs OR in rel-L2 - the GPU model test
asserts both.  Which case sees which mistake (max-abs on the worst map against the bf16 gate, measured here): the crop rules differ
from round-half-even at 5x7 and 64x47 (half-up: 4e-2 against 5e-3) and at every odd size (floor: 0.6); floor-mode pooling moves maps
2 - 6 wherever a stage is odd (0.7) and maps 4 - 6 only at 16x16 (0.2).  A pooling window that reads past an odd side is the one the
model gates see least: what it reads there - the next row's first pixel, the next sample's first row - is the quiet zero border,
34 image pixels from the crop, and a maximum with a quiet value seldom moves.  Only an odd stage 4 reaches the crop (through the three
convolutions of stage 5, on maps 5 and 6), and on the five sizes of the issue it reaches it too weakly for the bf16 gate: map 5 moves
by 1.23 x the gate at 33x20 and by less than the gate everywhere else (0.9 x at 1x1; squares of 2 .. 4, 13 .. 18, 29 .. 36, 49 and 65
were tried: at most 1.5 x).  13x4 is the case added for it, the smallest clear one: stage 4 is odd both ways (11 x 9) and the 6 x 5
stage-5 map is cropped next to its last row and column - map 5 moves by 2.4 x the bf16 gate and 15 x the fp16 gate in max-abs, 2.5 x
and 19 x in rel-L2.  The tail kernel's own test holds the window rule bit for bit (tests/test_gpu_hed_kernels.py; below: reading past
changes the pooled bits of every odd TAIL_SIZES entry)."""
import os

import numpy as np
import pytest
import torch

import hed_ref as R

SDTS = [torch.bfloat16, torch.float16]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hed_vectors.npz")
# (max-abs per map, rel-L2 per map) of net(store=dt) against the fp64 net on MODEL_CASES, as printed by test_storage_emulation_distance:
# the table tests/test_gpu_hed_model.py imports.  The assertion keeps it honest (a changed net or recipe must re-measure).  Each entry
# is the WORST of DRAWS input draws of the recipe (hed_ref.model_input(name, seed=0 .. DRAWS - 1)); the GPU tests run draw 0.  One draw
# is too few at the small sizes: a map of 1x1 has two pixels per batch, and whether their output rounding lands near a half step is
# luck - draw 0 alone gave 2.9e-4 for bf16 map 3 at 1x1, a third of the half step 9.8e-4 of a bf16 value in [0.5, 1).
DRAWS = 8
EMULATION = {
    ("1x1", torch.bfloat16): ([8.417e-04, 1.656e-03, 8.745e-04, 1.696e-03, 1.893e-03, 1.925e-03],
                              [1.955e-03, 3.167e-03, 1.437e-03, 2.340e-03, 2.019e-03, 3.097e-03]),
    ("1x1", torch.float16): ([1.660e-04, 2.136e-04, 1.115e-04, 2.697e-04, 2.310e-04, 2.410e-04],
                              [3.211e-04, 3.265e-04, 2.099e-04, 3.635e-04, 2.720e-04, 3.360e-04]),
    ("5x7", torch.bfloat16): ([3.044e-03, 3.594e-03, 2.592e-03, 2.263e-03, 2.510e-03, 2.786e-03],
                              [2.561e-03, 3.106e-03, 2.624e-03, 2.025e-03, 1.567e-03, 2.122e-03]),
    ("5x7", torch.float16): ([3.744e-04, 4.099e-04, 3.701e-04, 2.511e-04, 3.626e-04, 4.025e-04],
                              [2.972e-04, 3.178e-04, 3.194e-04, 2.777e-04, 2.025e-04, 2.762e-04]),
    ("16x16", torch.bfloat16): ([4.079e-03, 4.897e-03, 4.758e-03, 5.011e-03, 2.885e-03, 3.748e-03],
                              [2.407e-03, 2.774e-03, 4.226e-03, 5.007e-03, 1.348e-03, 2.023e-03]),
    ("16x16", torch.float16): ([4.694e-04, 7.058e-04, 6.264e-04, 5.174e-04, 3.556e-04, 5.260e-04],
                              [2.866e-04, 3.235e-04, 4.432e-04, 5.651e-04, 1.740e-04, 3.064e-04]),
    ("33x20", torch.bfloat16): ([4.154e-03, 6.627e-03, 6.079e-03, 5.773e-03, 3.394e-03, 4.544e-03],
                              [2.431e-03, 2.854e-03, 4.202e-03, 6.654e-03, 1.309e-03, 1.917e-03]),
    ("33x20", torch.float16): ([5.245e-04, 7.110e-04, 7.789e-04, 7.759e-04, 4.939e-04, 6.793e-04],
                              [2.875e-04, 3.353e-04, 5.338e-04, 8.445e-04, 1.878e-04, 3.362e-04]),
    ("64x47", torch.bfloat16): ([4.198e-03, 6.368e-03, 7.522e-03, 5.335e-03, 5.422e-03, 4.286e-03],
                              [2.388e-03, 2.865e-03, 4.366e-03, 7.859e-03, 1.247e-03, 1.699e-03]),
    ("64x47", torch.float16): ([5.004e-04, 7.717e-04, 1.108e-03, 7.526e-04, 6.239e-04, 7.635e-04],
                              [2.854e-04, 3.577e-04, 6.363e-04, 9.739e-04, 1.705e-04, 3.033e-04]),
    ("13x4", torch.bfloat16): ([3.353e-03, 4.068e-03, 2.866e-03, 2.230e-03, 2.520e-03, 2.745e-03],
                              [2.438e-03, 3.298e-03, 2.255e-03, 2.162e-03, 1.629e-03, 2.111e-03]),
    ("13x4", torch.float16): ([5.085e-04, 5.302e-04, 3.991e-04, 2.722e-04, 3.372e-04, 4.338e-04],
                              [3.062e-04, 3.664e-04, 2.956e-04, 3.119e-04, 2.022e-04, 3.093e-04]),
}
# the cases a mistake is looked for on, smallest first (the search stops at the first map that shows it)
TOUCHES = {"crop_floor": ("1x1", "5x7"), "crop_half_up": ("5x7", "64x47"), "pool_floor": ("1x1", "16x16"),
           "pool_reads_past": ("13x4",)}
_NET = {}


def _net(name, seed=0):
    """(weights, input, fp64 maps) - computed once per (case, draw) and shared"""
    if (name, seed) not in _NET:
        sd, x = R.model_weights(), R.model_input(name, seed=seed)
        _NET[(name, seed)] = (sd, x, R.net(sd, x, compute=torch.float64))
    return _NET[(name, seed)]


def _distances(got, ref):
    return [R.max_abs(a, b) for a, b in zip(got, ref)], [R.rel_l2(a, b) for a, b in zip(got, ref)]


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_every_map_is_informative(name):
    """the condition of the test inputs: at least half of the pixels of EACH map lie where the sigmoid still tells logits apart"""
    _, x, ref = _net(name)
    frac = R.informative_fraction(ref)
    print(f"[hed] {name}: share of pixels in (0.02, 0.98) per map {[round(f, 3) for f in frac]}")
    assert all(tuple(m.shape) == (R.BATCH, 1) + R.MODEL_CASES[name] for m in ref)
    assert min(frac) >= 0.5
    assert all(float(m.std()) > 1e-3 for m in ref[:3]) and float(x.abs().max()) < 150


def test_geometry_rules():
    assert R.stage_sizes(1) == [69, 35, 18, 9, 5] and R.stage_sizes(512) == [580, 290, 145, 73, 37]
    assert [R.crop_offset(d) for d in (0, 1, 2, 3, 4, 5, 7)] == [0, 0, 1, 2, 2, 2, 4]          # halves to even
    assert R.crop_offsets(5)[0] == 34 and all(R.crop_offsets(n)[0] == 34 for n in range(1, 81))
    differ = [n for n in range(1, 81) if R.crop_offsets(n) != R.crop_offsets(n, "half_up")]
    assert differ == list(range(3, 81, 4))                            # 7 of 5x7 and 47 of 64x47; not 5, 33, 20, 16 or 64
    assert all(R.crop_offsets(n) != R.crop_offsets(n, "floor") for n in range(1, 81, 2))
    for s in (2, 4, 8, 16):
        f = R.bilinear(s, torch.float64)[0, 0]
        assert float(f[s - 1, s - 1]) == (1 - 0.5 / s) ** 2 and torch.equal(f, f.t()) and torch.equal(f, f.flip(0))
        assert torch.equal(f.float().double(), f)                  # exact in fp32


def test_stored_reference_geometry_and_outputs():
    """tests/golden/hed_vectors.npz holds what the reference's own HED computed (make_hed_golden.py): stage sizes and crop offsets for
    H = 1 .. 80, and the six fp32 maps of the 5x7 case on the seeded weights"""
    stored = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    sides = stored["sides"].tolist()
    assert sides == list(range(1, 81))
    assert stored["stage_sizes"].tolist() == [R.stage_sizes(n) for n in sides]
    assert stored["crop_offsets"].tolist() == [R.crop_offsets(n) for n in sides]
    sd, x = R.model_case("5x7")
    got, want = torch.stack(R.net(sd, x)), torch.from_numpy(stored["maps_5x7"])
    assert got.shape == want.shape
    for k in range(6):
        d = R.max_abs(got[k], want[k])
        print(f"[hed] golden 5x7 map {k + 1}: max-abs {d:.3e}")
        assert d < 1e-5


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_storage_emulation_distance(name, sdt):
    ma, rl = [0.0] * 6, [0.0] * 6
    for seed in range(DRAWS):
        sd, x, ref = _net(name, seed)
        a, r = _distances(R.net(sd, x, store=sdt), ref)
        ma, rl = [max(p) for p in zip(ma, a)], [max(p) for p in zip(rl, r)]
    print(f'    ("{name}", {sdt}): ([{", ".join(f"{v:.3e}" for v in ma)}],\n        [{", ".join(f"{v:.3e}" for v in rl)}]),')
    # what is re-checked: the rel-L2 to 5 %, the max-abs - one element's rounding, which the host's summation order can flip - to 30 %,
    # and so the rel-L2 of a map of fewer than 64 values (1x1: two), which is a few elements' roundings as well
    want_ma, want_rl = EMULATION[(name, sdt)]
    tol_rl = 0.05 if R.BATCH * R.MODEL_CASES[name][0] * R.MODEL_CASES[name][1] >= 64 else 0.30
    for k in range(6):
        assert abs(rl[k] - want_rl[k]) <= tol_rl * want_rl[k], (k, rl[k], want_rl[k])
        assert abs(ma[k] - want_ma[k]) <= 0.30 * want_ma[k], (k, ma[k], want_ma[k])
    assert max(ma) <= (1.4e-2 if sdt == torch.bfloat16 else 1.5e-3) * 1.5         # the order of magnitude the issue measured


def test_fp32_net_is_far_inside_every_gate():
    """the reference alone (fp32 against fp64) stays inside every gate by orders of magnitude"""
    for name in R.MODEL_CASES:
        sd, x, ref = _net(name)
        ma, rl = _distances(R.net(sd, x), ref)
        for k in range(6):
            assert ma[k] <= 0.02 * EMULATION[(name, torch.float16)][0][k] and rl[k] <= 0.02 * EMULATION[(name, torch.float16)][1][k]


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_mistake_exceeds_the_gate_of_both_flavours(mistake):
    seen = {}
    for sdt in SDTS:
        for name in TOUCHES.get(mistake, ("5x7",)):
            sd, x, ref = _net(name)
            ma, rl = _distances(R.net(sd, x, store=sdt, mistake=mistake), ref)
            gate_ma, gate_rl = EMULATION[(name, sdt)]                     # what a native build of that flavour with the mistake meets
            hit = [(k + 1, ma[k] / (2 * gate_ma[k]), rl[k] / (2 * gate_rl[k])) for k in range(6)
                   if ma[k] > 2 * gate_ma[k] or rl[k] > 2 * gate_rl[k]]
            if hit:
                seen[sdt] = (name, hit)
                break
    print(f"[hed] {mistake}: (case, [(map, max-abs / gate, rel-L2 / gate)]) {seen}")
    assert set(seen) == set(SDTS)


def test_crop_mistakes_are_invisible_where_the_rules_agree():
    """the cases are there for a reason: 33x20 cannot tell half-up from half-even, 16x16 cannot tell any crop rule apart"""
    for name, mistake in (("33x20", "crop_half_up"), ("16x16", "crop_floor"), ("16x16", "crop_half_up")):
        sd, x, _ = _net(name)
        assert all(torch.equal(a, b) for a, b in zip(R.net(sd, x), R.net(sd, x, mistake=mistake)))
    sd, x, _ = _net("16x16")
    same = [torch.equal(a, b) for a, b in zip(R.net(sd, x), R.net(sd, x, mistake="pool_floor"))]
    assert same == [True, True, True, False, False, False]


# ------------------------------------------------------------------------------------------------------------------------ kernel bounds
@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("C", R.TAIL_WIDTHS)
def test_tail_bound_holds_for_fp32_and_sees_the_mistakes(C, sdt):
    for Hs, Ws in R.TAIL_SIZES[:4]:
        x, w, b = R.tail_case(sdt, 3, Hs, Ws, C)
        pooled, so, bound = R.tail_ref(x, w, b)
        fp32 = (x.float().clamp_min(0) * w).sum(-1) + b
        worst = R.verdict(fp32, so, bound)
        assert worst <= 1.0, (Hs, Ws, worst)
        assert R.verdict(R.tail_ref(x, w, b, before_relu=True)[1].float(), so, bound) > 1.0
        assert float(pooled.float().min()) == 0.0                      # a negative-only window pools to exactly zero
        assert tuple(pooled.shape[1:3]) == (-(-Hs // 2), -(-Ws // 2))
        if (Hs % 2 or Ws % 2) and Hs > 1 and Ws > 1:                   # a window past an odd side: floor mode drops it, reading on changes it
            xc = x.float().permute(0, 3, 1, 2)
            assert tuple(torch.nn.functional.max_pool2d(xc, 2, 2).shape[2:]) != tuple(pooled.shape[1:3])
            wrong = torch.relu(R._pool_reading_past(xc)).permute(0, 2, 3, 1).to(sdt)
            assert not torch.equal(R.bits(wrong), R.bits(pooled))


@pytest.mark.parametrize("name", list(R.MODEL_CASES))
def test_fuse_bound_holds_for_fp32_and_sees_the_mistakes(name):
    H, W = R.MODEL_CASES[name]
    so, wf, bf = R.fuse_case(name)
    ref, t = R.fuse_ref(so, wf, bf, H, W)
    assert tuple(ref.shape) == (6, R.BATCH, 1, H, W)
    # fp32 torch: the transposed convolutions, the 1x1 fuse, the sigmoids
    oy, ox = R.crop_offsets(H), R.crop_offsets(W)
    ls = [so[0][:, None, oy[0]:oy[0] + H, ox[0]:ox[0] + W]]
    for k in range(1, 5):
        up = torch.nn.functional.conv_transpose2d(so[k][:, None], R.bilinear(2 ** k, torch.float32), stride=2 ** k)
        ls.append(up[:, :, oy[k]:oy[k] + H, ox[k]:ox[k] + W])
    fuse = torch.nn.functional.conv2d(torch.cat(ls, 1), wf.reshape(1, 5, 1, 1), bf)
    got = torch.sigmoid(torch.stack(ls + [fuse]))
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert R.verdict(got.to(dt), ref, R.stored_bound(ref, t, dt)) <= 1.0
    bound = R.stored_bound(ref, t, torch.bfloat16)
    assert R.verdict(R.fuse_ref(so, wf, bf, H, W, centre_s=True)[0].float(), ref, bound) > 1.0
    if H % 2 or W % 2:
        assert R.verdict(R.fuse_ref(so, wf, bf, H, W, rule="floor")[0].float(), ref, bound) > 1.0
    if name in ("5x7", "64x47"):
        assert R.verdict(R.fuse_ref(so, wf, bf, H, W, rule="half_up")[0].float(), ref, bound) > 1.0
    assert R.verdict(R.fuse_ref(so, wf[[1, 0, 2, 3, 4]], bf, H, W)[0].float(), ref, bound) > 1.0
