"""The yardstick of the fused LoRA repack tests, checked on the CPU (tests/lora_ref.py): the numpy fp32 emulation in the kernel's
stated order meets the derived bound on Gaussian data and is bit-exact on the lattice, each seeded mistake is caught by the
lattice comparison, and the lattice is exact under the existing host merge too (lora_delta + ``w + d * scale``) - which is what
lets the GPU tests demand bit equality between the host path and the device path."""
import numpy as np
import pytest
import torch

import lora_ref as LRF
from gyre_amd import lora as LR

# (name, O, I, KH, KW, I_pad, geglu, scale_p, ranks): the operator cases of tests/test_gpu_lora_native.py
CASES = [("linear", 40, 24, 1, 1, 24, False, 1.0, (4,)),
         ("linear_padded_k", 40, 20, 1, 1, 24, False, 1.0, (4,)),
         ("conv3x3", 72, 12, 3, 3, 16, False, 1.0, (4,)),
         ("conv1x1", 40, 24, 1, 1, 24, False, 1.0, (4,)),
         ("geglu", 64, 24, 1, 1, 24, True, 1.0, (4,)),
         ("scale_p", 40, 24, 1, 1, 24, False, 0.5, (4,)),
         ("rank1", 72, 12, 3, 3, 16, False, 1.0, (1,)),
         ("rank33", 72, 12, 3, 3, 16, False, 1.0, (33,)),
         ("rank130", 40, 20, 1, 1, 24, False, 1.0, (130,)),
         ("two_pairs", 72, 12, 3, 3, 16, False, 0.5, (33, 4))]
STORAGES = (torch.bfloat16, torch.float16)


def _lattice(case, **kw):
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    conv = name.startswith("conv") or KH * KW > 1
    return LRF.lattice(O, I, ranks, KH, KW, conv=conv, seed=len(name), **kw)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_emulation_is_bit_exact_on_the_lattice(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    base, pairs, _ = _lattice(case)
    ref = LRF.ref64(base, pairs, I_pad, geglu, scale_p)
    assert LRF.on_lattice(ref)                                                         # the lattice's own promise
    emu = LRF.emulate(base, pairs, I_pad, geglu, scale_p)
    assert emu.shape == (O, KH, KW, I_pad) and np.array_equal(emu.astype(np.float64), ref)
    assert not emu[..., I:].any()
    for st in STORAGES:                                                                # representable: the rounding changes nothing
        assert np.array_equal(LRF.to_storage(emu, st).double().numpy(), ref)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_emulation_meets_the_bound_on_gaussian_data(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    sp = scale_p if scale_p == 1.0 else 0.1803                                         # (an attention scale: no power of two)
    base, pairs = LRF.gaussian(O, I, ranks, KH, KW, conv=name.startswith("conv") or KH * KW > 1, seed=len(name))
    ref = LRF.ref64(base, pairs, I_pad, geglu, sp)
    emu = LRF.emulate(base, pairs, I_pad, geglu, sp)
    for st in STORAGES:
        tol = LRF.bound(base, pairs, I_pad, geglu, sp, st)
        assert LRF.worst_ratio(f"{name} {st}", LRF.to_storage(emu, st), ref, tol) <= 1.0
        # the bound is not vacuous: it is the storage rounding plus a sliver - a result one storage ulp off is outside it
        off = LRF.to_storage(emu, st).double().numpy() * (1 + 4 * LRF.unit_roundoff(st))
        assert LRF.worst_ratio(f"{name} {st} +2ulp", off, ref, tol) > 1.0


# which case shows which seeded mistake (the smallest one that can)
SEEDED = [("drop_last_partial_rank", "rank33"), ("drop_last_partial_rank", "rank130"), ("drop_last_partial_rank", "rank1"),
          ("geglu_up_by_dest_row", "geglu"), ("no_alpha_over_r", "linear"), ("no_scale_p", "scale_p"),
          ("scale_p_on_base_only", "scale_p"), ("nonzero_pad", "linear_padded_k"), ("nonzero_pad", "conv3x3")]


@pytest.mark.parametrize("mistake,case_name", SEEDED)
def test_seeded_mistakes_fail_the_lattice_comparison(mistake, case_name):
    case = next(c for c in CASES if c[0] == case_name)
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    base, pairs, aor = _lattice(case)
    ref = LRF.ref64(base, pairs, I_pad, geglu, scale_p)
    for st in STORAGES:
        good = LRF.to_storage(LRF.emulate(base, pairs, I_pad, geglu, scale_p), st).double().numpy()
        bad = LRF.to_storage(LRF.emulate(base, pairs, I_pad, geglu, scale_p, mistake=mistake, alpha_over_r=aor, storage=st), st)
        assert np.array_equal(good, ref) and not np.array_equal(bad.double().numpy(), ref), (mistake, st)


@pytest.mark.parametrize("shape", [(40, 24, 1, 1, 24), (72, 12, 3, 3, 16)])
def test_a_delta_held_in_16_bits_fails_the_cancelling_lattice(shape):
    """On values as short as the lattice's a 16-bit delta is exact; the cancelling form (three pairs, +512 d, d'/4, -512 d) has the
    same merged values but partial sums that only fp32 holds."""
    O, I, KH, KW, I_pad = shape
    base, pairs, aor = LRF.lattice(O, I, (4,), KH, KW, cancel=True, seed=5)
    ref = LRF.ref64(base, pairs, I_pad)
    assert LRF.on_lattice(ref)
    for st in STORAGES:
        assert np.array_equal(LRF.to_storage(LRF.emulate(base, pairs, I_pad), st).double().numpy(), ref)
        bad = LRF.emulate(base, pairs, I_pad, mistake="delta_in_16_bits", storage=st)
        assert not np.array_equal(LRF.to_storage(bad, st).double().numpy(), ref), st


@pytest.mark.parametrize("case", CASES + [("cancel", 72, 12, 3, 3, 16, False, 1.0, (4,))], ids=[c[0] for c in CASES] + ["cancel"])
def test_lattice_is_exact_under_the_host_merge(case):
    """gyre_amd.lora.lora_delta + ``w + d * scale`` (what apply_lora uploads) gives the float64 reference's values exactly, for
    factors kept in fp32, bf16 or fp16."""
    name, O, I, KH, KW, I_pad, geglu, scale_p, ranks = case
    base, pairs, aor = _lattice(case, cancel=True) if name == "cancel" else _lattice(case)
    ref = LRF.ref64(base, pairs, None, False, 1.0)                                     # OIHW order, no repack
    for fdt in (torch.float32, torch.bfloat16, torch.float16):
        w = torch.from_numpy(base).clone()
        for (up, down, s), a in zip(pairs, aor):
            r = down.shape[0]
            d = LR.lora_delta(torch.from_numpy(up).to(fdt), torch.from_numpy(down).to(fdt), torch.tensor(a * r))
            w = w + d * (s / a)
        got = w.double().numpy().reshape(O, I, KH * KW).transpose(0, 2, 1).reshape(ref.shape)
        assert w.dtype == torch.float32 and np.array_equal(got, ref), fdt
