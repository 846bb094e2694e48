"""The yardsticks of tests/lyco_ref.py checked on the CPU: the emulation of the kernels' stated order equals the float64 reference
bit for bit on the lattice family and stays inside the bound on gaussian data (both storage types), the bound is not vacuous,
and each seeded mistake is caught by the smallest case that can show it."""
import numpy as np
import pytest
import torch

import lyco_ref as LY

STORAGES = [torch.bfloat16, torch.float16]
IDS = [c[0] for c in LY.CASES]


@pytest.mark.parametrize("case", LY.CASES, ids=IDS)
def test_lattice_emulation_is_bit_exact(case):
    name, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    base, terms = LY.case_terms(case)
    ref = LY.ref64(base, terms, I_pad, geglu, scale_p)
    assert LY.on_lattice(ref) and np.abs(ref).max() > 1
    emu = LY.emulate(base, terms, I_pad, geglu, scale_p)
    assert np.array_equal(emu.astype(np.float64), ref)
    for storage in STORAGES:                                          # representable: the storage rounding changes nothing
        assert np.array_equal(LY.to_storage(emu, storage).double().numpy(), ref)
    assert not emu[..., I:].any()


@pytest.mark.parametrize("storage", STORAGES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", LY.CASES, ids=IDS)
def test_gaussian_emulation_within_the_bound(case, storage):
    name, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    sp = scale_p if scale_p == 1.0 else 0.1803
    base, terms = LY.case_terms(case, "gaussian")
    ref, tol = LY.ref64(base, terms, I_pad, geglu, sp), LY.bound(base, terms, I_pad, geglu, sp, storage)
    got = LY.to_storage(LY.emulate(base, terms, I_pad, geglu, sp), storage)
    assert LY.worst_ratio(name, got, ref, tol) <= 1.0
    delta = np.abs(ref - LY.ref64(base, [], I_pad, geglu, sp))
    assert delta.max() > 0.05 * np.abs(ref).max()                     # the terms matter next to the base
    # not vacuous: three storage ulps off fails it
    off = got.double().numpy() + 3 * 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1e-30))) + 1) * LY.unit_roundoff(storage)
    assert LY.worst_ratio(name + " +3ulp", off, ref, tol) > 1.0


def test_core_emulation():
    g = np.random.default_rng(5)
    core, right = g.standard_normal((5, 7, 3, 3)).astype(np.float32), g.standard_normal((7, 9)).astype(np.float32)
    want = LY.core64(core, right)
    tol = 7 * LY.U32 * LY.core64(np.abs(core), np.abs(right)) * (1 + 2.0 ** -10)
    assert np.all(np.abs(LY.core_emulate(core, right) - want) <= tol)
    assert not np.all(np.abs(LY.core_emulate(core, right).astype(np.float64) * (1 + 2.0 ** -18) - want) <= tol)


def _case(name, O, I, KH, KW, I_pad, geglu, forms, scale_p=1.0):
    return (name, O, I, KH, KW, I_pad, geglu, scale_p, forms)


# the smallest case that can show each seeded mistake
SMALL = {
    "hadamard_as_sum": _case("s_hada", 4, 4, 1, 1, 4, False, [("loha", dict(rank=1))]),
    "drop_last_partial_rank_second": _case("s_drop", 4, 4, 1, 1, 4, False, [("loha", dict(rank=1))]),
    "wa_not_transposed": _case("s_wa", 4, 4, 3, 3, 4, False, [("loha_t", dict(rank=3))]),
    "core_ab_swapped": _case("s_core", 4, 4, 3, 3, 4, False, [("locon_mid", dict(rank=3))]),
    "kron_div_mod_swapped": _case("s_divmod", 6, 4, 1, 1, 4, False, [("lokr_dense", dict(kron=(2, 2)))]),
    "kron_col_per_lane": _case("s_lane", 4, 12, 1, 1, 12, False, [("lokr_dense", dict(kron=(2, 2)))]),
    "geglu_row_by_dest": _case("s_geglu", 64, 4, 1, 1, 4, True, [("full", {})]),
    "scale_key_ignored": _case("s_scale", 4, 4, 1, 1, 4, False, [("lora", dict(rank=1, scale_rule="scale"))]),
    "lokr_alpha_without_decomposition": _case("s_alpha", 4, 4, 1, 1, 4, False, [("lokr_dense", dict(kron=(2, 2), scale_rule="none"))]),
    "nonzero_pad": _case("s_pad", 4, 4, 1, 1, 8, False, [("full", {})]),
}


@pytest.mark.parametrize("mistake", LY.MISTAKES)
def test_seeded_mistakes_are_caught(mistake):
    case = SMALL[mistake]
    name, O, I, KH, KW, I_pad, geglu, scale_p, _ = case
    base, terms = LY.case_terms(case)
    ref = LY.ref64(base, terms, I_pad, geglu, scale_p)
    assert LY.on_lattice(ref)
    assert np.array_equal(LY.emulate(base, terms, I_pad, geglu, scale_p).astype(np.float64), ref)
    bad = LY.emulate(base, terms, I_pad, geglu, scale_p, mistake=mistake)
    assert not np.array_equal(bad.astype(np.float64), ref), f"{mistake} does not show on {name}"


def test_every_mistake_has_a_case():
    assert set(SMALL) == set(LY.MISTAKES)


def test_file_scale_rules():
    f = LY.lattice_fields("lora", 4, 4, rank=2, scale_rule="alpha")
    assert LY.file_scale(f) == 0.25
    assert LY.file_scale(LY.lattice_fields("lora", 4, 4, rank=2, scale_rule="scale")) == 0.25          # alpha / dim would be 2
    assert LY.file_scale(LY.lattice_fields("lora", 4, 4, rank=2, scale_rule="scale0")) == 0.25         # scale 0 -> alpha / dim
    assert LY.file_scale(LY.lattice_fields("lora", 4, 4, rank=2, scale_rule="none")) == 1.0
    assert LY.file_scale(LY.lattice_fields("full", 4, 4)) == 1.0                                        # alpha 0.5 ignored
    assert LY.file_scale(LY.lattice_fields("lokr_dense", 4, 4, kron=(2, 2), scale_rule="none")) == 1.0  # alpha 0.5 ignored
    assert LY.file_scale(LY.lattice_fields("lokr_w1_lowrank", 4, 4, rank=2, kron=(2, 2))) == 0.125
