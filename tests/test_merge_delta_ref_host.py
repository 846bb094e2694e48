"""The yardsticks of tests/test_gpu_merge_delta.py, checked on the CPU (tests/merge_delta_ref.py): the fp32 emulation of
k_merge_delta's stated operation order stays inside the derived bound for every output type, equals the float64 reference bit for
bit on the lattice family, and each seeded mistake is caught by the comparison that is meant to catch it.  Also: the build's
resource record shows the new kernel (and the one it shares its tile with) free of scratch."""
import numpy as np
import pytest
import torch

import lora_ref as LRF
import merge_delta_ref as MD

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("out", list(DT))
@pytest.mark.parametrize("case", MD.CASES, ids=MD.IDS)
def test_emulation_meets_the_bound(case, out):
    base, terms = MD.case_terms(case, "gaussian")
    got = MD.emulate(base, terms, DT[out])
    assert got.dtype == DT[out]
    assert MD.worst_ratio(f"{case[0]} {out}", got, MD.ref64(base, terms), MD.bound(base, terms, DT[out])) <= 1.0


@pytest.mark.parametrize("case", MD.CASES, ids=MD.IDS)
def test_lattice_emulation_is_the_float64_reference(case):
    base, terms = MD.case_terms(case)
    ref = MD.ref64(base, terms)
    assert MD.on_lattice(ref), "the case left the lattice: its values are no longer exact in every type"
    for dt in MD.OUT_DTYPES:
        assert np.array_equal(MD.emulate(base, terms, dt).double().numpy(), ref)


def test_zero_terms_reproduce_base_in_its_own_type():
    base = MD.LY.gaussian_base(130, 68, seed=5)
    for dt in MD.OUT_DTYPES:
        b = MD.quantize(base, dt)
        assert torch.equal(MD.emulate(b, [], dt), torch.from_numpy(b).to(dt))


def test_bound_is_lyco_refs_with_the_output_roundoff():
    """scale_p = 1 and a 16-bit output: the very numbers of lyco_ref.bound; fp32: smaller by exactly the storage term."""
    import lyco_ref as LY
    base, terms = MD.case_terms(MD.CASES[MD.IDS.index("four_terms")], "gaussian")
    for dt in (torch.bfloat16, torch.float16):
        assert np.array_equal(MD.bound(base, terms, dt), LY.bound(base, terms, storage=dt).reshape(base.shape))
    ref = np.abs(MD.ref64(base, terms))
    d = LY.bound(base, terms, storage=torch.bfloat16).reshape(base.shape) - MD.bound(base, terms, torch.float32)
    assert np.allclose(d, 2.0 ** -8 * ref * (1 + 2.0 ** -10), rtol=1e-9, atol=0)


def _cancel_terms(O, I, r):
    """lora_ref's cancel family as LORA terms: +512 d, + d'/4, -512 d - unchanged merged values, but a delta summed in 16 bits
    loses the quarter steps next to 512."""
    base, pairs, _ = LRF.lattice(O, I, (r,), cancel=True, seed=9)
    return base, [({"lora_up.weight": up, "lora_down.weight": down, "scale": np.float32(s)}, 1.0) for up, down, s in pairs]


@pytest.mark.parametrize("out", list(DT))
def test_seeded_mistakes_fail(out):
    dt = DT[out]
    # on the lattice (exact arithmetic): any indexing or accumulation mistake changes bits
    for mistake, name in (("drop_last_partial_rank", "lora_r33"), ("drop_last_partial_rank", "loha_r33_r4"),
                          ("drop_last_partial_rank", "lokr_lowrank_r33"), ("kron_div_mod_swapped", "lokr_dense"),
                          ("kron_div_mod_swapped", "lokr_lowrank_tiles")):
        base, terms = MD.case_terms(MD.CASES[MD.IDS.index(name)])
        ref = MD.ref64(base, terms)
        assert np.array_equal(MD.emulate(base, terms, dt).double().numpy(), ref)
        assert not np.array_equal(MD.emulate(base, terms, dt, mistake).double().numpy(), ref), (mistake, name)
    base, terms = _cancel_terms(72, 12, 4)
    ref = MD.ref64(base, terms)
    assert MD.on_lattice(ref) and np.array_equal(MD.emulate(base, terms, dt).double().numpy(), ref)
    assert not np.array_equal(MD.emulate(base, terms, dt, "delta_in_16_bits").double().numpy(), ref)
    # on gaussian data: outside the bound
    base, terms = MD.case_terms(MD.CASES[MD.IDS.index("four_terms")], "gaussian")
    ref, tol = MD.ref64(base, terms), MD.bound(base, terms, dt)
    assert MD.worst_ratio("correct", MD.emulate(base, terms, dt), ref, tol) <= 1.0
    for mistake in ("wrong_out_rounding", "delta_in_16_bits", "drop_last_partial_rank", "kron_div_mod_swapped"):
        assert MD.worst_ratio(f"{mistake} {out}", MD.emulate(base, terms, dt, mistake), ref, tol) > 1.0, mistake


def test_merge_kernels_have_no_scratch():
    """gyre_amd/build.py records clang's per-kernel resource remarks of kernels_lyco.hip: every instantiation of k_merge_delta
    (fp32, bf16, fp16 output) exists in both storage builds and neither it nor k_repack_delta spills."""
    import json
    from gyre_amd import build as B
    B.build()
    data = json.load(open(B.RESOURCES_JSON))
    for src in ("kernels_lyco.hip", "f16/kernels_lyco.hip"):
        kernels = data[src]
        merge = [k for k in kernels if "k_merge_delta" in k]
        assert len(merge) == 3, sorted(kernels)
        for name in merge + [k for k in kernels if "k_repack_delta" in k]:
            assert kernels[name]["scratch_bytes_per_lane"] == 0, f"{name} in {src} spills"
            assert kernels[name]["lds_bytes"] == 2 * 32 * 68 * 4


def test_lora_only_repack_keeps_the_occupancy_of_the_lora_kernel():
    """k_repack_delta<true>, the instantiation a LoRA-only repack runs, in both storage builds: no scratch, 17408 bytes of LDS, and
    an occupancy not below that of k_repack_lora, the separate LoRA kernel this instantiation replaced.  That kernel, compiled from
    its last revision with the flags of gyre_amd/build.py and -Rpass-analysis=kernel-resource-usage, reported 68 VGPRs, no scratch
    and 7 waves per SIMD in the bf16 build and the same three figures with -DGYRE_STORE_F16."""
    import json
    from gyre_amd import build as B
    B.build()
    data = json.load(open(B.RESOURCES_JSON))
    lora_kernel_waves = {"kernels_lyco.hip": 7, "f16/kernels_lyco.hip": 7}
    for src, waves in lora_kernel_waves.items():
        both = {k: v for k, v in data[src].items() if "k_repack_delta" in k}
        lora_only = [v for k, v in both.items() if "ILb1E" in k]                      # template <bool LORA_ONLY = true>
        assert len(both) == 2 and len(lora_only) == 1, sorted(both)
        r = lora_only[0]
        assert r["scratch_bytes_per_lane"] == 0 and r["lds_bytes"] == 2 * 32 * 68 * 4, (src, r)
        assert r["occupancy_waves_per_simd"] >= waves, (src, r)
