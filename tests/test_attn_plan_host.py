"""What the attention launchers decide, asked of the library without a device (gyre_debug_attn_plan, gyre_debug_attn_bwd_plan,
gyre_debug_attn_tables; csrc/kernels_attn.hip attn_plan(), csrc/kernels_bwd.hip attn_bwd_plan()).

1. Every case of the GPU tables (tests/attn_cases.py) reaches the kernel set its row names - "every dispatch branch" of
   tests/test_gpu_attn_fwd.py and tests/test_gpu_bwd_kernels.py is a checked statement, not a comment.
2. Every row of the forward launch table and of the two backward tables is reached by a case of those tables.
3. The rule at its edges.
4. Every planned LDS size fits the CU, twice where the kernel is compiled for two workgroups per CU.
5. The shapes the models launch, against the decisions of the code before attn_plan() existed (MODEL_SHAPES: written down from a
   scratch build of that code whose four launchers printed family, grid, LDS size and qiter; the same print agreed with
   gyre_debug_attn_plan on 52,800 (variant, B, H, Nq, Nk, D, prescaled) combinations).
"""
import ctypes as C
import json
import os

import pytest

import attn_cases as T
from attn_fwd_ref import expects_qloop
from gyre_amd import _lib

LDS_CU = 160 * 1024
FAM, D_, QI, PD, SLOTS, LDS, GX, GY, GZ, QITER, ALWAYS, QLOOP = range(12)


@pytest.fixture(params=[_lib.BF16, _lib.F16], ids=["bf16", "f16"])
def L(request):
    return _lib.lib(request.param)


def plan(L, variant, B, H, Nq, Nk, D, presc, ldq=None, ldk=None, ldvt=None, ldo=None):
    """(status, the twelve ints) under gyre_debug_force_attn_variant(variant); strides default to the dense layout"""
    out = (C.c_int32 * 12)()
    dense = lambda ld: H * D if ld is None else ld
    old = L.gyre_debug_force_attn_variant(variant)
    try:
        rc = L.gyre_debug_attn_plan(B, H, Nq, Nk, D, presc, dense(ldq), dense(ldk), (Nk + 7) // 8 * 8 if ldvt is None else ldvt,
                                    dense(ldo), out)
    finally:
        L.gyre_debug_force_attn_variant(old)
    return rc, list(out)


def bwd_plan(L, B, H, Nq, Nk, D, with_dk=1):
    out = (C.c_int32 * 10)()
    return L.gyre_debug_attn_bwd_plan(B, H, Nq, Nk, D, with_dk, out), list(out)


def tables(L, which, width):
    buf = (C.c_int32 * 512)()
    n = L.gyre_debug_attn_tables(which, buf, 512)
    return [tuple(buf[i * width:(i + 1) * width]) for i in range(n)]


def forward_cases():
    """(variant, B, heads, Nq, Nk, D, presc) -> (family, QI, qloop, qiter) for every launch of the forward GPU tables"""
    for branch, D in T.BRANCH_CASES:
        variant, presc, _, shapes = T.BRANCHES[branch][:4]
        fam, qi = T.branch_family(branch, D)
        for Nq, Nk in shapes:
            yield (variant, *T.batch_heads(D), Nq, Nk, D, presc), (fam, qi, 0, 1)
    for D in T.MOVING_FOLDED_DIMS:
        yield (T.VAR_V2_FOLD, *T.MOVING_SHAPE, D, 1), (T.K_ATTN2_FOLD, 2, 0, 1)
    for D in T.MOVING_ATTN3_DIMS:
        for variant in (T.VAR_AUTO, T.VAR_ALWAYS_CHECK):
            yield (variant, *T.MOVING_SHAPE, D, 1), (T.K_ATTN3, 2, 0, 1)
    for D in T.QLOOP_DIMS:
        for presc in (0, 1):
            for B, heads, Nq, Nk, qiter in T.qloop_shapes(D):
                for variant in T.qloop_variants(presc, qiter, Nk):
                    fam, on, qi = T.qloop_reaches(D, presc, Nk, qiter, variant)
                    yield (variant, B, heads, Nq, Nk, D, presc), (fam, 2, on, qi)


def test_every_forward_case_reaches_the_kernel_its_row_names(L):
    n = 0
    for args, (fam, qi, qloop, qiter) in forward_cases():
        rc, p = plan(L, *args)
        assert rc == 0, (args, rc)
        assert (p[FAM], p[D_], p[QI], p[QLOOP], p[QITER]) == (fam, args[5], qi, qloop, qiter), (args, p)
        assert p[ALWAYS] == int(fam == T.K_ATTN3 and args[0] == T.VAR_ALWAYS_CHECK), (args, p)
        n += 1
    assert n > 600
    for D in T.QLOOP_DIMS:           # the GPU test's own mirror of the rule agrees with the library
        for B, heads, Nq, Nk, qiter in T.qloop_shapes(D):
            assert expects_qloop(B, heads, Nq, Nk, D) == qiter
    for D in T.UNSUPPORTED_DIMS:
        for presc in (0, 1):
            assert plan(L, T.VAR_AUTO, 2, 2, 65, 77, D, presc)[0] == -6


def test_every_backward_case_reaches_the_kernel_set_its_row_names(L):
    assert set(T.BWD_REACHES) == set(T.BWD_D_ALL)
    assert set(T.BWD_SCALING_DIMS + T.BWD_SUM_DIMS + T.BWD_EQUAL_V_DIMS) <= set(T.BWD_D_ALL)
    sizes = {(B, Nq, Nk, D) for B, Nq, Nk, D, _ in T.bwd_elementwise_shapes()}
    sizes |= {(b, nq, nk, D) for D in T.BWD_D_ALL for b, nq, nk in ((1, 192, 640), (2, 300, 1), (2, 300, 77), (1, 300, 257),
                                                                  (2, 130, 97), (3, 70, 65), (2, 200, 150))}
    for B, Nq, Nk, D in sorted(sizes):
        H = T.bwd_heads(D)
        rc, p = bwd_plan(L, B, H, Nq, Nk, D)
        assert rc == 0 and (p[0], p[1]) == T.BWD_REACHES[D], (B, Nq, Nk, D, p)
        chunks = 1 if p[0] != T.BWD_REG else -(-((D + 31) // 32) // 4)          # the last register-staged row holds four 32-blocks
        assert p[2] == chunks and p[4:7] == [(Nq + 127) // 128 * chunks, H, B] and p[7:10] == [(Nk + 127) // 128 * chunks, H, B], p
        assert (p[3] == 0) == (p[0] == T.BWD_REG) and p[3] <= LDS_CU, p
        assert bwd_plan(L, B, H, Nq, Nk, D, with_dk=0)[1][7:10] == [0, 0, 0]      # cross-attention: the dQ kernel alone
    assert bwd_plan(L, 1, 2, 64, 64, 36)[0] == -1 and bwd_plan(L, 1, 2, 0, 64, 40)[0] == -1


def test_every_kernel_set_has_a_gpu_case(L):
    reached = set()
    for args, _ in forward_cases():
        p = plan(L, *args)[1]
        reached.add((p[FAM], p[D_], p[QI], p[QLOOP]))
    rows = tables(L, 0, 4)
    assert len(rows) == 35 and len(set(rows)) == 35
    assert set(rows) == reached, sorted(set(rows) ^ reached)

    got = {bwd_plan(L, 1, T.bwd_heads(D), 300, 257, D)[1][1] for D in T.BWD_D_ALL}
    lds_rows, reg_rows = [r[0] for r in tables(L, 1, 1)], [r[0] for r in tables(L, 2, 1)]
    assert lds_rows == [48, 64, 80, 96, 160] and set(lds_rows) <= got
    # launch_attention_bwd sends the register-staged kernels head dims above 160 only (attn_bwd_needs_transposes), so of their
    # table the last row is the one a launch can reach - and the only one that needs, or can have, a GPU case
    assert reg_rows[-1] == T.BWD_LAST and T.BWD_LAST in got
    for D in range(8, 1025, 8):
        fam, bound = bwd_plan(L, 1, 1, 64, 64, D)[1][:2]
        assert (fam == T.BWD_REG) == (D > 160) and (fam != T.BWD_REG or bound == T.BWD_LAST), (D, fam, bound)


def test_the_rule_at_its_edges(L):
    fam = lambda *a, **k: plan(L, *a, **k)[1][FAM]
    # 256 keys: k_attn3 takes over from the folded k_attn2 (prescaled K only)
    assert fam(0, 2, 8, 4096, 255, 40, 1) == T.K_ATTN2_FOLD and fam(0, 2, 8, 4096, 256, 40, 1) == T.K_ATTN3
    assert fam(0, 2, 8, 4096, 256, 40, 0) == T.K_ATTN2_PLAIN
    for v in (T.VAR_NO_QLOOP, T.VAR_ALWAYS_CHECK, T.VAR_AUTO_ALIAS):
        assert fam(v, 2, 8, 4096, 255, 40, 1) == T.K_ATTN2_FOLD and fam(v, 2, 8, 4096, 256, 40, 1) == T.K_ATTN3
    # qiter = min(8, nblk, nblk B H / 512) with nblk = ceil(Nq / 128): 1 (one block per workgroup), 2, 8
    for B, want in ((3, 1), (4, 2), (15, 7), (16, 8), (64, 8)):
        p = plan(L, 0, B, 8, 4096, 77, 40, 1)[1]
        assert (p[QLOOP], p[QITER], p[GX], p[GY]) == (int(want > 1), want, -(-32 // want), B * 8), (B, p)
    p = plan(L, 0, 32, 32, 200, 77, 40, 1)[1]                        # clipped to nblk = 2
    assert (p[QLOOP], p[QITER], p[GX]) == (1, 2, 1)
    # every key tile in its own ring slot: ceil(Nk / 64) = PD + 2 is the last key count inside, PD + 3 the first outside
    for D, slots in ((40, 4), (64, 4), (80, 4), (160, 3)):
        for presc in ((0, 1) if D == 160 else (0,)):          # (prescaled, D <= 80: 256 keys are k_attn3's)
            inside, outside = plan(L, 0, 13, 16, 640, 64 * slots, D, presc)[1], plan(L, 0, 13, 16, 640, 64 * slots + 1, D, presc)[1]
            assert inside[SLOTS] == slots and (inside[QLOOP], outside[QLOOP]) == (1, 0), (D, inside, outside)
            assert inside[FAM] == outside[FAM] == (T.K_ATTN2_FOLD if presc else T.K_ATTN2_PLAIN)
    # the 77-key cross-attention at batch 16: VAR_NO_QLOOP is the automatic choice but for QLOOP
    a, b = plan(L, T.VAR_AUTO, 16, 8, 4096, 77, 40, 1)[1], plan(L, T.VAR_NO_QLOOP, 16, 8, 4096, 77, 40, 1)[1]
    assert a[:LDS + 1] == b[:LDS + 1] and (a[QLOOP], a[QITER], a[GX]) == (1, 8, 4) and (b[QLOOP], b[QITER], b[GX]) == (0, 1, 32)
    # VAR_V3 needs prescaled K; without it the plain k_attn2
    assert fam(T.VAR_V3, 2, 2, 300, 77, 40, 1) == T.K_ATTN3 and fam(T.VAR_V3, 2, 2, 300, 77, 40, 0) == T.K_ATTN2_PLAIN
    assert fam(T.VAR_V3, 2, 2, 300, 77, 160, 1) == T.K_ATTN2_FOLD                 # no k_attn3 for D = 160
    assert fam(T.VAR_V2_FOLD, 2, 2, 300, 77, 80, 1) == T.K_ATTN2_PLAIN            # no folded k_attn2 for D = 80
    assert plan(L, T.VAR_V2_Q64, 2, 2, 300, 77, 32, 0)[1][QI] == 4 and plan(L, T.VAR_V2_Q64, 2, 2, 300, 77, 40, 0)[1][QI] == 2
    assert plan(L, T.VAR_ALWAYS_CHECK, 2, 2, 300, 300, 40, 1)[1][ALWAYS] == 1 and plan(L, 0, 2, 2, 300, 300, 40, 1)[1][ALWAYS] == 0
    # k_attn3: 1-D grid of ceil(Nq / 128) B H workgroups; ring slots PD + 3 where two workgroups still fit
    p = plan(L, 0, 2, 8, 4000, 4000, 40, 1)[1]
    assert p[GX:GZ + 1] == [32 * 16, 1, 1] and (p[PD], p[SLOTS]) == (2, 5)
    assert plan(L, 0, 2, 8, 1024, 1024, 80, 1)[1][PD:SLOTS + 1] == [1, 4]
    # rejections
    assert plan(L, 0, 2, 2, 65, 77, 24, 0)[0] == -6 and plan(L, 0, 2, 2, 65, 77, 24, 1)[0] == -6
    assert plan(L, 0, 2, 2, 65, 77, 36, 0)[0] == -1 and b"head dim must be a multiple of 8" in L.gyre_last_error()
    for kw in ({"ldq": 84}, {"ldk": 84}, {"ldvt": 84}, {"ldo": 82}):
        assert plan(L, 0, 2, 2, 65, 77, 40, 0, **kw)[0] == -1, kw
    assert plan(L, 0, 2, 2, 65, 77, 40, 0, ldo=84)[0] == 0                        # the output stride: a multiple of 4
    assert plan(L, 0, 2, 2, 65, 77, 40, 0, ldvt=72)[0] == -1                      # ldvt < ceil8(Nk)
    assert plan(L, 0, 2, 2, 0, 77, 40, 0)[0] == -1 and plan(L, 0, 2, 2, 65, 0, 40, 0, ldvt=8)[0] == -1


def _kernel_symbol(p):
    if p[FAM] == T.K_ATTN:
        return f"_Z6k_attnILi{p[D_]}ELi{p[QI]}EEv10AttnParams"
    if p[FAM] == T.K_ATTN3:
        return f"_Z7k_attn3ILi{p[D_]}ELi{p[PD]}ELi{p[QI]}ELi0EEv10AttnParamsPKt"
    return f"_Z7k_attn2ILi{p[D_]}ELi{p[QI]}ELi{p[PD]}ELb{int(p[FAM] == T.K_ATTN2_FOLD)}ELb{p[QLOOP]}EEv10AttnParamsPKti"


def test_planned_lds_fits_the_cu(L):
    """k_attn2 up to D = 80 and k_attn3 are compiled for two workgroups per CU (__launch_bounds__(256, 2)): their ring must fit twice,
    and the registers the build recorded must allow the second workgroup too."""
    path = os.path.join(os.path.dirname(_lib.__file__), "build", "kernel_resources.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res = res.get("kernels_attn.hip" if L.gyre_storage_dtype() == _lib.BF16 else "f16/kernels_attn.hip", {})
    seen = {}
    for args, _ in forward_cases():
        p = plan(L, *args)[1]
        seen[(p[FAM], p[D_], p[QI], p[QLOOP])] = p
    assert len(seen) == 35
    for p in seen.values():
        two = p[FAM] == T.K_ATTN3 or (p[FAM] in (T.K_ATTN2_PLAIN, T.K_ATTN2_FOLD) and p[D_] <= 80)
        assert 0 < p[LDS] <= LDS_CU and (not two or 2 * p[LDS] <= LDS_CU), p
        if p[FAM] != T.K_ATTN:
            stage = (64 * p[D_] * 2 + (p[D_] + 15) // 16 * 16 * 128 + 4095) // 4096 * 4096
            assert p[LDS] == p[SLOTS] * stage, p
        rec = res.get(_kernel_symbol(p))
        if rec is not None:
            assert rec["occupancy_waves_per_simd"] >= (2 if two else 1), (p, rec)
    for D in T.BWD_D_ALL:
        assert bwd_plan(L, 1, 1, 300, 257, D)[1][3] <= LDS_CU


# (B, heads, Nq, Nk, D, prescaled) -> (family, grid x, grid y, LDS bytes, qiter); automatic dispatch
MODEL_SHAPES = {
    # SD1.5, 8 heads, batch 2 (one image with guidance): 64^2 .. 8^2 self-attention, then the 77- and 154-key text context
    (2, 8, 4096, 4096, 40, 1): (T.K_ATTN3, 512, 1, 61440, 1),
    (2, 8, 4096, 77, 40, 1): (T.K_ATTN2_FOLD, 32, 16, 49152, 1),
    (2, 8, 4096, 154, 40, 1): (T.K_ATTN2_FOLD, 32, 16, 49152, 1),
    (2, 8, 1024, 1024, 80, 1): (T.K_ATTN3, 128, 1, 81920, 1),
    (2, 8, 1024, 77, 80, 1): (T.K_ATTN2_PLAIN, 8, 16, 81920, 1),
    (2, 8, 1024, 154, 80, 1): (T.K_ATTN2_PLAIN, 8, 16, 81920, 1),
    (2, 8, 256, 256, 160, 1): (T.K_ATTN2_FOLD, 2, 16, 122880, 1),
    (2, 8, 256, 77, 160, 1): (T.K_ATTN2_FOLD, 2, 16, 122880, 1),
    (2, 8, 256, 154, 160, 1): (T.K_ATTN2_FOLD, 2, 16, 122880, 1),
    (2, 8, 64, 64, 160, 1): (T.K_ATTN2_FOLD, 1, 16, 122880, 1),
    (2, 8, 64, 77, 160, 1): (T.K_ATTN2_FOLD, 1, 16, 122880, 1),
    (2, 8, 64, 154, 160, 1): (T.K_ATTN2_FOLD, 1, 16, 122880, 1),
    # batch 16: the cross-attention of the two large levels walks several query blocks per workgroup
    (16, 8, 4096, 4096, 40, 1): (T.K_ATTN3, 4096, 1, 61440, 1),
    (16, 8, 4096, 77, 40, 1): (T.K_ATTN2_FOLD, 4, 128, 49152, 8),
    (16, 8, 4096, 154, 40, 1): (T.K_ATTN2_FOLD, 4, 128, 49152, 8),
    (16, 8, 1024, 1024, 80, 1): (T.K_ATTN3, 1024, 1, 81920, 1),
    (16, 8, 1024, 77, 80, 1): (T.K_ATTN2_PLAIN, 4, 128, 81920, 2),
    (16, 8, 1024, 154, 80, 1): (T.K_ATTN2_PLAIN, 4, 128, 81920, 2),
    (16, 8, 256, 256, 160, 1): (T.K_ATTN2_FOLD, 2, 128, 122880, 1),
    (16, 8, 256, 77, 160, 1): (T.K_ATTN2_FOLD, 2, 128, 122880, 1),
    (16, 8, 256, 154, 160, 1): (T.K_ATTN2_FOLD, 2, 128, 122880, 1),
    (16, 8, 64, 64, 160, 1): (T.K_ATTN2_FOLD, 1, 128, 122880, 1),
    (16, 8, 64, 77, 160, 1): (T.K_ATTN2_FOLD, 1, 128, 122880, 1),
    (16, 8, 64, 154, 160, 1): (T.K_ATTN2_FOLD, 1, 128, 122880, 1),
    # SDXL's D = 64 levels (10 and 20 heads) at batch 2
    (2, 10, 4096, 4096, 64, 1): (T.K_ATTN3, 640, 1, 81920, 1),
    (2, 10, 4096, 77, 64, 1): (T.K_ATTN2_FOLD, 32, 20, 65536, 1),
    (2, 20, 1024, 1024, 64, 1): (T.K_ATTN3, 320, 1, 81920, 1),
    (2, 20, 1024, 77, 64, 1): (T.K_ATTN2_FOLD, 8, 40, 65536, 1),
    # the VAE's mid block: one head of 512 channels, K not prescaled
    (1, 1, 4096, 4096, 512, 0): (T.K_ATTN, 64, 1, 140288, 1),
}


def test_model_shapes_launch_what_they_always_did(L):
    for args, want in MODEL_SHAPES.items():
        rc, p = plan(L, T.VAR_AUTO, *args)
        assert rc == 0 and (p[FAM], p[GX], p[GY], p[LDS], p[QITER]) == want and p[GZ] == 1 and p[QLOOP] == int(want[4] > 1), (args, p)
