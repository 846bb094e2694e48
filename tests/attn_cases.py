"""Case tables of the attention GPU tests (tests/test_gpu_attn_fwd.py, tests/test_gpu_bwd_kernels.py), with the kernel set every row
is meant to reach written down as data.  Nothing here touches a GPU: tests/test_attn_plan_host.py asks the library's planner
(gyre_debug_attn_plan / gyre_debug_attn_bwd_plan) whether each row really gets there, and whether every kernel set has a row.
"""
# kernel families, as gyre_debug_attn_plan reports them (AttnFamily, csrc/kernels.h)
K_ATTN, K_ATTN2_PLAIN, K_ATTN2_FOLD, K_ATTN3 = 0, 1, 2, 3
# values of gyre_debug_force_attn_variant (AttnVariant, csrc/kernels.h)
VAR_AUTO, VAR_V1, VAR_V2_PLAIN, VAR_V2_FOLD, VAR_V2_Q64, VAR_V3, VAR_NO_QLOOP, VAR_ALWAYS_CHECK, VAR_AUTO_ALIAS = range(9)

# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
# (Nq, Nk): Nq in {1, 63, 65, 129, 300} and a multi-block 600; Nk in {1, 7, 8, 63, 64, 65, 77, 129, 257, 1000}; 300 x 300 gives
# family 5 a self-attention (Q and K out of one buffer)
SHAPES = [(1, 1), (129, 1), (63, 7), (65, 8), (129, 63), (300, 64), (65, 65), (129, 77), (300, 129), (63, 257), (300, 300),
          (600, 257), (300, 1000)]
LONG = [(1, 257), (63, 257), (65, 1000), (129, 256), (300, 300), (600, 257), (300, 1000)]       # Nk >= 256: k_attn3 by default
SHORT = [s for s in SHAPES if s[1] < 256] + [(600, 255)]                                          # below that: k_attn3 when forced


def batch_heads(D):
    return (3, 1) if D == 512 else (2, 2)


_D_ALL = [8, 16, 32, 40, 64, 80, 128, 160, 512]
_D_V2 = [16, 32, 40, 64, 80, 128, 160]
_D_V3 = [16, 32, 40, 64, 80]
# branch -> (variant, prescaled, head dims, shapes, V^T pad, {family: the head dims that reach it}, QI of the k_attn2 / k_attn3 rows).
# No shape here has enough query blocks for the several-query-blocks form (QLOOP): that is QLOOP_DIMS / qloop_shapes below.
BRANCHES = {
    "k_attn": (VAR_V1, 0, _D_ALL, SHAPES, "zero", {K_ATTN: _D_ALL}, 2),
    "auto_plain": (VAR_AUTO, 0, _D_ALL, SHAPES, "nan", {K_ATTN2_PLAIN: _D_V2, K_ATTN: [8, 512]}, 2),          # NaN pads
    "attn2_plain": (VAR_V2_PLAIN, 0, _D_V2, SHAPES, "zero", {K_ATTN2_PLAIN: _D_V2}, 2),
    "attn2_plain_q64": (VAR_V2_Q64, 0, [16, 32], SHAPES, "zero", {K_ATTN2_PLAIN: [16, 32]}, 4),
    "attn2_folded": (VAR_V2_FOLD, 1, [16, 32, 40, 64, 160], SHAPES, "zero", {K_ATTN2_FOLD: [16, 32, 40, 64, 160]}, 2),
    # no folded form for these head dims: the plain one, with unit scale
    "prescaled_no_folded_form": (VAR_V2_FOLD, 1, [80, 128], SHAPES, "zero", {K_ATTN2_PLAIN: [80, 128]}, 2),
    "attn3_optimistic": (VAR_AUTO, 1, _D_V3, LONG, "zero", {K_ATTN3: _D_V3}, 2),
    "attn3_checked": (VAR_ALWAYS_CHECK, 1, _D_V3, LONG, "zero", {K_ATTN3: _D_V3}, 2),
    "attn3_short_keys": (VAR_V3, 1, _D_V3, SHORT, "zero", {K_ATTN3: _D_V3}, 2),
}
BRANCH_CASES = [(b, D) for b, spec in BRANCHES.items() for D in spec[2]]


def branch_family(branch, D):
    """(family, QI) the (branch, D) row names; k_attn has one query fragment per wave for D = 512, two otherwise."""
    (fam,) = [f for f, dims in BRANCHES[branch][5].items() if D in dims]
    return fam, ((1 if D == 512 else 2) if fam == K_ATTN else BRANCHES[branch][6])


# moving maximum (family 3): (B, heads, Nq, Nk), the folded k_attn2 under VAR_V2_FOLD, k_attn3 under VAR_AUTO and VAR_ALWAYS_CHECK
MOVING_SHAPE = (2, 2, 300, 1000)
MOVING_FOLDED_DIMS = [16, 32, 40, 64, 160]
MOVING_ATTN3_DIMS = [16, 32, 40, 64, 80]

# several query blocks per workgroup (k_attn2<..., QLOOP>)
QLOOP_DIMS = [40, 64, 80, 160]


def qloop_shapes(D):
    """(B, heads, Nq, Nk, qiter expected; 0: the one-block form).  ring = the largest key count whose tiles each have a ring slot."""
    ring = 192 if D == 160 else 256
    shapes = [(13, 16, 600, 77, 2),          # nblk = 5: qiter 2, the last workgroup walks one block, that block a tail
              (13, 16, 640, 1, 2), (13, 16, 640, 80, 2),
              (13, 16, 640, ring, 2), (13, 16, 640, ring + 1, 0)]     # the last key count inside the branch, the first outside
    if D <= 64:
        shapes.append((32, 32, 200, 77, 2))  # nblk = 2 < nblk B H / 512 = 4: qiter clipped to nblk, a tail block
    if D == 40:
        shapes.append((16, 8, 4096, 77, 8))  # the 64x64 level's cross-attention at batch 16: qiter clipped to 8
    return shapes


def qloop_variants(presc, qiter, Nk):
    """The variants test_qloop_and_its_one_block_form runs a shape under.  The first key count outside the ring, prescaled,
    D <= 80: Nk >= 256 goes to k_attn3 under VAR_AUTO and VAR_NO_QLOOP alike, so VAR_V2_FOLD is what reaches the one-block k_attn2
    there (folded; plain with unit scale for D = 80)."""
    return (VAR_V2_FOLD,) if presc and qiter == 0 and Nk >= 256 else (VAR_AUTO, VAR_NO_QLOOP)


def qloop_reaches(D, presc, Nk, qiter, variant):
    """(family, QLOOP, qiter) of one launch of test_qloop_and_its_one_block_form.  Prescaled K with 256 keys and D <= 80 - the last
    key count inside the ring - belongs to k_attn3 under the automatic variants, so the folded QLOOP form is met at 77 and 80 keys
    (and at its ring edge for D = 160, 192 keys); the plain form is met at every edge."""
    if presc and Nk >= 256 and D <= 80 and variant != VAR_V2_FOLD:
        return K_ATTN3, 0, 1
    on = qiter > 0 and variant == VAR_AUTO
    return (K_ATTN2_FOLD if presc and D != 80 else K_ATTN2_PLAIN), int(on), qiter if on else 1


UNSUPPORTED_DIMS = [48, 24]              # -6, nothing written; (B, heads, Nq, Nk) = (2, 2, 65, 77)

# ---------------------------------------------------------------------------------------------------------------------------
# backward: launch_attention_bwd's kernel sets (gyre_debug_attn_bwd_plan: family, the head-dim bound of the row)
# ---------------------------------------------------------------------------------------------------------------------------
BWD_DMA, BWD_LDS, BWD_REG = 0, 1, 2
BWD_LAST = 1 << 30                       # the bound of the register-staged table's last row
BWD_D_ALL = [8, 32, 40, 48, 64, 80, 96, 128, 160, 192, 512]
# D -> (family, bound): D = 40 the LDS-DMA kernels; D <= 160 the LDS-tile kernels, every row of their table, D = 128 with a partial
# last k-step; above that the register-staged kernels with d-chunks (D = 192: a partial chunk)
BWD_REACHES = {8: (BWD_LDS, 48), 32: (BWD_LDS, 48), 40: (BWD_DMA, 40), 48: (BWD_LDS, 48), 64: (BWD_LDS, 64), 80: (BWD_LDS, 80),
               96: (BWD_LDS, 96), 128: (BWD_LDS, 160), 160: (BWD_LDS, 160), 192: (BWD_REG, BWD_LAST), 512: (BWD_REG, BWD_LAST)}
BWD_SCALING_DIMS = [40, 80, 160]
BWD_SUM_DIMS = [8, 40, 80, 128, 192, 512]
BWD_EQUAL_V_DIMS = [8, 40, 80, 160, 192]


def bwd_heads(D):
    return 2 if D < 512 else 1


def bwd_elementwise_shapes():
    """(B, Nq, Nk, D, presc) of test_attention_bwd_elementwise"""
    out = []
    for D in BWD_D_ALL:
        for (B, Nq, Nk) in ((2, 1, 1), (2, 33, 31), (1, 300, 257)) + (((1, 1030, 1030),) if D <= 160 else ()):
            for presc in (0, 1):
                out.append((B, Nq, Nk, D, presc))
    return out
