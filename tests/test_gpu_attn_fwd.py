"""Element-wise parity of the forward attention kernels (csrc/kernels_attn.hip, csrc/kernels_xattn.hip) against a float64 CPU
reference on every branch of launch_attention (-m gpu).

Reference, error model (K_FWD, the fp16 floor) and the input families are in tests/attn_fwd_ref.py, which
tests/test_attn_fwd_ref_host.py shows to be achievable by an fp32 emulation and sharp against seeded mistakes.  Every element is held
to  |got - ref| <= K_FWD u bound + u |ref| + tiny  (gpu_util.check_bound; the `[bound]` lines give the worst ratio of each case and
where it is), so one wrong row, or one 16-row fragment that stops a key short, is measured against its own size.

Families: 1 randn, 2 key probes (one row per 16-row fragment puts >= 0.99 of its mass on one key at a tile / granule edge),
3 moving maximum (ramps, a late key TAU -+ 2 / 90 / 300 log2 units above the first tile, a balanced row), 4 uniform softmax and a
single key (bit-exact), 5 strided operands with NaN gaps and an output sentinel; and `negative` (every real score far below the 0 a
key that is not there would have).

V^T pad columns Nk .. ldvt hold NaN where the suite has always used NaN (the automatic non-prescaled path; the fused block) and
zero elsewhere (tests/test_gpu_kernels.py::test_attention_variants: "pad columns must be finite (zero) for v2"; ToMe writes zeros).
"""
import math

import pytest
import torch

import attn_fwd_ref as R
from attn_cases import (BRANCH_CASES, BRANCHES, MOVING_ATTN3_DIMS, MOVING_FOLDED_DIMS, MOVING_SHAPE, QLOOP_DIMS, UNSUPPORTED_DIMS,
                        batch_heads, qloop_shapes, qloop_variants)
from gyre_amd import _lib
from gpu_util import DEV, HDT, check_bound, randn, release_kept, repack_linear, st, vp

pytestmark = pytest.mark.gpu

SENTINEL = 0x7E5A
DIMS = ("sample", "query", "channel")
TAU = R.TAU[HDT]

def run_fwd(q, k, v, heads, presc, variant, layout="dense", vpad="zero"):
    """gyre_op_attention_ex under gyre_debug_force_attn_variant(variant).  layout: dense (ld = C); qk2c - Q and K at columns 0 and
    C of one [B][N][2C] buffer (needs Nq == Nk), as the fused Q|K|V projection leaves them; wide - Q and K at column C of [B][N][3C]
    buffers whose other columns are NaN.  The output goes to column C of a [B][Nq][2C] buffer filled with SENTINEL unless dense.
    Returns (rc, out [B, Nq, C] float32 on the host, the whole output buffer)."""
    L = _lib.lib()
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // heads
    dev = lambda t: t.to(HDT).contiguous().to(DEV)
    if layout == "dense":
        qd, kd, ldq, ldk = dev(q), dev(k), C, C
    elif layout == "qk2c":
        assert Nq == Nk
        buf = dev(torch.cat([q, k], -1))
        qd, kd, ldq, ldk = buf[..., :C], buf[..., C:], 2 * C, 2 * C
    else:
        def place(t):
            b = torch.full((B, t.shape[1], 3 * C), float("nan"), dtype=HDT, device=DEV)
            b[..., C:2 * C] = t.to(HDT).to(DEV)
            return b[..., C:2 * C]
        qd, kd, ldq, ldk = place(q), place(k), 3 * C, 3 * C
    ldvt = (Nk + 7) // 8 * 8
    vt = torch.full((B, C, ldvt), float("nan") if vpad == "nan" else 0.0, dtype=HDT, device=DEV)
    vt[:, :, :Nk] = v.permute(0, 2, 1).to(HDT).to(DEV)
    if layout == "dense":
        obuf = torch.full((B, Nq, C), SENTINEL, dtype=torch.int16, device=DEV).view(HDT)
        o, ldo = obuf, C
    else:
        obuf = torch.full((B, Nq, 2 * C), SENTINEL, dtype=torch.int16, device=DEV).view(HDT)
        o, ldo = obuf[..., C:], 2 * C
    old = L.gyre_debug_force_attn_variant(variant)
    try:
        rc = L.gyre_op_attention_ex(st(), vp(qd), ldq, vp(kd), ldk, vp(vt), ldvt, B, heads, Nq, Nk, D, vp(o), ldo, presc)
    finally:
        L.gyre_debug_force_attn_variant(old)
    release_kept()
    return rc, o.float().cpu(), obuf


def gap_untouched(obuf, C):
    return bool((obuf.view(torch.int16)[..., :C] == SENTINEL).all().cpu())


def check_case(tag, ins, heads, presc, variant, layout="dense", vpad="zero", cache=None):
    """One launch against the float64 reference; returns (worst ratio, output).  cache: a dict that keeps the reference of `ins`
    between variants."""
    q, k, v = ins[:3]
    rc, got, obuf = run_fwd(q, k, v, heads, presc, variant, layout, vpad)
    _lib.check(rc)
    if cache is None or "ref" not in cache:
        ref = R.fwd_ref(q, k, v, heads, presc)
        if cache is not None:
            cache["ref"] = ref
    else:
        ref = cache["ref"]
    w = check_bound(tag, got, ref[0], ref[1], k=R.K_FWD, tiny=R.fwd_tiny(v, HDT), dims=DIMS)
    if layout != "dense":
        assert gap_untouched(obuf, q.shape[-1]), f"{tag}: output columns outside the head block were overwritten"
    return w, got


# the branches, their head dims and shapes, and the kernel family each reaches: tests/attn_cases.py
@pytest.mark.parametrize("branch,D", BRANCH_CASES, ids=[f"{b}-D{D}" for b, D in BRANCH_CASES])
def test_branch_elementwise(branch, D):
    """Families 1, 2 and 5 on every shape the branch takes, `negative` on the key counts with pad columns, uniform softmax, and a
    single key bit for bit."""
    variant, presc, _, shapes, vpad = BRANCHES[branch][:5]
    B, heads = batch_heads(D)
    worst = {}

    def note(fam, w):
        worst[fam] = max(worst.get(fam, 0.0), w)
    for Nq, Nk in shapes:
        tag = f"{branch} D{D} {Nq}x{Nk}"
        note("randn", check_case(f"{tag} randn", R.family_randn(B, heads, Nq, Nk, D, presc, HDT), heads, presc, variant, vpad=vpad)[0])
        probes = R.family_probes(B, heads, Nq, Nk, D, presc, HDT)
        note("probes", check_case(f"{tag} probes", probes, heads, presc, variant, vpad=vpad)[0])
        # family 5 on the probes (a head or row offset slip moves a probed row by its own size)
        cache = {}
        for layout in (("qk2c", "wide") if Nq == Nk else ("wide",)):
            note("strided", check_case(f"{tag} probes {layout}", probes, heads, presc, variant, layout, vpad, cache=cache)[0])
        if Nk % 8 and Nk > 1:
            note("negative", check_case(f"{tag} negative", R.family_negative(B, heads, Nq, Nk, D, presc, HDT), heads, presc, variant,
                                        vpad=vpad)[0])
        if Nq >= 129:
            ins = R.family_uniform(B, heads, Nq, Nk, D, presc, HDT)
            note("uniform", check_case(f"{tag} uniform", ins, heads, presc, variant, vpad=vpad)[0])
        if Nk == 1:
            ins = R.family_randn(B, heads, Nq, 1, D, presc, HDT, seed=5)
            _, got = check_case(f"{tag} one key", ins, heads, presc, variant, vpad=vpad)
            assert torch.equal(got, ins[2].expand_as(got)), f"{tag}: one key (p = 1, sum = 1) must return V's row bit for bit"
    print(f"[branch] {branch} D{D} ({'fp16' if HDT == torch.float16 else 'bf16'}): worst ratio per family "
          + ", ".join(f"{n} {w:.2f}" for n, w in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------------
# family 3: moving maximum, on the folded k_attn2 and on k_attn3
# ---------------------------------------------------------------------------------------------------------------------------
def _moving(B, heads, Nq, Nk, D):
    """name -> (inputs, the side of TAU the case is built for: True above, False below, None wherever its scores fall)"""
    fams = {"ramp_up": (R.family_ramp(B, heads, Nq, Nk, D, 1, HDT, up=True), None),
            "ramp_down": (R.family_ramp(B, heads, Nq, Nk, D, 1, HDT, up=False), None),
            "balanced": (R.family_balanced(B, heads, Nq, Nk, D, 1, HDT), False)}
    for e in (TAU - 2, TAU + 2, 90.0, 300.0):
        fams[f"late_key_{e:g}"] = (R.family_late_key(B, heads, Nq, Nk, D, 1, HDT, e), e > TAU)
    return fams


@pytest.mark.parametrize("D", MOVING_FOLDED_DIMS)
def test_moving_maximum_folded_attn2(D):
    B, heads, Nq, Nk = MOVING_SHAPE
    for name, (ins, _) in _moving(B, heads, Nq, Nk, D).items():
        cache = {}
        _, got = check_case(f"attn2_folded D{D} {name}", ins, heads, 1, 3, cache=cache)
        if name.startswith("late_key"):
            _peaked_row(f"attn2_folded D{D} {name}", got, ins, cache)


def _peaked_row(tag, got, ins, cache):
    row = ins[3]
    ref, bound = (t[:, row:row + 1] for t in cache["ref"])
    check_bound(f"{tag} the peaked row {row}", got[:, row:row + 1], ref, bound, k=R.K_FWD, tiny=R.fwd_tiny(ins[2], HDT), dims=DIMS)


@pytest.mark.parametrize("D", MOVING_ATTN3_DIMS)
def test_moving_maximum_attn3_default_equals_checked_and_counts_its_redos(D):
    """Default (optimistic first pass where built: OPTIMISTIC = D <= 40 in k_attn3) and variant 7 (per-tile check from the start)
    both inside the bound, bit-identical on all of family 3, the peaked row checked on its own; and the redo counter moves exactly
    when a row's first-tile-centred sum reaches 2^TAU - proof that the branch under test ran."""
    L = _lib.lib()
    B, heads, Nq, Nk = MOVING_SHAPE
    for name, (ins, above) in _moving(B, heads, Nq, Nk, D).items():
        q, k, v = ins[:3]
        x = float(R.first_tile_excess(q, k, heads, 1).max())
        if above is not None:
            assert (x > TAU + 0.5) if above else (x < TAU - 0.5), f"{name}: log2 row sum {x:.2f} is on the wrong side of TAU = {TAU}"
        else:                                   # the ramps: the float64 row sums say which side they fall on (if clearly on one)
            above = True if x > TAU + 0.5 else False if x < TAU - 0.5 else None
        cache = {}
        c0 = L.gyre_debug_attn_redo_count()
        _, got0 = check_case(f"attn3 default D{D} {name}", ins, heads, 1, 0, cache=cache)
        c1 = L.gyre_debug_attn_redo_count()
        _, got7 = check_case(f"attn3 checked D{D} {name}", ins, heads, 1, 7, cache=cache)
        c2 = L.gyre_debug_attn_redo_count()
        print(f"[redo] D{D} {name}: log2 of the largest first-tile-centred row sum {x:.2f} (TAU {TAU:g}); redo count +{c1 - c0} default, "
              f"+{c2 - c1} always checked")
        assert c0 >= 0 and c2 == c1, "the always-checked pass never repeats"
        if above is not None:
            if above and D <= 40:
                assert c1 > c0, f"{name}: a row above TAU must send its workgroup through the checked pass"
            else:
                assert c1 == c0, f"{name}: no workgroup should repeat its pass"
        assert torch.equal(got0, got7), f"{name}: the optimistic default must be bit-identical to the always-checked pass"
        if name.startswith("late_key"):
            _peaked_row(f"attn3 default D{D} {name}", got0, ins, cache)


# ---------------------------------------------------------------------------------------------------------------------------
# several query blocks per workgroup (k_attn2<..., QLOOP>)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("presc", [0, 1], ids=["plain", "prescaled"])
@pytest.mark.parametrize("D", QLOOP_DIMS)
def test_qloop_and_its_one_block_form(D, presc):
    """Automatic dispatch (variant 0: QLOOP where expects_qloop says so) and variant 6 (the same without QLOOP) on the same inputs,
    both inside the bound; the first key count outside the ring reaches the one-block form under either (see below for the prescaled
    exception).  prescaled: the folded form for D = 40, 64, 160, the plain form with unit scale for D = 80.  (No
    bit-equality between the two is asserted: the source does not state it.)  Non-prescaled automatic dispatch: NaN V^T pads."""
    vpad = "zero" if presc else "nan"
    for B, heads, Nq, Nk, qiter in qloop_shapes(D):
        assert R.expects_qloop(B, heads, Nq, Nk, D) == qiter, (B, heads, Nq, Nk, D)
        variants = qloop_variants(presc, qiter, Nk)       # (the first key count outside the ring: see there)
        fams = {"randn": (R.family_randn(B, heads, Nq, Nk, D, presc, HDT), ("dense",)),
                "probes": (R.family_probes(B, heads, Nq, Nk, D, presc, HDT), ("dense", "wide"))}
        for fam, (ins, layouts) in fams.items():
            cache = {}
            for layout in layouts:
                for variant in variants:
                    check_case(f"qloop D{D} presc{presc} B{B} h{heads} {Nq}x{Nk} qiter {qiter} v{variant} {fam} {layout}", ins, heads,
                               presc, variant, layout, vpad, cache=cache)


@pytest.mark.parametrize("D", UNSUPPORTED_DIMS)
def test_unsupported_head_dim_returns_minus_six_and_writes_nothing(D):
    B, heads, Nq, Nk = 2, 2, 65, 77
    q, k, v = R.family_randn(B, heads, Nq, Nk, D, 0, HDT)
    for presc in (0, 1):
        rc, _, obuf = run_fwd(q, k, v, heads, presc, 0)
        assert rc == -6, rc
        assert bool((obuf.view(torch.int16) == SENTINEL).all().cpu()), "a refused call must leave the output buffer alone"


# ---------------------------------------------------------------------------------------------------------------------------
# the fused cross-attention block against the chain of operators it replaces
# ---------------------------------------------------------------------------------------------------------------------------
K_XATTN = 3.0


@pytest.mark.parametrize("Nk,probe", [(1, None), (33, 0), (33, 32), (77, 0), (77, 76), (80, 0), (80, 79), (33, None), (77, None), (80, None)])
def test_fused_cross_attention_block_against_its_operator_chain(Nk, probe):
    """gyre_op_cross_attention_block against gyre_op_ln_linear -> gyre_op_attention_ex -> gyre_op_linear (+ bias + residual) on the
    same operands - the operators the tests above and the GEMM tests hold to their own references.  The two may legitimately differ
    only in the fp32 summation order in front of each of the three 16-bit roundings (q, the attention output a, the stored
    result), so a rounding may flip: one u per stage, K_XATTN = 3, on bound = |x| + |bo| + |a| |Wo|^T in float64 with the chain's
    a.  probe = j: in every 16-row fragment one row (all of them the same x row, hence the same q) puts >= 0.99 of its softmax
    mass on key j, whose V row is 4x the others' (family 2 on the first / last key); None: randn (family 1).  NaN V^T pads."""
    L = _lib.lib()
    C_, heads, tokens, B = 320, 8, 4096, 8
    D, M = C_ // heads, B * tokens
    x = randn(B, tokens, C_, seed=401) * 1.5 + 0.2
    rows = R.probe_rows(tokens)
    if probe is not None:
        x[:, rows] = randn(B, 1, C_, seed=402) * 1.5 + 0.2
    x = x.to(HDT).float().reshape(M, C_)
    g, be = randn(C_, seed=403) * 0.2 + 1, randn(C_, seed=404) * 0.2
    wq = (randn(C_, C_, seed=405) / math.sqrt(C_)).to(HDT).float()
    wo = (randn(C_, C_, seed=406) / math.sqrt(C_)).to(HDT).float()
    bo = randn(C_, seed=407) * 0.1
    xd, wqd, wod, gd, bed, bod = x.to(HDT).to(DEV), repack_linear(wq), repack_linear(wo), g.to(DEV), be.to(DEV), bo.to(DEV)
    ws = torch.empty(L.gyre_op_ln_linear_workspace(C_, C_, M), dtype=torch.uint8, device=DEV)
    # chain, step 1: q = LayerNorm(x) Wq^T
    qd = torch.empty(M, C_, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_ln_linear(st(), vp(xd), M, C_, vp(gd), vp(bed), 1e-5, vp(wqd), C_, None, 0, 0, None, 0, None, 0, vp(ws),
                                   ws.numel(), vp(qd)))
    q = qd.float().cpu().reshape(B, tokens, C_)
    k = randn(B, Nk, C_, seed=408) * (R.LOG2E / math.sqrt(D))
    v = randn(B, Nk, C_, seed=409)
    if probe is not None:
        qr = q[:, rows[0]].reshape(B, heads, D).double()
        assert torch.equal(q[:, rows], q[:, rows[:1]].expand(B, len(rows), C_)), "equal x rows must give equal q rows"
        gap = math.log2(99.0 * max(Nk, 2)) + 6.0                                    # log2 units over a typical key
        k[:, probe] = (qr * (gap / (qr * qr).sum(-1, keepdim=True))).float().reshape(B, C_)
        v[:, probe] *= 4.0
    k, v = k.to(HDT).float(), v.to(HDT).float()
    if probe is not None:
        P = (R.heads_of(q[:, rows[:1]], heads) @ R.heads_of(k, heads).transpose(-1, -2) * math.log(2.0)).softmax(-1)
        assert float(P[..., probe].min()) >= 0.99, float(P[..., probe].min())
    ldvt = (Nk + 7) // 8 * 8
    kd = k.to(HDT).to(DEV)
    vt = torch.full((B, C_, ldvt), float("nan"), dtype=HDT, device=DEV)
    vt[:, :, :Nk] = v.permute(0, 2, 1).to(HDT).to(DEV)
    # chain, steps 2 and 3
    ad = torch.empty(M, C_, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_attention_ex(st(), vp(qd), C_, vp(kd), C_, vp(vt), ldvt, B, heads, tokens, Nk, D, vp(ad), C_, 1))
    chain = torch.empty(M, C_, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_linear(st(), vp(ad), M, C_, vp(wod), C_, vp(bod), vp(xd), 0, vp(chain)))
    fused = torch.empty(M, C_, dtype=HDT, device=DEV)
    _lib.check(L.gyre_op_cross_attention_block(st(), vp(xd), M, tokens, C_, heads, vp(gd), vp(bed), 1e-5, vp(wqd), vp(kd), vp(vt), Nk,
                                               ldvt, vp(wod), vp(bod), vp(ws), ws.numel(), vp(fused), None))
    release_kept()
    a = ad.float().cpu().double()
    bound = x.double().abs() + bo.double().abs() + a.abs() @ wo.double().abs().t()
    tag = f"fused cross-attention block vs its chain Nk{Nk} " + ("randn" if probe is None else f"probe on key {probe}")
    check_bound(tag, fused.float().cpu(), chain.float().cpu(), bound, k=K_XATTN, dims=("row", "channel"))
    if probe is not None:
        idx = torch.tensor([b * tokens + r for b in range(B) for r in rows])
        check_bound(tag + ", the probing rows", fused.float().cpu()[idx], chain.float().cpu()[idx], bound[idx], k=K_XATTN,
                    dims=("row", "channel"))
