"""Host self-test of the range-edge family (tests/range_cases.py, tests/range_ref.py): CPU only.

Every row is built for every storage type it exists for, and the conditions its property needs are asserted from the float64
reference alone: the recorded exponents are the derived ones, the scaled maximum lies in (top / 2, top] (bf16: the fp32
intermediate in absolute-value form, in (2^125, 2^126]), every scaled operand is still a value of its type, operands that are claimed
subnormal are, the partial sums of the offset rows really leave fp16, the exclusion cap of check 1 holds, and a torch emulation of
a correct kernel passes both checks.  Then each range mistake the family exists for is seeded into the emulation
(range_ref.MISTAKES; 16-bit token sums and pool sums for the non-GEMM kernels) and must fail check 1 or check 2 on the rows of
the matching property - the evidence that the GPU tests would notice it."""
import ctypes as C

import pytest
import torch

import gemm_cases as GC
import gemm_ref as G
import range_cases as RC
import range_ref as R
from gyre_amd import _lib

F16, BF16 = torch.float16, torch.bfloat16
F64 = torch.float64
PAIRS = [(r["id"], h) for r in RC.ROWS for h in (F16, BF16) if R.NAME[h] in r["only"]]


def pairs(*families):
    return [pytest.param(rid, h, id=f"{rid}-{R.NAME[h]}") for rid, h in PAIRS if RC.BY_ID[rid]["family"] in families]


def in_top_half(m, top):
    return top / 2 < m <= top


def test_table_is_well_formed():
    assert set(RC.EXPS) == {r["id"] for r in RC.ROWS}
    for r in RC.ROWS:
        assert set(RC.EXPS[r["id"]]) == set(r["only"]), r["id"]
        assert r["prop"] in RC.PROPS
    assert {r["prop"] for r in RC.ROWS} == set(RC.PROPS), "a property without a row"
    # the cancellation and offset rows need headroom between storage and accumulator: fp16 only
    assert all(r["only"] == ("f16",) for r in RC.ROWS if r["prop"] in R.OFFSET_PROPS)
    # one row per kernel family for the GEMM properties, the conv configs with and without zero-fill
    for prop in ("top", "cancel", "bias_back", "res_order", "sub_act", "sub_w", "sub_out"):
        cfgs = {r["base"]["cfg"] for r in RC.ROWS if r["family"] == "gemm" and r["prop"] == prop and r["op"] == "linear"}
        assert cfgs >= set(GC.VARIANT_BASE), (prop, cfgs)
    for prop in ("top", "cancel", "bias_back", "res_order", "sub_act", "sub_w"):
        cfgs = {(r["base"]["cfg"], r["base"]["abl"]) for r in RC.ROWS if r["family"] == "conv" and r["prop"] == prop and r["op"] == "conv"}
        assert cfgs == {(c, a) for c in (1, 5, 12, 24) for a in (0, GC.ZFILL)}, (prop, cfgs)
    assert {r["base"]["cfg"] for r in RC.ROWS if r["id"].startswith("splitk-cancel")} == {4, 5, 6, 7, 8, 24}


def test_rows_judged_to_the_last_bit_only():
    """Exactly the Gaussian subnormal-operand rows and the folded LayerNorm with x in the subnormals, on the fp16 build only; and the
    bounded form of check 1 they get still fails a difference of two units, or last-bit differences in more than 1 % of a row."""
    marked = {r["id"] for r in RC.ROWS if R.mfma_subnormal_row(r, F16)}
    want = {r["id"] for r in RC.ROWS if r["prop"] in ("sub_act_gauss", "sub_w_gauss")} | {r["id"] for r in RC.ROWS
                                                                                         if r["op"] == "ln_linear" and r["end"] == "down"}
    assert marked == want and not any(R.mfma_subnormal_row(r, BF16) for r in RC.ROWS)
    w = torch.linspace(0.5, 4.0, 1000, dtype=F64).to(F16).double()
    ex = torch.zeros(1000, dtype=torch.bool)
    one, two = w.clone(), w.clone()
    one[:5] += R.ulp_of(w[:5], F16)
    two[:1] += 2 * R.ulp_of(w[:1], F16)
    assert R.check1(w, w, ex, F16, True) == (0, 0) and R.check1(one, w, ex, F16, True) == (5, 0) and R.check1(two, w, ex, F16, True) == (1, 1)
    many = w + R.ulp_of(w, F16)
    kw = dict(exclude=False, enforce=False, last_bit=True)
    assert not R.judge_scaling("five last bits", F16, (0,), w, one, 0, w, w, 0.0, **kw)["failed"]
    assert R.judge_scaling("two units", F16, (0,), w, two, 0, w, w, 0.0, **kw)["failed"]
    assert R.judge_scaling("every last bit", F16, (0,), w, many, 0, w, w, 0.0, **kw)["failed"]
    assert R.judge_scaling("five last bits, plain row", F16, (0,), w, one, 0, w, w, 0.0, exclude=False, enforce=False)["failed"]


@pytest.mark.parametrize("rid,hdt", pairs("gemm", "conv", "norm", "attn", "xattn", "tome", "elem", "temb", "lora"))
def test_recorded_exponents_are_the_derived_ones(rid, hdt):
    assert tuple(RC.EXPS[rid][R.NAME[hdt]]) == tuple(R.derive(RC.BY_ID[rid], hdt))


def test_scaling_the_operands_is_scaling_the_reference():
    """c1.value is gemm_ref.reference of the SCALED operands; a power of two commutes with every float64 rounding, so it equals
    2^k times the base value bit for bit - which is what lets check 1 compare the two device runs."""
    for rid in ("lin-top-cfg5", "conv-top-cfg24", "geglu-top-cfg6", "lin-sub_act-cfg1"):
        for hdt in (F16, BF16):
            row = RC.BY_ID[rid]
            c0 = R.gemm_base(row, hdt)
            c1 = R.gemm_scaled(row, c0, RC.EXPS[rid][R.NAME[hdt]])
            assert torch.equal(c1.value, c0.value * 2.0 ** c1.k) and torch.equal(c1.bound, c0.bound * 2.0 ** c1.k)


def _plan_runs_the_forced_config(row, c):
    b = row["base"]
    if row["op"] in ("qkv", "conv_nchw") + R.STAT_OPS:
        return                                       # not expressible in the plan query / unforced rows of tests/gemm_cases.py, whose
                                                     # plans tests/test_gemm_ref_host.py asserts
    L = _lib.lib()
    force = b["cfg"] | (b["splits"] << 8 if b["splits"] > 1 else 0)
    old, oab = L.gyre_debug_force_gemm_cfg(force), L.gyre_debug_gemm_ablation(b["abl"])
    if b["cfg"] == GC.AR:
        L.gyre_debug_set_ar_workspace(C.c_void_p(4096), 1 << 30)
    try:
        rc, plan = G.plan_query(L, G.gemm_test_args(c, None, 0, (4096, 1 << 40)))
    finally:
        L.gyre_debug_force_gemm_cfg(old), L.gyre_debug_gemm_ablation(oab), L.gyre_debug_set_ar_workspace(None, 0)
    assert rc == 0, (row["id"], rc, L.gyre_last_error())
    assert plan["cfg"] == b["cfg"] and plan["splits"] == max(1, b["splits"]), (row["id"], plan)
    if b["feats"].get("wblk"):
        assert plan["w_block"] == 1, row["id"]


@pytest.mark.parametrize("rid,hdt", pairs("gemm", "conv"))
def test_gemm_row_conditions(rid, hdt):
    row = RC.BY_ID[rid]
    prop, f16 = row["prop"], hdt == F16
    c0 = R.gemm_base(row, hdt)
    c1 = R.gemm_scaled(row, c0, RC.EXPS[rid][R.NAME[hdt]])
    odt = R.out_dtype(row, hdt)
    top = R.TOP[hdt]
    if row["op"] == "shortcut":
        # the planner-sized fold (its plan is asserted by tests/test_gemm_ref_host.py): operands stay storage values, the scaled
        # maximum is at the top, the exact value passes both checks
        for c in (c0, c1):
            assert all(R.representable(t, hdt) for t in (c.a1, c.w, c.sc, c.w_sc)) and R.representable(c.bias + c.bias_sc, torch.float32)
        assert in_top_half(float(c1.value.abs().max()) if f16 else float(c1.inter), top)
        assert float(c1.inter) / 2.0 ** c1.k < 2.0 ** 24, "every partial sum an exact fp32 integer times 2^k"
        assert not R.judge_gemm(row, c0, c1, G.rne(c0.value, hdt), G.rne(c1.value, hdt), hdt)["failed"]
        return
    _plan_runs_the_forced_config(row, c0)
    for c in (c0, c1):
        for t in (c.a1, c.w, c.residual):
            assert t is None or R.representable(t, hdt), f"{rid}: an operand is not a value of the storage type"
        for t in (c.bias, c.rowbias):
            assert t is None or R.representable(t, torch.float32)
    assert torch.equal(c1.value, c0.value * 2.0 ** c1.k + c1.offset), "the scaled problem is 2^k times the base problem (+ offset)"
    vmax, imax = float(c1.value.abs().max()), float(c1.inter.max())
    A, W, bias, rb, res = R.operands(c1)
    lattice = row["base"]["kind"] != "gauss"
    if lattice:
        # exact in fp32 in any order: every partial sum is a multiple of the smallest product below 2^24 of them
        q = 2.0 ** c1.k
        assert float(c1.bound.max()) / q < 2.0 ** 24 and bool(((c1.value / q) == (c1.value / q).round()).all())
        assert bool((G.rne(c1.value, torch.float32).double() == c1.value).all())
    if prop in ("top", "geglu"):
        if row["op"] == "conv_nchw" and not f16:
            if odt == F16:
                assert 65520 <= vmax <= 2 * 65504 and float(c1.value.abs().min()) < 65504, "some outputs inf, some finite"
            else:
                assert in_top_half(imax, top)
        elif row["op"] in R.STAT_OPS and not f16:
            ssq = float(R.stats_of(row, c1)[..., 1].max())
            assert 2.0 ** 124 < ssq <= 2.0 ** 126, "the largest fp32 sum of squares, within a factor 4 of 2^126 (k moves it by 4)"
        else:
            assert in_top_half(vmax if f16 else imax, top), (vmax, imax)
        if row["op"] in R.STAT_OPS:
            st = R.stats_of(row, c1)
            assert float(st[..., 1].max()) / 4.0 ** c1.k < 2.0 ** 24, "every sum of squares is an exact fp32 value"
        if prop == "geglu" and f16:
            assert float(G.geglu_value_abs(A, W, bias).max()) > 65504, "the value half must leave fp16 before the product brings it back"
    if prop in R.OFFSET_PROPS:
        assert in_top_half(vmax, top)
        acc = A @ W.T
        if prop == "cancel":
            if c1.conv:
                Cin = c1.a_shape[-1]
                first = torch.tensor([t * Cin + ch for t in range(9) for ch in range(64)])     # the first 64-channel chunk, all taps
            else:
                steps = (c1.K + 63) // 64
                per = (steps + max(1, row["base"]["splits"]) - 1) // max(1, row["base"]["splits"]) if row["base"]["splits"] > 1 else steps // 2
                first = torch.arange(per * 64)
            part = A[:, first] @ W[:, first].T
            assert float(part.abs().min()) > 65504, "every output's first partial sum must leave fp16"
            assert float(acc.abs().max()) <= 65504
        elif prop in ("bias_back", "rowbias_back"):
            assert float(acc.abs().min()) > 65504, "the accumulator must be out of range before the bias"
        else:
            assert float(acc.abs().max()) <= 65504 and float(res.abs().max()) <= 65504
            over = ((acc + bias).abs() > 65504).double().mean()
            assert float(over) > 0.95, "accumulator + bias must exceed the top before the residual (all but the odd element)"
    if prop == "sub_act_gauss" and f16:
        assert R.all_subnormal(c1.a1, F16) and float(c1.a1.abs().max()) * 2.0 ** 24 > 128, "subnormals with eight and more significant bits"
    if prop == "sub_w_gauss" and f16:
        assert R.all_subnormal(c1.w, F16) and float(c1.w.abs().max()) * 2.0 ** 24 > 128
    if prop == "sub_act" and f16:
        assert R.all_subnormal(c1.a1, F16) and float(c1.value[c1.value != 0].abs().min()) >= 2.0 ** -14
    if prop == "sub_w" and f16:
        assert R.all_subnormal(c1.w, F16) and float(c1.value[c1.value != 0].abs().min()) >= 2.0 ** -14
    if prop == "sub_out":
        n = c1.value * 2.0 ** 24
        assert bool((n == n.round()).all()) and float(n.abs().max()) <= 1023 and float(n.abs().max()) > 0
        assert R.all_subnormal(c1.residual, F16)
    if not lattice:
        ex = R.excluded_mask(c0.value, c1.value, hdt)
        assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel(), f"{rid}: {int(ex.sum())} of {ex.numel()} elements would be excluded"
    # a correct kernel passes both checks
    res = R.judge_gemm(row, c0, c1, R.emulate_gemm(c0, hdt, odt=odt), R.emulate_gemm(c1, hdt, odt=odt), hdt)
    assert not res["failed"]


MISTAKE_ROWS = {
    "narrow_before_bias": ("bias_back", "rowbias_back"),
    "narrow_before_residual": ("res_order",),
    "splitk_16bit_partials": ("cancel",),
    "geglu_value_narrowed": ("geglu",),
    "flush_subnormal_operands": ("sub_act", "sub_w", "sub_act_gauss", "sub_w_gauss"),
    "flush_subnormal_results": ("sub_out",),
}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_seeded_gemm_mistakes_are_caught(mistake):
    """The mistake is in the kernel, so it is in the base run and in the scaled run alike; every row of the matching property must
    fail (fp16 storage, where the range ends)."""
    assert set(MISTAKE_ROWS) == set(R.MISTAKES)
    rows = [r for r in RC.ROWS if r["family"] in ("gemm", "conv") and r["prop"] in MISTAKE_ROWS[mistake] and r["op"] != "qkv"
            and (mistake != "splitk_16bit_partials" or r["base"]["splits"] > 1)]
    assert rows
    caught = 0
    for row in rows:
        c0 = R.gemm_base(row, F16)
        c1 = R.gemm_scaled(row, c0, RC.EXPS[row["id"]]["f16"])
        res = R.judge_gemm(row, c0, c1, R.emulate_gemm(c0, F16, mistake), R.emulate_gemm(c1, F16, mistake), F16, enforce=False)
        caught += res["failed"]
        assert res["failed"], f"{mistake} passes both checks on {row['id']}"
    print(f"[seeded] {mistake}: caught on {caught} of {len(rows)} rows")


# ---- normalisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,hdt", pairs("norm"))
def test_norm_row_conditions(rid, hdt):
    import norm_fwd_ref as N
    row = RC.BY_ID[rid]
    x, gamma, beta = R.norm_inputs(row, hdt)
    (k,) = RC.EXPS[rid][R.NAME[hdt]]
    x1 = x.double() * 2.0 ** k
    assert R.representable(x.double(), hdt) and R.representable(x1, hdt), "x and 2^k x are values of the storage type"
    eps0, eps1 = R.eps_scaled(0), R.eps_scaled(k)
    assert R.representable(torch.tensor([eps1], dtype=F64), torch.float32) and eps1 >= 2.0 ** -126
    ssq = R.norm_sumsq_max(row, x) * 4.0 ** k
    if row["op"] == "gn_fold":
        W, bias = R.fold_weights(row, hdt)
        wf0 = N.fold_ref(x, row["shape"]["G"], gamma, beta, eps0, W, bias)
        wf1 = N.fold_ref(x1, row["shape"]["G"], gamma, beta, eps1, W, bias)
        assert torch.allclose(wf1[0], wf0[0] * 2.0 ** -k, rtol=1e-12, atol=0) and torch.allclose(wf1[2], wf0[2], rtol=1e-9, atol=1e-12)
        if hdt == F16:
            assert in_top_half(float(wf1[0].abs().max()), 65504.0), "the float64 folded weights reach the top and stay below it"
            ex = R.excluded_mask(wf0[0], wf1[0], hdt)
            assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel()
    elif row["end"] == "up":
        if hdt == F16:
            assert in_top_half(float(x1.abs().max()), 65504.0)
        else:
            assert 2.0 ** 124 < ssq <= 2.0 ** 126, "the largest fp32 sum of squares, within a factor 4 of 2^126 (k moves it by 4)"
    else:
        if hdt == F16:
            assert R.all_subnormal(x1, F16)
        assert float(x1[x1 != 0].abs().min()) ** 2 >= 2.0 ** -125 or hdt == F16
    assert ssq < 2.0 ** 127 and float(x1[x1 != 0].abs().min()) ** 2 > 2.0 ** -149
    # the float64 reference is invariant (what check 1 demands of the device, bit for bit)
    if row["op"] == "ln_linear":
        s = row["shape"]
        L = _lib.lib()
        assert L.gyre_debug_ln_linear_folds(s["M"], s["C"], row["N"], row["geglu"]) and not L.gyre_debug_ln_linear_folds(
            s["M"] - 1, s["C"], row["N"], row["geglu"]), "the smallest M the planner keeps folded"
        W, bias = R.ln_linear_weights(row, hdt)
        r0 = R.ln_linear_ref(row, x[:64], gamma, beta, eps0, W, bias, hdt)[0]
        r1 = R.ln_linear_ref(row, x1[:64], gamma, beta, eps1, W, bias, hdt)[0]
        assert torch.allclose(r0, r1, rtol=1e-9, atol=1e-11)
    elif row["op"] == "layernorm":
        r0, r1 = N.ln_ref(x, gamma, beta, eps0)[0], N.ln_ref(x1, gamma, beta, eps1)[0]
        assert torch.allclose(r0, r1, rtol=1e-10, atol=1e-12)
    elif row["op"] != "gn_fold":
        G_ = row["shape"]["G"]
        r0, r1 = N.gn_ref(x[:1], G_, gamma, beta, eps0, 0, True)[0], N.gn_ref(x1[:1], G_, gamma, beta, eps1, 0, True)[0]
        assert torch.allclose(r0, r1, rtol=1e-10, atol=1e-12)


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,hdt", pairs("attn"))
def test_attention_row_conditions(rid, hdt):
    import attn_cases as AC
    import attn_fwd_ref as A
    row = RC.BY_ID[rid]
    q, k, v, heads, presc, variant, vpad = R.attn_inputs(row, hdt)
    assert row["D"] in AC.BRANCHES[row["branch"]][2], "the branch takes this head dim"
    (kk,) = RC.EXPS[rid][R.NAME[hdt]]
    v1 = v.double() * 2.0 ** kk
    assert all(R.representable(t.double(), hdt) for t in (q, k, v)) and R.representable(v1, hdt)
    if row["D"] == 512 and row["end"] == "up":
        ref0 = A.fwd_ref(q[:1], k[:1], v[:1], heads, presc)[0]
        ref1 = A.fwd_ref(q[:1], k[:1], v1[:1].float() if hdt == F16 else v1[:1], heads, presc)[0]
    else:
        ref0, ref1 = A.fwd_ref(q, k, v, heads, presc)[0], A.fwd_ref(q, k, v1, heads, presc)[0]
    assert torch.allclose(ref1, ref0 * 2.0 ** kk, rtol=1e-12, atol=0)
    if row["end"] == "up":
        if hdt == F16:
            assert in_top_half(float(v1.abs().max()), 65504.0)
        else:
            assert in_top_half(2.0 ** A.TAU[hdt] * v.shape[1] * float(v1.abs().max()), 2.0 ** 126)
        assert int(R.excluded_mask(ref0, ref1, hdt).sum()) == 0 and float(ref0.abs().min()) > 0.3, "no output anywhere near zero"
    else:
        Nk = v.shape[1]
        assert Nk in (64, 256) and not bool(q.any())
        if hdt == F16:
            assert R.all_subnormal(v1, F16)
        n = ref1 * 2.0 ** 24
        assert bool((n == n.round()).all()) and 0 < float(n.abs().max()) <= Nk, "outputs on the subnormal lattice, exact"
        assert R.representable(ref0, hdt) and R.representable(ref1, hdt)


# ---- token merging ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,hdt", pairs("tome"))
def test_tome_row_conditions_and_16_bit_token_sums_are_caught(rid, hdt):
    import tome_exact_ref as X
    row = RC.BY_ID[rid]
    keys, v, r = R.tome_inputs(row, hdt)
    (kk,) = exps = RC.EXPS[rid][R.NAME[hdt]]
    v1 = v.double() * 2.0 ** kk
    assert R.representable(v1, hdt)
    order, node_idx, _, reff = X.select64(keys, r)
    u = 2.0 ** -8 if hdt == BF16 else 2.0 ** -11
    if row["op"] == "tome_unmerge":
        dy1 = v1[:, :v.shape[1] - reff]
        assert in_top_half(float(dy1.abs().max()), R.TOP[hdt])
        return
    ref0, cnt, _ = X.merge_wavg64(v, order, node_idx, reff)
    ref1, _, absmean1 = X.merge_wavg64(v1, order, node_idx, reff)
    assert int(cnt.max()) >= 3, "a row that merges three tokens"
    three = (cnt >= 3)[..., None]
    sums = (ref1 * cnt[..., None].double()).abs()
    if hdt == F16:
        assert in_top_half(float(v1.abs().max()), 65504.0)
        assert float(sums[three.expand_as(sums)].max()) > 65504 and float(ref1.abs().max()) <= 65504, "a sum of three beyond the top, its mean inside"
    else:
        assert in_top_half(float((absmean1 * cnt[..., None]).max()), 2.0 ** 126)
    ex = R.excluded_mask(ref0, ref1, hdt)
    assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel()
    tol = X.merge_tolerance(ref1, cnt, absmean1, u)
    out = {}
    for mistake in (None, "token_sum_16bit"):
        g0, g1 = R.tome_emulate(v, order, node_idx, reff, hdt, mistake), R.tome_emulate(v1.float(), order, node_idx, reff, hdt, mistake)
        ratio = float(((g1 - ref1).abs() / tol).nan_to_num(nan=float("inf")).max())
        out[mistake] = R.judge_scaling(rid, hdt, exps, g0, g1, kk, ref0, ref1, ratio, enforce=False)["failed"]
    assert not out[None]
    assert out["token_sum_16bit"] or hdt == BF16, "a 16-bit token sum must fail on the fp16 rows"


# ---- element-wise ------------------------------------------------------------------------------------------------------------------------------
def test_cast_specials_hold_what_they_claim():
    sp = R.cast_specials("f32")
    h, b = sp.to(F16), sp.to(BF16)
    one = lambda v: torch.tensor([v], dtype=F64).float()
    assert float(one(65519.99).half()) == 65504 and torch.isinf(one(65520.0).half()) and float(one(1 + 2.0 ** -11).half()) == 1.0
    assert float(one(1 + 3 * 2.0 ** -11).half()) == 1 + 2.0 ** -9 and float(one(2.0 ** -25).half()) == 0 and float(one(1.5 * 2.0 ** -24).half()) == 2.0 ** -23
    assert bool(torch.isinf(h).any()) and bool(torch.isnan(h).any()) and bool(((h != 0) & (h.abs().double() < 2.0 ** -14)).any())
    assert bool(((b != 0) & (b.abs().double() < 2.0 ** -126)).any()) and float(one(2.0 ** -134).bfloat16()) == 0
    for src in ("f32", "bf16", "f16"):
        x = R.cast_image(src, (2, 9, 240))
        assert x.dtype == R.SRC_DT[src] and bool(torch.isnan(x).any()) and bool(torch.isinf(x).any())


@pytest.mark.parametrize("rid,hdt", [p for p in pairs("elem") if RC.BY_ID[p.values[0]]["op"] == "avgpool2"])
def test_avgpool_rows_and_16_bit_pool_sums(rid, hdt):
    row = RC.BY_ID[rid]
    x = R.avgpool_inputs(row, hdt)
    (kk,) = exps = RC.EXPS[rid][R.NAME[hdt]]
    x1 = x.double() * 2.0 ** kk
    assert R.representable(x.double(), hdt) and R.representable(x1, hdt)
    ref0, _ = R.avgpool_ref(x)
    ref1, mabs1 = R.avgpool_ref(x1)
    sub = row["prop"] == "sub_out"
    if sub:
        n = ref1 * 2.0 ** 24
        assert bool((n == n.round()).all()) and 0 < float(n.abs().max()) <= 252
        assert R.all_subnormal(x1, F16) or hdt == BF16
    else:
        assert in_top_half(float(x1.abs().max()) * (1 if hdt == F16 else 4), R.TOP[hdt])
        assert float((ref1.abs() * 4).max()) > R.TOP[hdt] / (1 if hdt == F16 else 4) and float(ref1.abs().max()) <= R.TOP[hdt]
        ex = R.excluded_mask(ref0, ref1, hdt)
        assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel()
    tol = R.avgpool_tolerance(ref1, mabs1, hdt)
    out = {}
    for mistake in (None, "pool_sum_16bit", "flush_subnormal_operands", "flush_subnormal_results"):
        g0, g1 = R.avgpool_emulate(x, hdt, mistake), R.avgpool_emulate(x1, hdt, mistake)
        ratio = float(((g1 - ref1).abs() / tol).nan_to_num(nan=float("inf")).max())
        out[mistake] = R.judge_scaling(rid, hdt, exps, g0, g1, kk, ref0, ref1, ratio, exclude=not sub, exact=G.rne(ref1, hdt) if sub else None,
                                       enforce=False)["failed"]
    assert not out[None]
    if hdt == F16:
        assert out["pool_sum_16bit"] != sub, "a 16-bit pool sum is inf on the top row"
        assert (out["flush_subnormal_operands"] and out["flush_subnormal_results"]) == sub, "flushed subnormals fail the lattice row"


# ---- time embedding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,hdt", pairs("temb"))
def test_temb_row_conditions(rid, hdt):
    import temb_ref as T
    row = RC.BY_ID[rid]
    x, W, bias = R.temb_inputs(row, hdt)
    (kk,) = RC.EXPS[rid][R.NAME[hdt]]
    W1 = W.double() * 2.0 ** kk
    assert R.representable(W.double(), hdt) and R.representable(W1, hdt)
    assert R.all_subnormal(W1, F16) or hdt == BF16
    ref0, _ = T.linear64(x, W, bias, False)
    ref1, _ = T.linear64(x, W1, bias.double() * 2.0 ** kk, False)
    assert torch.equal(ref1, ref0 * 2.0 ** kk)
    assert int(R.excluded_mask(ref0, ref1, torch.float32).sum()) == 0


# ---- the fused cross-attention block -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hdt", [F16, BF16], ids=["f16", "bf16"])
def test_xattn_block_row_conditions(hdt):
    rid = "xattn-block-top-Nk77"
    row = RC.BY_ID[rid]
    ins = R.xattn_inputs(row, hdt)
    x, v, bo = ins[0], ins[5], ins[7]
    (kk,) = RC.EXPS[rid][R.NAME[hdt]]
    assert all(R.representable(t.double() * 2.0 ** e, hdt) for t in (x, v) for e in (0, kk))
    assert R.representable(bo.double() * 2.0 ** kk, torch.float32)
    ref0 = R.xattn_ref(row, ins)[0]
    assert float(ref0.abs().min()) > 1.0 and int(R.excluded_mask(ref0, ref0 * 2.0 ** kk, hdt).sum()) == 0, "no output anywhere near zero"
    if hdt == F16:
        assert in_top_half(float(ref0.abs().max()) * 2.0 ** kk, 65504.0)
    else:
        assert 2.0 ** 124 < float((x.double() ** 2).sum(1).max()) * 4.0 ** kk <= 2.0 ** 126


# ---- LoRA / LyCORIS ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,hdt", pairs("lora"))
def test_lora_row_conditions_and_flushed_results_are_caught(rid, hdt):
    import numpy as np
    import lora_ref as LRF
    import lyco_ref as LY
    row = RC.BY_ID[rid]
    (kk,) = exps = RC.EXPS[rid][R.NAME[hdt]]
    if row["op"] == "lyco_core":
        core, right = R.lyco_core_inputs(row)
        c1 = torch.from_numpy(core).double() * 2.0 ** kk
        assert R.representable(c1, F16) and R.all_subnormal(c1, F16)
        return
    case, base, terms = R.lora_inputs(row, hdt)
    name, O, I, KH, KW, I_pad, geglu, scale_p = case[:8]
    base1, terms1 = R.lora_scaled(row, base, terms, kk)
    ref0, _, _ = R.lora_ref(row, case, base, terms, hdt)
    ref1, tol1, absform = R.lora_ref(row, case, base1, terms1, hdt)
    assert np.array_equal(ref1, ref0 * 2.0 ** kk)
    assert not ref1[..., I:].any()
    ref0, ref1, tol1 = ref0[..., :I], ref1[..., :I], tol1[..., :I]              # (pad columns: exact zeros, asserted apart)
    r0, r1 = torch.from_numpy(ref0.copy()), torch.from_numpy(ref1.copy())
    lattice = row["data"] == "lattice"
    if row["end"] == "up":
        if hdt == F16:
            assert in_top_half(float(np.abs(ref1).max()), 65504.0)
        else:
            assert float(np.abs(ref1).max()) <= 2.0 ** 126 and (absform is None or in_top_half(float(absform.max()), 2.0 ** 126))
    else:
        n = ref1 * 2.0 ** 24
        assert np.array_equal(n, np.round(n)) and 0 < np.abs(n).max() <= 64 and (hdt == BF16 or R.all_subnormal(r1, F16))
    if lattice:
        assert R.representable(r0, hdt) and R.representable(r1, hdt)
    else:
        ex = R.excluded_mask(r0, r1, hdt)
        assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel()
    emu = (lambda b, t: LRF.emulate(b, t, I_pad, geglu, scale_p, storage=hdt)) if row["op"] == "repack_lora" else \
          (lambda b, t: LY.emulate(b, t, I_pad, geglu, scale_p))
    to16 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(hdt).double().reshape(O, KH, KW, I_pad)[..., :I]
    g0, g1 = to16(emu(base, terms)), to16(emu(base1, terms1))
    out = {}
    for mistake in (None, "flush_subnormal_results"):
        f = (lambda t: R.flush(t, hdt)) if mistake else (lambda t: t)
        err = np.abs(f(g1).numpy() - ref1)
        ratio = float(np.nan_to_num(np.where(err == 0, 0.0, err / np.where(err == 0, 1.0, tol1)), nan=np.inf).max())
        out[mistake] = R.judge_scaling(rid, hdt, exps, f(g0), f(g1), kk, r0, r1, ratio, exclude=not lattice, exact=r1 if lattice else None,
                                       enforce=False)["failed"]
    assert not out[None]
    if hdt == F16 and row["end"] == "down":
        assert out["flush_subnormal_results"], "a store that flushes subnormals must fail the subnormal merge rows"


def test_residual_add_targets_reach_the_edges():
    """The residual that takes a skip tensor to 65504 / 65519.99 / 65520 / the subnormal ends does so in the fp32 sum the kernel forms."""
    skip = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(1)).to(F16).float()
    for src in ("f32", "bf16", "f16"):
        r = R.residual_targets(skip, src)
        want = R.residual_expected(skip, r, F16)
        assert r.dtype == R.SRC_DT[src] and want.dtype == F16
        if src == "f32":
            assert bool(torch.isinf(want).any()) and bool((want.float().abs() == 65504).any())
            assert bool(((want != 0) & (want.float().abs() < 2.0 ** -14)).any())
