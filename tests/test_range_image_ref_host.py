"""Host self-test of the range-edge family of the image-model kernels (tests/range_image_cases.py, tests/range_image_ref.py): CPU only.

Every row is built for every storage type it exists for, and the conditions its property needs are asserted from the float64
reference alone: the recorded exponents are the derived ones, the scaled maximum lies in (top / 2, top] (bf16: the largest fp32
intermediate in absolute-value form), every scaled operand is still a value of its type, operands claimed subnormal are, the
intermediate of the offset rows really leaves fp16, the exclusion cap of check 1 holds on reference against reference, and a host
emulation of a correct kernel passes the checks the GPU runner applies.  Then each mistake the family exists for is seeded into the
emulation (range_image_ref.MISTAKES) and must fail those checks on the rows of the matching property."""
import pytest
import torch

import hat_ref as HT
import lineart_ref as LA
import range_image_cases as IC
import range_image_ref as Q
import range_ref as R

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
PAIRS = [(r["id"], h) for r in IC.ROWS for h in (F16, BF16) if R.NAME[h] in r["only"]]


def pairs(pred):
    return [pytest.param(rid, h, id=f"{rid}-{R.NAME[h]}") for rid, h in PAIRS if pred(IC.BY_ID[rid])]


def in_top_half(m, top):
    return top / 2 < m <= top


def scaling(r):
    return r["family"] in Q.SCALING_FAMILIES


def test_table_is_well_formed():
    assert set(IC.IMAGE_EXPS) == {r["id"] for r in IC.ROWS}
    for r in IC.ROWS:
        assert set(IC.IMAGE_EXPS[r["id"]]) == set(r["only"]), r["id"]
        assert r["op"] in Q.OPS or r["family"] == "cast", r["id"]
    assert all(r["only"] == ("f16",) for r in IC.ROWS if r["prop"] in ("epi_back", "res_order"))
    props = {"epi_back", "gate_back", "saturate", "specials", "top", "sub_act", "sub_w", "cancel", "sub_out", "invariant", "cast", "res_order",
             "convex", "logit_shift"}
    assert props == {r["prop"] for r in IC.ROWS}
    # every kernel of the specials list has its row, and each of those rows records what torch gives
    ops = {r["op"] for r in IC.ROWS if r["prop"] == "specials"}
    assert ops == {"hed_tail", "inorm", "ln_live", "swin_act", "silu", "cab", "rdb_epilogue", "ctrl_emit_acc", "conv7_out", "hed_fuse"}
    assert all(r.get("torch") for r in IC.ROWS if r["prop"] == "specials")


@pytest.mark.parametrize("rid,hdt", pairs(lambda r: True))
def test_recorded_exponents_are_the_derived_ones(rid, hdt):
    assert tuple(IC.IMAGE_EXPS[rid][R.NAME[hdt]]) == tuple(Q.derive(IC.BY_ID[rid], hdt))


def _operands(P):
    """the tensors of a problem that are stored in the 16-bit type"""
    names = ("x", "c2", "y", "buf", "r1", "r2", "xp", "w", "res")
    return {n: P[n] for n in names if torch.is_tensor(P.get(n)) and not (n == "w" and "xp" not in P)}


def _emulated(row, hdt, P0, P1, mistake=None):
    op = Q.OPS[row["op"]]
    return op.emulate(row, P0, hdt, mistake), op.emulate(row, P1, hdt, mistake)


def _saturation_conditions(P1, l0, t0, k):
    """the scaled minimum over the sure elements lies in [SAT, 2 SAT), nothing overflows fp32, both saturated values occur among the
    sure elements, and the unsure ones (a base logit within twice its fp32 bound of zero) stay under the exclusion cap"""
    sure = P1["sure"]
    assert torch.equal(sure, l0.abs() > 2 * t0) and int((~sure).sum()) <= R.EXCLUDE_CAP * sure.numel()
    assert Q.SAT <= float(l0[sure].abs().min()) * 2.0 ** k < 2 * Q.SAT and float(l0.abs().max()) * 2.0 ** k < 2.0 ** 100
    assert bool(P1["sign"][sure].any()) and not bool(P1["sign"][sure].all()), "both saturated values occur"


@pytest.mark.parametrize("rid,hdt", pairs(scaling))
def test_scaling_row_conditions(rid, hdt):
    row = IC.BY_ID[rid]
    op, prop, f16 = Q.OPS[row["op"]], row["prop"], hdt == F16
    exps = IC.IMAGE_EXPS[rid][R.NAME[hdt]]
    P0, P1 = Q.problems(row, hdt, exps)
    top = R.TOP[hdt]
    for P in (P0, P1):
        for n, t in _operands(P).items():
            assert R.representable(t.double(), hdt), f"{rid}: operand {n} is not a value of the storage type"
        for n in ("bias", "b", "s", "eps"):
            if n in P and P[n] is not None:
                t = P[n] if torch.is_tensor(P[n]) else torch.tensor([P[n]])
                assert R.representable(t.double(), F32) and bool(torch.isfinite(t).all()), f"{rid}: {n} is not an fp32 value"
    o0, o1 = op.outputs(row, P0, hdt), op.outputs(row, P1, hdt)
    # the float64 reference scales as check 1 demands of the device
    for name, o in o1.items():
        if o.k is not None:
            assert torch.allclose(o.value, o0[name].value * 2.0 ** o.k + o.offset, rtol=1e-9, atol=0 if o.k else 1e-11), (rid, name)
    k = sum(exps)
    if row["op"] == "hed_tail":
        x1 = P1["x"].double()
        if prop == "top":
            mag = (x1.clamp_min(0) * P1["w"].double()).abs().sum(-1)
            assert in_top_half(float(x1.abs().max()) if f16 else float(mag.max()), top)
        else:
            assert R.all_subnormal(x1, F16) and float(P1["b"].abs().max()) == 0
            assert float(o1["pool"].value.abs().max()) > 0 and R.all_subnormal(o1["pool"].value, F16)
    elif row["op"] == "inorm":
        x1 = P1["x"].double()
        d = Q.inorm.shifted(P1["x"])
        ssq = float((d * d).sum((1, 2)).max())
        if row["end"] == "up":
            assert in_top_half(float(x1.abs().max()), top) if f16 else 2.0 ** 124 < ssq <= 2.0 ** 126
        else:
            assert R.all_subnormal(x1, F16) if f16 else float(d[d != 0].abs().min()) ** 2 >= 2.0 ** -125
        assert ssq < 2.0 ** 127 and P1["eps"] >= 2.0 ** -126
        # the data is where a variance without the shift cancels: the mean is a hundred times the spread
        m, rstd, _, _, _, _ = LA.inorm_stats_ref(P0["x"].to(hdt), P0["eps"])
        assert float((m.abs() * rstd).min()) > 50
        chunks = -(-row["shape"][1] * row["shape"][2] // 512)
        assert chunks in (1, 15), "one chunk, and 15 chunks across the eight slices"
    elif row["op"] == "ln_live":
        x1 = P1["x"].double()
        ssq = float((x1 * x1).sum(1).max())
        if row["end"] == "up":
            assert in_top_half(float(x1.abs().max()), top) if f16 else 2.0 ** 124 < ssq <= 2.0 ** 126
        else:
            assert R.all_subnormal(x1, F16) if f16 else float(x1[x1 != 0].abs().min()) ** 2 >= 2.0 ** -125
        assert bool((o1["out"].value[:, row["shape"]["C"]:] == 0).all()), "the pad columns stay zero"
    elif row["op"] == "chan_pool":
        live = P1["c2"][..., :P1["C"]].double().abs()
        if f16:
            assert in_top_half(float(live.max()), top)
            assert 2 * float(live.min()) > 65504 >= float(o1["pool"].value.abs().max()), "no 16-bit partial of two elements is in range, the mean is"
        else:
            assert in_top_half(float(live.sum(1).max()), top)
        assert not bool(P1["c2"][..., P1["C"]:].any())
    elif row["op"] == "scale_add":
        c2, y, v = P1["c2"].double(), P1["y"].double(), o1["y"].value
        if prop == "gate_back":
            assert in_top_half(max(float(c2.abs().max()), float(y.abs().max()), float(v.abs().max())), top)
            assert float(c2.abs().max()) > top / 4 and 0 < float(P1["s"].max()) <= 0.01 * (1 + 2.0 ** -20), "c2 near the top, a small gate"
        else:
            assert all(R.all_subnormal(t, F16) for t in (c2, y, v)) and R.representable(v, hdt)
            n = v * 2.0 ** 24
            assert bool((n == n.round()).all()) and 0 < float(n.abs().max()) <= 127
        assert not bool(v[..., P1["C"]:].any()), "the pad channels stay zero"
    elif row["op"] == "rdb_epilogue":
        v, G = Q.rdb_epilogue.value(P1)
        if prop == "epi_back":
            s = slice(P1["c0"], P1["c0"] + P1["live"])
            step1 = P1["alpha"] * (P1["buf"][:, s].double() + P1["bias"].double())
            assert float(step1.min()) > 65504 and in_top_half(float(v.abs().max()), 65504.0) and float(v.min()) > 0
            if P1["r2"] is not None:
                assert float((step1 + P1["beta1"] * P1["r1"].double()).max()) > 65504, "rrdb form: still beyond the top after beta1 r1, in range after beta2 r2"
            assert R.representable(v, hdt) and bool((G * 2.0 ** -k < 2.0 ** 24).all()), "every step an exact fp32 integer times 2^k"
        else:
            m = max(float(t.abs().max()) for t in (P1["buf"], P1["r1"], P1["r2"], v) if t is not None)
            assert in_top_half(m if f16 else float(G.max()), top)
    elif row["op"] == "hed_fuse":
        l0, t0 = Q.hed_fuse.logits(P0)
        _saturation_conditions(P1, l0, t0, k)
    elif row["op"] == "conv7_out":
        l0, t0 = LA.conv7_out_ref(P0["xp"], P0["w"], P0["b"], 0)
        if prop == "saturate":
            _saturation_conditions(P1, l0, t0, k)
        else:
            assert in_top_half(float(l0.abs().max()) * 2.0 ** k, 65504.0)
    elif row["op"] == "ups4":
        import ctypes as C
        import ups4_ref as U4
        from gyre_amd import _lib
        B, Hi, Wi, Cin, N = Q.ups4.shape(row)
        # the smallest problem the plan rule takes under tuning bit 30: config 24, unsplit; a narrower chunk or fewer outputs are not taken
        L = _lib.lib(_lib.F16 if f16 else _lib.BF16)
        old = L.gyre_debug_gemm_ablation(Q.UPS4_ALL)
        try:
            q = (C.c_int32 * 4)()
            assert L.gyre_debug_ups4_plan(B, Hi, Wi, Cin, N, 0, 0, 0, 0, q) == 0 and tuple(q)[:3] == (1, 24, 1)
            assert L.gyre_debug_ups4_plan(1, 1, 1, 56, 8, 0, 0, 0, 0, q) == 0 and q[0] == 0
            assert L.gyre_debug_ups4_plan(1, 1, 1, 64, 7, 0, 0, 0, 0, q) != 0 and L.gyre_debug_ups4_plan(1, 0, 1, 64, 8, 0, 0, 0, 0, q) != 0
        finally:
            L.gyre_debug_gemm_ablation(old)
        x1, w1 = P1["x"], P1["w"]
        wc0, wc1 = U4.compose(P0["w"]), U4.compose(w1)
        v1, b1 = Q.ups4.reference(P1)
        assert all(R.representable(t, hdt) for t in (x1, w1)) and R.representable(P1["bias"], F32)
        assert torch.allclose(U4.forward(x1, wc1) + P1["bias"], v1, rtol=1e-12, atol=1e-300), "four parities = nine taps on the upsampled image"
        live = wc1.abs().amax(dim=(1, 4))                                   # [parity, ty, tx]: the taps a 1 x 1 image reads
        if prop == "top":
            assert in_top_half(float(v1.abs().max()) if f16 else float(b1.max()), top)
        else:
            assert R.representable(wc1, hdt), "every composed weight, a sum of up to four taps, is a storage value"
            assert float(b1.max()) * 2.0 ** -k < 2.0 ** 24, "every partial sum an exact fp32 integer times 2^k"
        if prop == "cancel":
            w0 = w1.clone()
            w0[..., 1:] = 0
            first = Q.ups4.reference(dict(P1, w=w0, bias=P1["bias"] * 0))[0]
            assert float(first.abs().min()) > 65504 and in_top_half(float(v1.abs().max()), 65504.0) and Cin == 128
        if prop == "sub_act":
            assert R.all_subnormal(x1, F16) and float(v1[v1 != 0].abs().min()) >= 2.0 ** -14
        if prop == "sub_w":
            assert R.all_subnormal(w1, F16) and R.all_subnormal(wc1, F16) and float(v1[v1 != 0].abs().min()) >= 2.0 ** -14
            # each parity's live tap at the one source pixel is a sum of FOUR nine-tap weights
            for a in (0, 1):
                for b in (0, 1):
                    four = sum(P0["w"][:, ky, kx] for ky in U4.tap_groups(a)[1 - a] for kx in U4.tap_groups(b)[1 - b])
                    assert len(U4.tap_groups(a)[1 - a]) == 2 and torch.equal(wc0[2 * a + b, :, 1 - a, 1 - b], four)
    elif row["op"] == "merge_delta":
        import numpy as np
        import merge_delta_ref as MD
        ref0, ref1 = MD.ref64(P0["base"], P0["terms"]), MD.ref64(P1["base"], P1["terms"])
        odt = R.SRC_DT[row["out"]]
        assert MD.on_lattice(ref0) and np.array_equal(ref1, ref0 * 2.0 ** k) and R.representable(torch.from_numpy(ref1.copy()), odt)
        assert P1["base"].dtype == np.float32 and all(np.isfinite(np.float32(u)) for _, u in P1["terms"])
        if row["end"] == "up":
            m = float(np.abs(ref1).max())
            assert in_top_half(m, 65504.0) if odt == F16 else in_top_half(m * 256.0, 2.0 ** 126)
        else:
            n = ref1 * 2.0 ** 24
            assert np.array_equal(n, np.round(n)) and 0 < np.abs(n).max() <= 1023 and R.all_subnormal(torch.from_numpy(ref1.copy()), F16)
    elif row["op"] == "conv7_in":
        ref1, t1 = LA.conv7_in_ref(P1["x"], P1["w"], P1["b"])
        mag = t1 / ((49 * 8 + 2) * Q.E)
        if prop == "top":
            assert in_top_half(float(ref1.abs().max()) if f16 else float(mag.max()), top)
        else:
            sub = P1["x"] if prop == "sub_act" else P1["w"]
            assert R.all_subnormal(sub.double(), F16) and float(ref1[ref1 != 0].abs().min()) >= 2.0 ** -14
            assert float(mag.max()) * 2.0 ** -k * 256 < 2.0 ** 24, "every partial sum an exact fp32 integer over 256, times 2^k"
    elif row["op"] == "rdb_conv":
        import rrdb_ref as RB
        L0, L1 = P0["L"], P1["L"]
        Cin, live = L1["Cin"], L1["live"]
        for L in (L0, L1):
            ops = [L["x"][..., :Cin], L["w"], L["r1"], L["r2"]]
            assert all(t is None or bool(torch.isfinite(t.float()).all()) for t in ops), "an operand left its storage type"
            assert R.representable(L["bias"].double(), F32)
        x1, w1 = L1["x"][..., :Cin].double(), L1["w"].double()
        v, A, G = RB.value64(L1)
        acc = RB._sum(L1, F64)
        if prop == "top":
            m = max(float(t.abs().max()) for t in (v, L1["r1"], L1["r2"]) if t is not None)
            assert in_top_half(m if f16 else max(float(G.max()), abs(L1["alpha"]) * float(A.max())), top)
        else:
            assert float(G.max()) * 2.0 ** -k < 2.0 ** 24, "every partial sum and every step of the epilogue an exact fp32 integer times 2^k"
        if prop == "cancel":
            w0 = L1["w"].clone()
            w0[..., 1:] = 0
            first = RB._sum(dict(L1, w=w0), F64)              # channel 0 alone: what a kernel holds after the first channel's nine taps
            assert float(first.abs().min()) > 65504 >= float(acc.abs().max()) and in_top_half(float(v.abs().max()), 65504.0)
        if prop == "epi_back":
            step1 = L1["alpha"] * (acc + L1["bias"].double())
            assert float(step1.min()) > 65504 and in_top_half(float(v.abs().max()), 65504.0) and float(v.min()) > 0
            assert float((step1 + L1["beta1"] * L1["r1"].double()).max()) > 65504, "still beyond the top after beta1 r1, in range after beta2 r2"
        if prop == "sub_act":
            assert R.all_subnormal(x1, F16) and float(v[v != 0].abs().min()) >= 2.0 ** -14
        if prop == "sub_w":
            assert R.all_subnormal(w1, F16) and float(v[v != 0].abs().min()) >= 2.0 ** -14
        if prop == "sub_out":
            n = acc * 2.0 ** 24
            assert bool((n == n.round()).all()) and 0 < float((v * 2.0 ** 24).abs().max()) <= 1023 and R.all_subnormal(o1["slice"].value, F16)
    elif row["family"] == "attn":
        t0, t1 = Q._qkv_view(P0["L"]).double(), Q._qkv_view(P1["L"]).double()
        assert R.representable(t0, hdt) and R.representable(t1, hdt), "q, k, v and their scaled forms are storage values"
        assert not bool(t1[..., 30:].any()), "the two pad columns of every head stay zero"
        if prop == "logit_shift":
            up, down = (0, 1) if row["dir"] == "q_up" else (1, 0)
            assert in_top_half(float(t1[:, up].abs().max()), 65504.0) and R.all_subnormal(t1[:, down], F16)
            assert torch.equal(t1[:, 2], t0[:, 2]) and torch.equal(o1["o"].value, o0["o"].value), "the float64 value does not move"
        elif row["end"] == "up":
            assert in_top_half(float(t1[:, 2].abs().max()), top) and float(o0["o"].value.abs().min()) > 0.3, "no output anywhere near zero"
        else:
            n = o1["o"].value * 2.0 ** 24
            assert R.all_subnormal(t1[:, 2], F16) and not bool(t1[:, 0].any()) and 0 < float(n.abs().max()) < 1024
            if Q.win_attn.lattice(row):
                assert bool(((n - n.round()).abs() < 1e-9).all()) and R.representable(n.round() * 2.0 ** -24, hdt), "outputs on the subnormal lattice"
            else:
                assert o1["o"].k is None
        if row["op"] == "hat_attn" and row["case"][0] == "oca":
            valid = HT._oca_windows(P0["L"], F64)[3]
            assert bool((~valid).reshape(valid.shape[0], -1).any(1).all()), "every window has keys outside the image"
    else:
        raise AssertionError(f"no conditions written for {row['op']}")
    # reference against reference: what check 1 would leave out, from the float64 values alone
    for name, o in o1.items():
        if o.k is not None:
            ex = Q.excluded(o0[name], o)
            assert int(ex.sum()) <= R.EXCLUDE_CAP * ex.numel(), f"{rid}: {int(ex.sum())} of {ex.numel()} elements of {name} would be excluded"
    # a correct kernel passes both checks
    assert not Q.judge(row, hdt, exps, P0, P1, *_emulated(row, hdt, P0, P1))["failed"]


@pytest.mark.parametrize("rid,hdt", pairs(lambda r: r["family"] == "act"))
def test_activation_row_conditions(rid, hdt):
    row = IC.BY_ID[rid]
    op = Q.OPS[row["op"]]
    P = op.base(row, hdt)
    x = P["x"].double()
    fi = torch.finfo(hdt)
    assert R.representable(x, hdt) and x.numel() % 8 == 0
    if row["prop"] == "top":
        assert float(x.max()) == fi.max and float(x.min()) == -fi.max and float(x.abs().min()) > fi.max / 2
        ref = op.outputs(row, P, hdt)["x"].value
        assert torch.equal(ref[x > 0].to(hdt), P["x"].to(hdt)[x > 0]), "f(x) rounds to x itself for the positive inputs: f(top) is top"
    else:
        assert float(x.abs().max()) < fi.smallest_normal and float(x.abs().max()) == fi.smallest_normal * (1 - fi.eps)
        assert float(x.abs().min()) == fi.smallest_normal * fi.eps
    out = {m: Q.judge_single(row, hdt, P, op.emulate(row, P, hdt, m), enforce=False)["failed"]
           for m in (None, "flush_subnormal_operands", "flush_subnormal_results")}
    assert not out[None]
    if row["prop"] == "sub_out" and hdt == F16:
        assert out["flush_subnormal_operands"] and out["flush_subnormal_results"], "flushed subnormals must fail the subnormal rows"


@pytest.mark.parametrize("rid,hdt", pairs(lambda r: r["family"] == "cast"))
def test_cast_rows_hold_the_edges(rid, hdt):
    row = IC.BY_ID[rid]
    P, want = Q.cast_problem(row, hdt)
    if row["prop"] == "res_order":
        prod = P["scale"] * P["f"].double()
        assert float(prod.min()) > 65504 and float(P["out"].double().abs().max()) <= 65504, "every product beyond the top"
        assert bool(torch.isfinite(want).all()) and in_top_half(float(want.double().abs().max()), 65504.0)
        bad = Q.ctrl_emit_acc.emulate(row, P, hdt, "rounded_before_accumulate")["out"]
        assert R.same_bits(bad, want) > 0 and not bool(torch.isfinite(bad).all()), "a product narrowed before the sum must fail"
        return
    src = next(v for v in P.values() if torch.is_tensor(v) and v.numel() > 55)
    assert bool(torch.isnan(src).any()) and bool(torch.isinf(src).any()) and bool((src == 0).any())
    w = want.double()
    assert bool(torch.isnan(w).any()) and bool(torch.isinf(w).any())
    if want.dtype != F32:
        lim = float(torch.finfo(want.dtype).smallest_normal)
        assert bool(((w != 0) & (w.abs() < lim)).any()) or (want.dtype == BF16 and src.dtype == F16), "subnormal outputs"
    if want.dtype == F16 and src.dtype != F16 and row["op"] not in ("swin_exit", "swin_entry"):      # (those keep 3 of 8 channels)
        assert int(torch.isinf(w).sum()) > int(torch.isinf(src).sum()), "finite values above 65520 become inf in an fp16 output, as torch's cast makes them"


MISTAKE_ROWS = {
    "flush_subnormal_operands": lambda r: (r["op"], r["prop"]) in (("hed_tail", "sub_act"), ("scale_add", "sub_out"), ("rdb_conv", "sub_act"),
                                                                    ("rdb_conv", "sub_w"), ("conv7_in", "sub_act"), ("conv7_in", "sub_w"),
                                                                    ("ups4", "sub_act"), ("ups4", "sub_w")),
    "flush_subnormal_results": lambda r: (r["op"], r["prop"]) in (("hed_tail", "sub_act"), ("scale_add", "sub_out"), ("rdb_conv", "sub_out")) or (
        r["op"] == "merge_delta" and r["end"] == "down" and r["out"] == "f16"),
    "pool_16bit_partials": lambda r: r["op"] == "chan_pool",
    "variance_unshifted": lambda r: r["op"] == "inorm" and r["prop"] == "invariant",
    "rounded_before_residual": lambda r: r["prop"] == "epi_back",
    # q goes into the subnormals on the k_up rows: a scale multiplied into the 16-bit q is rounded absolutely there
    "scale_folded_into_q": lambda r: r["prop"] == "logit_shift" and r["dir"] == "k_up",
    # a peaked softmax: the output's error is the rounding of one or two P values, and bf16's is eight times fp16's
    "p_narrowed_twice": lambda r: r["family"] == "attn" and bool(r.get("peaked")),
}
MISTAKE_ROWS["flush_subnormal_operands"] = lambda r, f=MISTAKE_ROWS["flush_subnormal_operands"]: f(r) or (
    r["family"] == "attn" and (r["prop"] == "logit_shift" or r["end"] == "down"))


@pytest.mark.parametrize("mistake", sorted(MISTAKE_ROWS))
def test_seeded_range_mistakes_are_caught(mistake):
    """The mistake is in the kernel, so it is in the base run and in the scaled run alike; every row of the matching property must fail
    (fp16 storage, where the range ends; the variance without the shift on both)."""
    assert mistake in Q.MISTAKES
    rows = [r for r in IC.ROWS if MISTAKE_ROWS[mistake](r)]
    assert rows
    for row in rows:
        for hdt in ((F16, BF16) if mistake == "variance_unshifted" else (F16,)):
            exps = IC.IMAGE_EXPS[row["id"]][R.NAME[hdt]]
            P0, P1 = Q.problems(row, hdt, exps)
            res = Q.judge(row, hdt, exps, P0, P1, *_emulated(row, hdt, P0, P1, mistake), enforce=False)
            assert res["failed"], f"{mistake} passes both checks on {row['id']} ({R.NAME[hdt]})"
    print(f"[seeded] {mistake}: caught on {len(rows)} rows")


@pytest.mark.parametrize("rid,hdt", pairs(lambda r: r["prop"] == "specials"))
def test_specials_rows_and_a_dropped_nan(rid, hdt):
    """The inputs hold all three specials and leave samples clean; torch's evaluation has every class among its outputs' classes that
    the row is about; the host emulation of a correct kernel passes, and fmaxf semantics (nan_dropped_by_max) fail on the four kernels
    that have a max in them."""
    row = IC.BY_ID[rid]
    op = Q.OPS[row["op"]]
    P = op.base(row, hdt)
    Ps = op.specials(row, P, hdt)
    changed = [n for n in P if torch.is_tensor(P[n]) and not torch.equal(torch.nan_to_num(P[n].double(), 7.0, 8.0, 9.0),
                                                                         torch.nan_to_num(Ps[n].double(), 7.0, 8.0, 9.0))]
    changed += [n for n in P if isinstance(P[n], list) and any(not bool(torch.isfinite(t).all()) for t in Ps[n])]
    assert changed, rid
    seen = set()
    for n in changed:
        for t in (Ps[n] if isinstance(Ps[n], list) else [Ps[n]]):
            seen |= set(Q.classes(t).unique().tolist())
    assert seen == {0, 1, 2, 3}, f"{rid}: +inf, -inf and NaN among finite values"
    want = op.torch_eval(row, Ps, hdt)
    assert any(3 in Q.classes(w).unique().tolist() for w in want.values()), "torch gives a NaN somewhere"
    clean, spec = op.emulate(row, P, hdt), op.emulate(row, Ps, hdt)
    assert not Q.judge_specials(row, hdt, P, Ps, clean, spec, enforce=False)["failed"]
    if row["op"] in ("hed_tail", "inorm", "cab"):
        bad = op.emulate(row, Ps, hdt, "nan_dropped_by_max")
        assert Q.judge_specials(row, hdt, P, Ps, clean, bad, enforce=False)["classdiff"] > 0, "fmaxf semantics must fail the row"
