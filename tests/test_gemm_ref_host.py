"""Host self-test of the GEMM / convolution reference, its exact lattice and its error model (tests/gemm_ref.py, tests/gemm_cases.py):
no GPU.

  * the gather reference against independent ATen formulations in float64 for every geometry variant;
  * every row of the case table built on the CPU: its lattice conditions hold (asserted inside gemm_ref.build_case);
  * gelu_erf_f transcribed into numpy float32: error against float64 erf-GELU measured and printed (the GEGLU tolerance term is twice
    it), gelu(0) == 0 and gelu(16) == 16 exactly (the GEGLU lattice stands on that);
  * an fp32 emulation of a correct kernel (64-wide K chunks, taps inside chunks, one rounding): passes the lattice bit for bit and the
    bound with a ratio <= 0.5 measured on the fp32 value BEFORE the store;
  * seeded mistakes in that emulation: each must be caught by the lattice, the wide lattice or the bound; printed next to it is
    whether the whole-tensor rel-L2 <= 4e-3 of tests/test_gpu_kernels.py would have let it through.  EXPECTATION: several pass the
    rel-L2, none passes the new checks;
  * the planner's answers (gyre_debug_gemm_plan, no device) for every row that states them, and the coverage list: every id of
    g_tiles and every dispatch feature is reached by at least one row."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as GC
import gemm_ref as R
from gyre_amd import _lib

F64 = torch.float64
DTS = (torch.bfloat16, torch.float16)


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _flat(y):     # NCHW -> [M][N]
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


# ---- 1. the gather against ATen ----------------------------------------------------------------------------------------------------
GEOMETRIES = [dict(), dict(stride=2), dict(stride=2, pad=0), dict(ups=1), dict(ups=1, crop=1), dict(ups=1, crop=1, stride=2),
              dict(wrap=1), dict(wrap=2), dict(wrap=3), dict(wrap=3, ups=1), dict(wrap=1, ups=1, crop=1), dict(stride=1, pad=0)]


@pytest.mark.parametrize("g", GEOMETRIES, ids=lambda g: "-".join(f"{k}{v}" for k, v in g.items()) or "plain")
@pytest.mark.parametrize("B,H,W,Cin,C1", [(3, 9, 7, 16, 0), (1, 17, 17, 24, 8), (2, 2, 3, 8, 0)])
def test_gather_reference_matches_aten(g, B, H, W, Cin, C1):
    stride, pad, ups, crop, wrap = g.get("stride", 1), g.get("pad", 1), g.get("ups", 0), g.get("crop", 0), g.get("wrap", 0)
    N = 12
    x, w, b = _rand((B, Cin, H, W), 1), _rand((N, Cin, 3, 3), 2), _rand((N,), 3)
    # independent formulation: interpolate (+ crop), explicit padding per axis, F.conv2d
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    if crop:
        xi = xi[:, :, :2 * H - 1, :2 * W - 1]
    if pad == 0:
        xp = F.pad(xi, (0, 1, 0, 1))                                   # the asymmetric downsampler pad
    else:
        xp = F.pad(xi, (1, 1, 0, 0), mode="circular") if wrap & 1 else F.pad(xi, (1, 1, 0, 0))
        xp = F.pad(xp, (0, 0, 1, 1), mode="circular") if wrap & 2 else F.pad(xp, (0, 0, 1, 1))
    want = F.conv2d(xp, w, b, stride=stride)
    Hup, Wup = (2 * H - 1, 2 * W - 1) if crop else (0, 0)
    xs = _nhwc(x)
    # two sources: torch.cat of the halves IS the single tensor; the reference takes them split at C1
    src = R.two_sources(xs[..., :C1], xs[..., C1:]) if C1 else xs
    A = R.conv_gather(src, stride, pad, ups, Hup, Wup, wrap).reshape(-1, 9 * Cin)
    Wm = w.permute(0, 2, 3, 1).reshape(N, 9 * Cin)
    got, bound = R.reference(A, Wm, b)
    assert (want.shape[2], want.shape[3]) == R.conv_out_size(H, W, stride, pad, ups, Hup, Wup)
    assert torch.allclose(got, _flat(want), rtol=0, atol=1e-12)
    wantb = F.conv2d(xp.abs(), w.abs(), b.abs(), stride=stride)
    assert torch.allclose(bound, _flat(wantb), rtol=0, atol=1e-12)


def test_linear_forms_match_aten():
    M, K, N, C1 = 34, 40, 32, 16
    a, w, b = _rand((M, K), 1), _rand((N, K), 2), _rand((N,), 3)
    rb, res = _rand((2, N), 4), _rand((M, N), 5)
    got, bound = R.reference(R.two_sources(a[:, :C1], a[:, C1:]), w, b, rb, 17, res)
    want = F.linear(torch.cat([a[:, :C1], a[:, C1:]], dim=1), w, b) + rb.repeat_interleave(17, 0) + res
    assert torch.allclose(got, want, atol=1e-12) and bool((bound >= got.abs() - 1e-12).all())
    # GEGLU: value | gate halves, erf form
    wg, bg = _rand((2 * N, K), 6), _rand((2 * N,), 7)
    got, bound = R.reference(a, wg, bg, geglu=True)
    h = F.linear(a, wg, bg)
    assert torch.allclose(got, h[:, :N] * F.gelu(h[:, N:]), atol=1e-12)
    il = R.geglu_interleave(wg)
    assert torch.equal(il[0:16], wg[0:16]) and torch.equal(il[16:32], wg[N:N + 16]) and torch.equal(il[32:48], wg[16:32])
    # transposed / fused V^T layouts and the folded 1x1 shortcut as a separate convolution
    t = R.transposed(got, 17, 24, -3.0)
    assert t.shape == (2, N, 24) and torch.equal(t[1, 5, :17], got[17:, 5]) and bool((t[:, :, 17:] == -3.0).all())
    x, s1, s2 = _rand((2, 8, 5, 5), 8), _rand((2, 8, 5, 5), 9), _rand((2, 16, 5, 5), 10)
    w3, wsc = _rand((N, 8, 3, 3), 11), _rand((N, 24), 12)
    want = F.conv2d(x, w3, b, padding=1) + F.conv2d(torch.cat([s1, s2], 1), wsc[:, :, None, None])
    A = torch.cat([R.conv_gather(_nhwc(x)).reshape(50, 72), _nhwc(s1).reshape(50, 8), _nhwc(s2).reshape(50, 16)], dim=1)
    got, _ = R.reference(A, torch.cat([w3.permute(0, 2, 3, 1).reshape(N, 72), wsc], dim=1), b)
    assert torch.allclose(got, _flat(want), atol=1e-12)
    assert torch.equal(R.nchw(got, 2, 5, 5), got.reshape(2, 5, 5, N).permute(0, 3, 1, 2))
    st_ = R.colstats(got, 25, 8)
    assert st_.shape == (2, 4, 2) and torch.allclose(st_[1, 2, 0], got[25:, 16:24].sum()) and torch.allclose(st_[0, 0, 1], (got[:25, :8] ** 2).sum())
    rs = R.rowstats(got, 20)
    assert rs.shape == (2, 50, 2) and torch.allclose(rs[1, 7, 0], got[7, 20:].sum())


# ---- 2. every row of the table -------------------------------------------------------------------------------------------------------
def test_every_row_builds_and_meets_its_lattice_conditions():
    ids = set()
    n = {"lattice": 0, "wide": 0, "gauss": 0, "stat": 0}
    for r in GC.ROWS:
        assert r["id"] not in ids
        ids.add(r["id"])
        assert all(cv in GC.COVERAGE for cv in r["covers"]), r["covers"]
        assert bool(r["rc"]) == bool(r["why"]) or not r["rc"], f"{r['id']}: a refusal names its rule"
        for dt in (DTS if r["kind"] == "gauss" else DTS[:1]):          # lattice data does not depend on the storage type
            c = R.build_case(r, dt)                                  # asserts |exact| <= 256 (32), integers, exact partial sums
            if r["kind"] in ("lattice", "stat", "wide"):
                for h in DTS:                                        # representable in BOTH storage types
                    st_ = R.expected_store(c, h)
                    if r["kind"] != "wide":
                        assert torch.equal(st_.to(F64), c.value)
        if r["kind"] == "stat" and r["op"] in ("colstats_conv", "colstats_linear"):
            rows = r["plan"]["colstat_rows"]
            assert float(R.colstats(c.value, rows, r["feats"]["unit"])[..., 1].max()) < 2.0 ** 24
        if r["op"] == "rowstats":
            bn = {t[0]: t[2] for t in _tiles(_lib.lib())}[r["plan"]["cfg"]]
            assert r["kind"] == "stat" and float(R.rowstats(c.value, bn)[..., 1].max()) < 2.0 ** 24 and float(c.value.abs().max()) <= R.STAT_MAX
        if r["kind"] == "wide":
            h = R.expected_store(c, torch.bfloat16).to(F64)
            assert float((h != c.value).double().mean()) > 0.5, "the wide lattice must need a rounding"
        n[r["kind"]] += 1
    print(f"[table] {len(GC.ROWS)} rows: {n}")
    assert min(n.values()) > 0


# ---- 3. gelu_erf_f -------------------------------------------------------------------------------------------------------------------
def test_gelu_transcription():
    x = np.arange(-12 * 1024, 12 * 1024 + 1, dtype=np.float64) / 1024.0
    got = R.gelu_erf_f_np(x.astype(np.float32)).astype(np.float64)
    ref = R.gelu64(torch.from_numpy(x)).numpy()
    err = np.abs(got - ref)
    big = np.abs(ref) > 1e-3
    print(f"[gelu] gelu_erf_f (numpy float32 transcription) vs float64 erf-GELU over [-12, 12], step 2^-10: max abs err {err.max():.3e} at "
          f"x = {x[err.argmax()]:.4f}, max rel err {(err[big] / np.abs(ref[big])).max():.3e} where |gelu| > 1e-3")
    assert err.max() <= R.GELU_ABS_ERR, "gemm_ref.GELU_ABS_ERR is the measured value: update it with the kernel's polynomial"
    assert err.max() >= 0.5 * R.GELU_ABS_ERR, "GELU_ABS_ERR is not a loose guess"
    assert R.gelu_erf_f_np(np.float32(0.0)) == 0.0 and R.gelu_erf_f_np(np.float32(16.0)) == 16.0
    assert float(R.gelu64(torch.tensor(16.0, dtype=F64))) == 16.0
    # max |gelu'|: the factor of the gate's error in the GEGLU bound
    d = np.diff(ref) * 1024.0
    assert np.abs(d).max() <= R.GELU_DERIV_MAX


# ---- 4. / 5. the emulation and the seeded mistakes --------------------------------------------------------------------------------------
TOL_L2 = 4e-3


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _problem(kind, dt, conv=None, M=289, K=200, N=328, geglu=False, rowbias=False, res=True, rps=17, seed=7, geom=None):
    """Operands of one problem in float64 storage values (gemm_ref.make_operands: the table's own generator); conv = (B, H, W, Cin)."""
    geom = geom or {}
    if conv:
        B, H, W, Cin = conv
        a_shape, K = (B, H, W, Cin), 9 * Cin
        Ho, Wo = R.conv_out_size(H, W, geom.get("stride", 1), geom.get("pad", 1), geom.get("ups", 0), geom.get("Hup", 0), geom.get("Wup", 0))
        M, rps = B * Ho * Wo, Ho * Wo
    else:
        a_shape = (M, K)
    Nw = 2 * N if geglu else N
    a, w, bias, rb, rs = R.make_operands(kind, dt, a_shape, (Nw, K), M, N, K, rps, seed, geglu, True, rowbias, res and not geglu)
    return dict(a=a, W=w, bias=bias, rowbias=rb, rps=rps, residual=rs, geglu=geglu, conv=conv, geom=geom, K=K, M=M, N=N)


def _A(p, bug=None):
    if p["conv"]:
        return R.conv_gather(p["a"], bug=bug, **p["geom"]).reshape(p["M"], p["K"])
    return p["a"]


def _emulate(p, bug=None, gather_bug=None, splits=1, A=None, residual="same"):
    A = _A(p, gather_bug) if A is None else A
    cin = p["conv"][3] if p["conv"] else 0
    return R.emulate_fp32(A, p["W"], p["bias"], p["rowbias"], p["rps"], p["residual"] if isinstance(residual, str) else residual,
                          p["geglu"], conv_cin=cin, splits=splits, bug=bug)


def _verdict(kind, dt, p, acc32, pre_round=None):
    """(caught, rel_l2 passes) of an fp32 result before the store under the instrument of its data kind."""
    value, bound = R.reference(_A(p), p["W"], p["bias"], p["rowbias"], p["rps"], p["residual"], p["geglu"])
    stored = acc32.to(dt) if pre_round is None else pre_round
    l2 = _rel_l2(stored, value)
    if kind == "gauss":
        from gpu_util import check_bound
        tiny = 2 * R.GELU_ABS_ERR * R.geglu_value_abs(_A(p), p["W"], p["bias"]) if p["geglu"] else 0.0
        ratio = check_bound("seeded", stored, value, bound, k=R.gauss_k(p["K"], dt), tiny=tiny, hdt=dt, enforce=False)
        return ratio > 1.0, l2 <= TOL_L2, ratio
    want = R.rne(value, dt)
    ndiff = int((stored != want).sum())
    return ndiff > 0, l2 <= TOL_L2, ndiff


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_emulated_correct_kernel_passes(dt):
    cases = [("linear K tail", dict()), ("linear two chunks", dict(K=128)), ("conv uniform", dict(conv=(3, 9, 7, 64))),
             ("conv non-uniform", dict(conv=(3, 9, 7, 8))), ("conv upsample crop", dict(conv=(3, 9, 7, 64), geom=dict(ups=1, Hup=17, Wup=13))),
             ("conv row bias", dict(conv=(3, 9, 7, 64), rowbias=True)), ("geglu", dict(K=192, N=176, geglu=True)),
             ("split K", dict(K=2304, N=64))]
    for name, kw in cases:
        splits = 5 if name == "split K" else 1
        for kind in ("lattice", "wide", "gauss"):
            if kind == "wide" and kw.get("geglu"):
                continue
            p = _problem(kind, dt, **kw)
            acc = _emulate(p, splits=splits)
            value, bound = R.reference(_A(p), p["W"], p["bias"], p["rowbias"], p["rps"], p["residual"], p["geglu"])
            if kind != "gauss":
                if kind == "lattice":
                    R.assert_lattice("lattice", value, bound)
                assert torch.equal(acc.to(dt), R.rne(value, dt)), f"{name} {kind}: the emulation of a correct kernel is not exact"
                continue
            # fp32 part: the value BEFORE the store against the tolerance WITHOUT its u |ref| term
            tiny = 2 * R.GELU_ABS_ERR * R.geglu_value_abs(_A(p), p["W"], p["bias"]) if p["geglu"] else 0.0
            tol = p["K"] * 2.0 ** -23 * bound + tiny
            r32 = float(((acc.double() - value).abs() / tol.clamp_min(1e-300)).max())
            caught, l2ok, ratio = _verdict(kind, dt, p, acc)
            print(f"[emu] {_name(dt)} {name}: fp32 part {r32:.3f} of K 2^-23 bound, rounded output ratio {ratio:.3f}")
            assert r32 <= 0.5 and ratio <= 1.0


MISTAKES = [
    # name, data kinds that must catch it (first listed = the instrument recorded), problem, how
    ("one product dropped", ("lattice",), dict(K=2880, N=64), dict(bug="one_product")),
    ("last K chunk dropped in one tile column", ("lattice",), dict(K=2880, N=128), dict(bug="last_chunk_col")),
    ("K tail (K % 64 = 8) dropped", ("lattice",), dict(K=200), dict(bug="k_tail")),
    ("bias shifted by 4 columns in the last N tile", ("lattice",), dict(), dict(bug="bias_shift")),
    ("residual read with ldr = N where ldr = N + 16", ("lattice",), dict(), dict(special="ldr")),
    ("ky / kx transposed", ("lattice",), dict(conv=(3, 9, 7, 64)), dict(gather_bug="kykx")),
    ("right-edge padding off by one", ("lattice",), dict(conv=(3, 9, 7, 64)), dict(gather_bug="right_edge")),
    ("asymmetric pad applied to the wrong side", ("lattice",), dict(conv=(3, 9, 7, 64), geom=dict(stride=2, pad=0)), dict(gather_bug="asym_wrong_side")),
    ("upsample source index rounded up", ("lattice",), dict(conv=(3, 9, 7, 64), geom=dict(ups=1)), dict(gather_bug="ups_round_up")),
    ("Hup = 2H - 1 crop ignored", ("lattice",), dict(conv=(3, 9, 7, 64), geom=dict(ups=1, Hup=17, Wup=13)), dict(gather_bug="crop_ignored")),
    ("wrap applied on one side only", ("lattice",), dict(conv=(3, 9, 7, 64), geom=dict(wrap=3)), dict(gather_bug="wrap_one_side")),
    ("C1 split off by 8 channels", ("lattice",), dict(K=200), dict(special="c1")),
    ("sample boundary ignored inside a tile", ("lattice",), dict(conv=(3, 9, 7, 64), rowbias=True), dict(bug="sample_boundary")),
    ("one split-K slab dropped", ("lattice",), dict(K=2304, N=64), dict(bug="slab", splits=5)),
    ("rounding before the residual add", ("wide", "gauss"), dict(), dict(special="round_twice")),
    # at the K of the table's GEGLU rows (192; 320 for the A-resident kernel), so that the verdict is what the GPU rows can see
    ("tanh-GELU in place of erf (K = 192)", ("gauss",), dict(K=192, N=176, geglu=True), dict(bug="tanh_gelu")),
    ("tanh-GELU in place of erf (K = 320)", ("gauss",), dict(K=320, N=192, geglu=True), dict(bug="tanh_gelu")),
    ("value / gate pairing shifted by one 16-row group", ("lattice",), dict(K=192, N=176, geglu=True), dict(bug="pairing")),
]


@pytest.mark.parametrize("dt", DTS, ids=_name)
def test_seeded_mistakes_are_caught(dt):
    """Each mistake, on the instrument that is meant to see it and on Gaussian data under the OLD whole-tensor check."""
    passed_old = []
    for name, kinds, kw, how in MISTAKES:
        results = []
        for kind in kinds:
            p = _problem(kind, dt, **kw)
            sp = how.get("special")
            pre = None
            if sp == "ldr":          # rows of a [M][N + 16] residual buffer read with stride N
                buf = R._padded(p["residual"], 16, fill=R.PAD_POISON).reshape(-1)
                acc = _emulate(p, residual=buf[:p["M"] * p["N"]].reshape(p["M"], p["N"]))
            elif sp == "c1":         # sources split at 64 but read as if split at 72: 8 channels of the second source come from the first's pad
                a = p["a"]
                A = torch.cat([a[:, :64], torch.full((p["M"], 8), R.PAD_POISON, dtype=F64), a[:, 64:-8]], dim=1)
                acc = _emulate(p, A=A)
            elif sp == "round_twice":
                noq = _emulate(p, residual=None)
                pre = (noq.to(dt).float() + p["residual"].float()).to(dt)
                acc = None
            else:
                acc = _emulate(p, bug=how.get("bug"), gather_bug=how.get("gather_bug"), splits=how.get("splits", 1))
            caught, _, measure = _verdict(kind, dt, p, acc, pre)
            results.append((kind, caught, measure))
        # the same mistake on Gaussian data under rel-L2 <= 4e-3, what tests/test_gpu_kernels.py asks
        pg = _problem("gauss", dt, **kw)
        sp = how.get("special")
        if sp == "ldr":
            buf = R._padded(pg["residual"], 16, fill=0.0).reshape(-1)
            out = _emulate(pg, residual=buf[:pg["M"] * pg["N"]].reshape(pg["M"], pg["N"])).to(dt)
        elif sp == "c1":
            a = pg["a"]
            out = _emulate(pg, A=torch.cat([a[:, :64], torch.zeros(pg["M"], 8, dtype=F64), a[:, 64:-8]], dim=1)).to(dt)
        elif sp == "round_twice":
            out = (_emulate(pg, residual=None).to(dt).float() + pg["residual"].float()).to(dt)
        else:
            out = _emulate(pg, bug=how.get("bug"), gather_bug=how.get("gather_bug"), splits=how.get("splits", 1)).to(dt)
        value, _ = R.reference(_A(pg), pg["W"], pg["bias"], pg["rowbias"], pg["rps"], pg["residual"], pg["geglu"])
        l2 = _rel_l2(out, value)
        old = l2 <= TOL_L2
        if old:
            passed_old.append(name)
        by = next((k for k, cgt, _ in results if cgt), None)
        print(f"[mistake] {_name(dt)} {name}: caught by {by or 'NOTHING'} ({', '.join(f'{k}: {m:.3g}' for k, _, m in results)}); "
              f"old rel-L2 {l2:.2e} {'PASSES' if old else 'fails'} 4e-3")
        assert results[0][1], f"{name}: not caught by {kinds[0]}"
    print(f"[mistake] {_name(dt)}: {len(passed_old)} of {len(MISTAKES)} pass the old rel-L2 check: {passed_old}")
    assert len(passed_old) >= 3, "expectation: several seeded mistakes pass rel-L2 4e-3"


# ---- 6. the planner's answers and the coverage list -------------------------------------------------------------------------------------
def _tiles(L):
    buf = (C.c_int32 * 256)()
    n = L.gyre_debug_gemm_tiles(buf, 256)
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]


def test_planner_answers_and_coverage():
    """Every row that launches a tile kernel is put to gyre_debug_gemm_plan from its shapes alone (gemm_ref.case_shapes: no data is
    built here).  Not expressible in the query's argument struct, and therefore read off the row instead: the fused V^T rows (all of
    them forced: the launch runs the forced config or answers an error) and the k_conv_out rows, which run no tile config at all."""
    L = _lib.lib()
    tiles = _tiles(L)
    kinds = {t[0]: t[3] for t in tiles}
    assert {t[0] for t in tiles} == set(GC.FOUR_WAVE + GC.EIGHT_WAVE + (12,) + GC.PIPELINED + (GC.AR, GC.SM))
    reached, covered = set(), set()
    for r in GC.ROWS:
        if r["rc"]:
            continue
        covered.update(r["covers"])
        if r["op"] == "qkv":
            assert r["cfg"], "fused V^T rows are forced"
            reached.add(r["cfg"])
            continue
        if r["op"] == "conv_nchw" and not r["feats"]["force_tiles"]:
            continue                                 # k_conv_out: its own kernel (conv_out_supports), no tile config
        c = R.case_shapes(r)
        force = r["cfg"] | (r["splits"] << 8 if r["splits"] > 1 else 0)
        old, oab = L.gyre_debug_force_gemm_cfg(force), L.gyre_debug_gemm_ablation(r["abl"])
        if r["cfg"] == GC.AR:
            L.gyre_debug_set_ar_workspace(C.c_void_p(4096), 1 << 30)      # (never dereferenced: the query touches no device)
        a = R.gemm_test_args(c, None, 0, (4096, 1 << 40))
        if r["op"] in ("colstats_conv", "colstats_linear", "rowstats"):
            a.rows_per_sample = 0 if c.conv else r["feats"].get("rps", 1)
        try:
            rc, plan = R.plan_query(L, a)
        finally:
            L.gyre_debug_force_gemm_cfg(old), L.gyre_debug_gemm_ablation(oab), L.gyre_debug_set_ar_workspace(None, 0)
        assert rc == 0, (r["id"], rc, L.gyre_last_error())
        for k, v in r["plan"].items():
            assert plan[k] == v, f"{r['id']}: planner answers {k} = {plan[k]}, the row relies on {v} ({plan})"
        if r["cfg"]:
            assert plan["cfg"] == r["cfg"] and plan["splits"] == max(1, r["splits"])
        assert plan["cfg"] in kinds, (r["id"], plan)
        reached.add(plan["cfg"])
        fam = kinds[plan["cfg"]]
        if fam == 1:
            covered.add(f"ring depth {plan['nst']}")
            assert 2 <= plan["nst"] <= 4
        else:
            assert plan["nst"] == 0
        if c.conv and fam in (0, 1):
            tap = "uniform tap" if plan["uni"] else "non-uniform tap"
            assert tap in r["covers"] or not any("tap" in cv for cv in r["covers"]), (r["id"], plan)
            covered.add(tap)
        else:
            assert plan["uni"] == 0
        assert ("shortcut fold" in r["covers"]) == bool(plan["shortcut_fold"]), (r["id"], plan)
        if "blocked weights" in r["covers"]:
            assert plan["w_block"] == 1, r["id"]
        if "split-K" in r["covers"]:
            assert plan["splits"] > 1 and plan["ws_lo"] == (plan["splits"] * c.M * c.Nw * 4) % (1 << 32), r["id"]
        if "direct epilogue" in r["covers"]:
            assert c.N % 8 or r["feats"].get("out_off"), r["id"]
    missing_tiles = {t[0] for t in tiles} - reached
    missing = set(GC.COVERAGE) - covered
    print(f"[coverage] tile configs reached: {sorted(reached)}; features: {sorted(covered)}")
    assert not missing_tiles, f"tile configs no row reaches: {missing_tiles}"
    assert not missing, f"features no row covers: {missing}"


def test_plan_query_rejects_bad_arguments_and_matches_the_launch_problem():
    L = _lib.lib()
    out = (C.c_int32 * 12)()
    a = _lib.GemmTestArgs()
    a.M, a.K, a.N = 64, 64, 64
    assert L.gyre_debug_gemm_plan(C.byref(a), out) == 0 and out[0] in (1, 2, 3, 32)      # no pointers needed
    assert L.gyre_debug_gemm_plan(C.byref(a), None) == -1 and L.gyre_debug_gemm_plan(None, out) == -1
    for kw in (dict(M=0), dict(K=12), dict(N=-1), dict(conv=3), dict(lda=8), dict(rows_per_sample=7), dict(out_mode=5)):
        b = _lib.GemmTestArgs()
        b.M, b.K, b.N = 64, 64, 64
        for k, v in kw.items():
            setattr(b, k, v)
        assert L.gyre_debug_gemm_plan(C.byref(b), out) == -1, kw
    # an output pointer off its 16-byte alignment takes the fusions away (the direct epilogue): same rule as the launch
    a.M, a.K, a.N, a.out = 65536, 64, 320, 4096
    assert L.gyre_debug_gemm_plan(C.byref(a), out) == 0 and out[6] > 0
    a.out = 4096 + 8
    assert L.gyre_debug_gemm_plan(C.byref(a), out) == 0 and out[6] == 0
