"""Range-edge tests of the 16-bit storage type (-m gpu): values at 65504 and in the fp16 subnormals, where the O(1) data of the other
suites never goes.  Walks tests/range_cases.py; builders, the derivation of every exponent and the two checks are in
tests/range_ref.py, and tests/test_range_ref_host.py shows on the CPU that every row meets its conditions and that the seeded
range mistakes (a narrowing before the last add, 16-bit split-K partials, flushed subnormals, ...) fail these checks.

Every row runs its kernel twice: on the base problem and on the scaled one.  Check 1: the scaled output equals 2^k times the
base output bit for bit.  Check 2: the scaled output against float64 under the family's own bound.  One `[range]` line per row:
case, storage, exponents, excluded elements, bit differences, worst bound ratio.

Written against gpu_util.HDT: the file runs on both flavours (tests/test_gpu_f16_flavour.py re-runs it with fp16 storage).  Rows that
need headroom between the storage type and the fp32 accumulator (range_cases `only`) exist for fp16 storage only."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import attn_fwd_ref as A
import gemm_ref as GR
import lora_ref as LRF
import lyco_ref as LY
import norm_fwd_ref as N
import range_cases as RC
import range_ref as R
import temb_ref as T
import test_gpu_attn_fwd as AX
import test_gpu_gemm_exact as GX
import test_gpu_lora_native as LX
import test_gpu_lyco_native as YX
import test_gpu_norm_fwd as NX
import test_gpu_temb as EX
import test_gpu_tome_exact as TX
import tome_exact_ref as X
import test_gpu_t2i as TTX
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.modules import GyreHipUNet
from gpu_util import DEV, HDT, check_bound, randn, release_kept, repack_bias, repack_conv, repack_linear, st, vp

pytestmark = pytest.mark.gpu
SN = R.NAME[HDT]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ids(family):
    return [r["id"] for r in R.rows_for(RC.ROWS, HDT) if r["family"] in family]


# ---- GEMM / convolution ----------------------------------------------------------------------------------------------------------------
def _weights(row, c):
    """The weight operand on the device.  sub_w rows take it through the repack kernels from fp32 (gyre_op_repack_linear_weight,
    plain and GEGLU-interleaved; gyre_op_repack_conv_weight), which must produce exactly the 16-bit values - subnormals included."""
    direct = GX.dev(c.w)
    if row["prop"] != "sub_w":
        return direct
    W = R.operands(c)[1].float()                        # reference row order, fp32 source (every value is an fp32 normal)
    if c.conv:
        Cin = c.a_shape[-1]
        oihw = W.reshape(c.Nw, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
        if row["base"]["abl"]:
            # gyre_op_repack_conv_weight_scaled: source x 16 with scale 1 / 16 - the product is formed in fp32 and rounded once
            packed = torch.zeros(c.Nw * 9 * Cin, dtype=HDT, device=DEV)
            _lib.check(_lib.lib().gyre_op_repack_conv_weight_scaled(st(), vp((oihw * 16.0).to(DEV)), 0, c.Nw, Cin, 3, 3, Cin, 0.0625, vp(packed)))
        else:
            packed = repack_conv(oihw, Cin)
    else:
        packed = repack_linear(W, geglu=c.geglu)
    torch.cuda.synchronize()
    # by value: subnormals must be kept exactly; a -0 weight may come back as +0 (v * scale contracts into an fma with +0)
    assert torch.equal(packed.float().cpu(), direct.reshape(-1).float().cpu()), \
        f"{row['id']}: the repack kernel does not store the 16-bit value of its fp32 source"
    return packed


def _bias(row, c):
    if c.bias is None:
        return None
    if row["prop"] != "sub_w":
        return GX.dev(c.bias, torch.float32)
    ref_bias = R.operands(c)[2].float()
    packed = repack_bias(ref_bias, geglu=c.geglu)
    torch.cuda.synchronize()
    assert torch.equal(packed.cpu(), c.bias.float()), f"{row['id']}: gyre_op_repack_bias changed an fp32 bias"
    return packed


def launch_gemm(row, c):
    """One launch of a gemm / conv row's entry point on Case c under the row's forced config; the stored output in the layout of
    c.value (float32 on the host).  Sentinels around the output are checked as in tests/test_gpu_gemm_exact.py."""
    L = _lib.lib()
    b = row["base"]
    f, s = b["feats"], b["shape"]
    op = row["op"]
    w, bias = _weights(row, c), _bias(row, c)
    if op == "qkv":
        Cc, tok, ldt = c.K, f["tokens"], f["ldt"]
        B = c.M // tok
        fq, qk = GX.canary_buffer(c.M, 2 * Cc)
        fv, vt = GX.canary_buffer(B * Cc, ldt)
        vp(fq), vp(fv)
        with GX.Forced(b, c):
            _lib.check(L.gyre_op_qkv(st(), vp(GX.dev(c.a1)), c.M, Cc, vp(w), tok, C.c_void_p(qk.data_ptr()), C.c_void_p(vt.data_ptr()), ldt))
        GX.assert_canaries(row["id"] + " Q|K", fq, qk, c.M, 2 * Cc)
        GX.assert_canaries(row["id"] + " V^T", fv, vt, B * Cc, tok)
        v = vt[:B * Cc, :tok].float().cpu().reshape(B, Cc, tok).permute(0, 2, 1).reshape(c.M, Cc)
        return torch.cat([qk[:c.M].float().cpu(), v], dim=1)
    if op == "shortcut":
        C1, C2 = f["C1s"], f["C2s"]
        flat, y = GX.canary_buffer(c.M, c.N)
        ws = torch.empty(c.N * c.Ktot * 2 + c.N * 4 + 1024, dtype=torch.uint8, device=DEV)
        vp(flat)
        with GX.Forced(b, c):
            _lib.check(L.gyre_op_conv3x3_shortcut(st(), vp(GX.dev(c.a1)), s["B"], s["H"], s["W"], s["Cin"], vp(w), c.N, vp(bias),
                                                  vp(GX.dev(c.sc[:, :C1])), C1, vp(GX.dev(c.sc[:, C1:])) if C2 else None, C2, vp(GX.dev(c.w_sc)),
                                                  vp(GX.dev(c.bias_sc, torch.float32)), vp(ws), ws.numel(), C.c_void_p(y.data_ptr())))
        GX.assert_canaries(row["id"], flat, y, c.M, c.N)
        return y[:c.M].float().cpu()
    if op == "conv_nchw":
        odt = R.NCHW_DT[f["dtype"]]
        B, H, W = s["B"], s["H"], s["W"]
        flat, out = GX.canary_buffer(B * c.N, H * W, dt=odt)
        vp(flat)
        with GX.Forced(b, c):
            _lib.check(L.gyre_op_conv3x3_nchw(st(), vp(GX.dev(c.a1)), B, H, W, s["Cin"], vp(w), c.N, vp(bias), C.c_void_p(out.data_ptr()),
                                              f["dtype"], f["force_tiles"]))
        GX.assert_canaries(row["id"], flat, out, B * c.N, H * W)
        return out[:B * c.N].reshape(B, c.N, H * W).permute(0, 2, 1).reshape(c.M, c.N).float().cpu()
    ptr = dict(a1=GX.dev(c.a1), a2=None, w=w, bias=bias, rowbias=GX.dev(c.rowbias, torch.float32), residual=GX.dev(c.residual))
    addr = {k: (vp(v).value if v is not None else 0) for k, v in ptr.items()}
    if op == "linear_t":
        B = c.M // f["tokens"]
        flat, out = GX.canary_buffer(B * c.N, f["ldt"])
        rows, cols = B * c.N, f["tokens"]
    else:
        flat, out = GX.canary_buffer(c.M, c.ldc)
        rows, cols = c.M, c.N
    vp(flat)
    with GX.Forced(b, c) as fz:
        a = GR.gemm_test_args(c, addr, out.data_ptr(), (vp(fz.ws).value, fz.ws.numel()))
        prc, plan = GR.plan_query(L, a)
        assert prc == 0 and (b["splits"] <= 1 or plan["splits"] == b["splits"]) and (not b["cfg"] or plan["cfg"] == b["cfg"]), (prc, plan)
        _lib.check(L.gyre_op_gemm_test(st(), C.byref(a)))
    GX.assert_canaries(row["id"], flat, out, rows, cols)
    got = out[:rows, :cols].float().cpu()
    if op == "linear_t":
        got = got.reshape(B, c.N, cols).permute(0, 2, 1).reshape(c.M, c.N)
    return got


def launch_stats(row, c):
    """The fused-statistics entry points as tests/test_gpu_gemm_exact.py calls them: (y [M][N], statistics in the layout of
    range_ref.stats_of, float64)."""
    L = _lib.lib()
    b = row["base"]
    s, f = b["shape"], b["feats"]
    flat, y = GX.canary_buffer(c.M, c.N)
    vp(flat)
    want_shape = R.stats_of(row, c).shape
    n = 1
    for d in want_shape:
        n *= d
    bias, res = GX.dev(c.bias, torch.float32), GX.dev(c.residual)
    with GX.Forced(b, c) as fz:
        if row["op"] == "rowstats":
            assert L.gyre_op_linear_rowstats_parts(c.M, c.K, c.N, 1 if c.residual is not None else 0) == b["plan"]["rowstat_parts"]
            stats = torch.full((n + 64,), GR.CANARY, dtype=torch.float32, device=DEV)
            _lib.check(L.gyre_op_linear_rowstats(st(), vp(GX.dev(c.a1)), c.M, c.K, vp(GX.dev(c.w)), c.N, vp(bias), vp(res),
                                                 C.c_void_p(y.data_ptr()), vp(stats)))
        else:
            unit = f["unit"]
            stats = torch.full((c.M // 16 * (c.N // unit) * 2 + 64,), GR.CANARY, dtype=torch.float32, device=DEV)
            rows = C.c_int(0)
            if row["op"] == "colstats_conv":
                rc = L.gyre_op_conv3x3_colstats(st(), vp(GX.dev(c.a1)), s["B"], s["H"], s["W"], s["Cin"], vp(GX.dev(c.w)), c.N, vp(bias), vp(res),
                                                1, 0, unit, C.c_void_p(y.data_ptr()), vp(stats), stats.numel() * 4 - 256, vp(fz.ws),
                                                fz.ws.numel(), C.byref(rows))
            else:
                rc = L.gyre_op_linear_colstats(st(), vp(GX.dev(c.a1)), c.M, c.K, vp(GX.dev(c.w)), c.N, vp(bias), vp(res), f["rps"], unit,
                                               C.c_void_p(y.data_ptr()), vp(stats), stats.numel() * 4 - 256, vp(fz.ws), fz.ws.numel(),
                                               C.byref(rows))
            _lib.check(rc)
            assert rows.value == b["plan"]["colstat_rows"], (rows.value, b["plan"])
    GX.assert_canaries(row["id"], flat, y, c.M, c.N)
    assert bool((stats[n:].cpu() == GR.CANARY).all()), "statistics written past their block"
    return y[:c.M].float().cpu(), stats[:n].double().cpu().reshape(want_shape)


@pytest.mark.parametrize("rid", ids(("gemm", "conv")))
def test_gemm_range_row(rid):
    row = RC.BY_ID[rid]
    c0 = R.gemm_base(row, HDT)
    exps = RC.EXPS[rid][SN]
    c1 = R.gemm_scaled(row, c0, exps)
    if row["op"] in R.STAT_OPS:
        (got0, st0), (got1, st1) = launch_stats(row, c0), launch_stats(row, c1)
        release_kept()
        # the statistics of the stored outputs: sums x 2^k, sums of squares x 4^k, and equal to the float64 ones (exact on the lattice)
        scale = torch.tensor([2.0 ** c1.k, 4.0 ** c1.k], dtype=torch.float64)
        want = R.stats_of(row, c1)
        assert float(want[..., 1].max()) / 4.0 ** c1.k < 2.0 ** 24
        diff = int((st1 != st0 * scale).sum()) + int((st1 != want).sum())
        print(f"[range] {rid} statistics: storage {SN} exponents {tuple(exps)} excluded 0 bit differences {diff} worst ratio {0.0 if not diff else float('inf'):.3g}")
        assert diff == 0, f"{rid}: {diff} fused statistics differ from the scaled base run / the float64 sums"
    else:
        got0 = launch_gemm(row, c0)
        got1 = launch_gemm(row, c1)
        release_kept()
    R.judge_gemm(row, c0, c1, got0, got1, HDT)


# ---- GroupNorm / LayerNorm: the output does not move when x -> 2^k x and eps -> 4^k eps ------------------------------------------------
def _fold(x, G_, gamma, beta, eps, W_, bias_t, producer, unit, width):
    """gyre_op_gn_fold as tests/test_gpu_norm_fwd.py::test_gn_fold_weights_and_bias calls it: (folded weights [B, N, C], bias [B, N])."""
    L = _lib.lib()
    B, HW, Cc = x.shape
    N = W_.shape[0]
    nan = float("nan")
    wf = torch.full((B * N * Cc + 64,), nan, dtype=HDT, device=DEV)
    bf = torch.full((B * N + 64,), nan, dtype=torch.float32, device=DEV)
    wsb = L.gyre_op_groupnorm_workspace(B, HW, Cc, G_)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    cs, chunks = None, 0
    if producer:
        cs, chunks = NX._colstats(x, width, unit).to(DEV), HW // width
    rc = L.gyre_op_gn_fold(st(), vp(NX.dev16(x)), B, HW, Cc, G_, vp(gamma.to(DEV)), vp(beta.to(DEV)), eps, vp(NX.dev16(W_)),
                           vp(bias_t.to(DEV)), N, vp(cs) if producer else None, chunks, unit if producer else 0, vp(ws), wsb, vp(wf), vp(bf))
    release_kept()
    assert rc == 0, rc
    assert bool(torch.isnan(wf[B * N * Cc:]).all()) and bool(torch.isnan(bf[B * N:]).all()), "the fold wrote behind its outputs"
    return wf[:B * N * Cc].float().cpu().reshape(B, N, Cc), bf[:B * N].cpu().reshape(B, N)


@pytest.mark.parametrize("rid", ids(("norm",)))
def test_norm_range_row(rid):
    row = RC.BY_ID[rid]
    s, op = row["shape"], row["op"]
    x, gamma, beta = R.norm_inputs(row, HDT)
    (k,) = exps = RC.EXPS[rid][SN]
    x1 = x * 2.0 ** k
    eps0, eps1 = R.eps_scaled(0), R.eps_scaled(k)
    if op == "layernorm":
        got0, got1 = NX.run_ln(x, gamma, beta, eps0), NX.run_ln(x1, gamma, beta, eps1)
        ref, bound, tiny = N.ln_ref(x1, gamma, beta, eps1)
        ratio = check_bound(f"<k_layernorm> {rid}", got1, ref, bound, k=N.k_of(HDT), tiny=tiny, dims=("row", "channel"), enforce=False)
        R.judge_scaling(rid, HDT, exps, got0, got1, 0, ref, ref, ratio, exclude=False)
        return
    if op == "ln_linear":
        L = _lib.lib()
        M, K, n, geglu = s["M"], s["C"], row["N"], row["geglu"]
        assert L.gyre_debug_ln_linear_folds(M, K, n, geglu), "the planner no longer folds this shape: the row must move"
        W_, bias = R.ln_linear_weights(row, HDT)
        wd, bd = repack_linear(W_, geglu=bool(geglu)), repack_bias(bias, geglu=bool(geglu))
        ws = torch.empty(L.gyre_op_ln_linear_workspace(W_.shape[0], K, M), dtype=torch.uint8, device=DEV)
        got = []
        nparts = row.get("parts", 0)
        for t, eps in ((x, eps0), (x1, eps1)):
            y = torch.full((M, n), float("nan"), dtype=HDT, device=DEV)
            parts = R.row_parts(t).to(DEV) if nparts else None
            rc = L.gyre_op_ln_linear(st(), vp(NX.dev16(t)), M, K, vp(gamma.to(DEV)), vp(beta.to(DEV)), eps, vp(wd), n, vp(bd), geglu, 0, None, 0,
                                     vp(parts), nparts, vp(ws), ws.numel(), vp(y))
            release_kept()
            assert rc == 0, rc
            got.append(y.float().cpu())
        ref, bound, tiny = R.ln_linear_ref(row, x1, gamma, beta, eps1, W_, bias, HDT)
        ratio = check_bound(f"<ln_linear> {rid}", got[1], ref, bound, k=N.k_ln_linear(HDT), tiny=tiny, dims=("row", "column"), enforce=False)
        u = 2.0 ** -8 if HDT == torch.bfloat16 else 2.0 ** -11
        R.judge_scaling(rid, HDT, exps, got[0], got[1], 0, ref, ref, ratio, exclude=False, last_bit=R.mfma_subnormal_row(row, HDT),
                        allow=N.k_of(HDT) * u * bound + tiny)        # the fp32 part of the bound (the weights' rounding is the same in both runs)
        return
    HW, Cc, C1, G_ = s["H"] * s["W"], s["C"], s["C1"], s["G"]
    if op == "gn_fold":
        W_, bias_t = R.fold_weights(row, HDT)
        wf0, bf0 = _fold(x, G_, gamma, beta, eps0, W_, bias_t, row["producer"], row["unit"], s["W"])
        wf1, bf1 = _fold(x1, G_, gamma, beta, eps1, W_, bias_t, row["producer"], row["unit"], s["W"])
        r0 = N.fold_ref(x, G_, gamma, beta, eps0, W_, bias_t)
        wf_ref, wf_tiny, bf_ref, bf_tol = N.fold_ref(x1, G_, gamma, beta, eps1, W_, bias_t)
        ratio = check_bound(f"<fold> {rid} weights", wf1, wf_ref, wf_ref.abs(), k=N.k_of(HDT), tiny=wf_tiny, dims=("sample", "row", "channel"),
                            enforce=False)
        ratio = max(ratio, N.check_abs(f"<fold> {rid} bias", bf1, bf_ref, bf_tol, enforce=False))
        assert torch.equal(bf1, bf0), f"{rid}: the folded bias beta - mean rstd gamma does not depend on the scale of x"
        R.judge_scaling(rid, HDT, exps, wf0, wf1, -k, r0[0], wf_ref, ratio)
        return
    silu = row["silu"]
    cs0 = cs1 = None
    if op == "groupnorm_colstats":
        unit, (ra, rb) = row["unit"], row["rows"]
        mk = lambda t: (NX._colstats(t[..., :C1], ra, unit), HW // ra, NX._colstats(t[..., C1:], rb, unit), HW // rb, unit)
        cs0, cs1 = mk(x), mk(x1)
    got0 = NX.run_gn(x, C1, G_, gamma, beta, eps0, silu, cs=cs0)
    got1 = NX.run_gn(x1, C1, G_, gamma, beta, eps1, silu, cs=cs1)
    one_pass = cs0 is not None or not NX.expects_small(HW, Cc, C1 if C1 else Cc, G_)
    path = "producer-statistics" if cs0 is not None else NX.path_of(HW, Cc, C1 if C1 else Cc, G_)
    ratio = N.gn_check(f"<{path}> {rid}", got1, x1, G_, gamma, beta, eps1, silu, one_pass, HDT, enforce=False)
    R.judge_scaling(rid, HDT, exps, got0, got1, 0, got0, got0, ratio, exclude=False)


@pytest.mark.skipif(NX.SEPARATE, reason="already inside the separate-finalize run")
def test_groupnorm_rows_pass_with_the_separate_finalize_kernels():
    """k_gn_finalize + k_gn_apply (GYRE_GN_SEPARATE_FINALIZE, as tests/test_gpu_norm_fwd.py runs its plain cases) on the plain GroupNorm
    rows of this family, in a child process of the same build."""
    env = dict(os.environ, GYRE_GN_SEPARATE_FINALIZE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_range.py", "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "test_norm_range_row and (gn-up or gn-down)"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("[range]")]
    print("\n".join(l.replace("[range]", "[range] <separate-finalize>") for l in lines))
    tail = "\n".join(l for l in r.stdout.splitlines() if l.startswith(("E ", "FAILED", "[range]")) or "passed" in l or "failed" in l)[-3000:]
    assert r.returncode == 0 and len(lines) == 12, f"separate finalize failed:\n{tail}\n{r.stderr[-2000:]}"


# ---- attention forward: V at the top, V and the output in the subnormals ------------------------------------------------------------------
@pytest.mark.parametrize("rid", ids(("attn",)))
def test_attention_range_row(rid):
    row = RC.BY_ID[rid]
    q, k, v, heads, presc, variant, vpad = R.attn_inputs(row, HDT)
    (kk,) = exps = RC.EXPS[rid][SN]
    v1 = v * 2.0 ** kk
    rc0, got0, _ = AX.run_fwd(q, k, v, heads, presc, variant, vpad=vpad)
    rc1, got1, _ = AX.run_fwd(q, k, v1, heads, presc, variant, vpad=vpad)
    _lib.check(rc0), _lib.check(rc1)
    ref0, ref1 = A.fwd_ref(q, k, v, heads, presc), A.fwd_ref(q, k, v1, heads, presc)
    ratio = check_bound(rid, got1, ref1[0], ref1[1], k=A.K_FWD, tiny=A.fwd_tiny(v1, HDT), dims=AX.DIMS, enforce=False)
    down = row["end"] == "down"
    R.judge_scaling(rid, HDT, exps, got0, got1, kk, ref0[0], ref1[0], ratio, exclude=not down, exact=GR.rne(ref1[0], HDT) if down else None)


def test_fused_cross_attention_block_scales_with_x_v_and_bias():
    """x -> 2^k x (eps -> 4^k eps), V -> 2^k V, bo -> 2^k bo: q does not move, the attention output - re-packed inside the kernel as the
    operand of the output projection - and the stored result scale by 2^k.  Check 2 is the block's existing yardstick: its operator
    chain gyre_op_ln_linear -> gyre_op_attention_ex -> gyre_op_linear on the scaled operands, K_XATTN (tests/test_gpu_attn_fwd.py)."""
    rid = "xattn-block-top-Nk77"
    row = RC.BY_ID[rid]
    assert SN in row["only"]
    L = _lib.lib()
    s = row["shape"]
    B, tokens, C_, heads, Nk = s["B"], s["tokens"], s["C"], s["heads"], s["Nk"]
    D, M = C_ // heads, B * tokens
    x, g, be, wq, k, v, wo, bo = R.xattn_inputs(row, HDT)
    (kk,) = exps = RC.EXPS[rid][SN]
    wqd, wod, gd, bed, kd = repack_linear(wq), repack_linear(wo), g.to(DEV), be.to(DEV), k.to(HDT).to(DEV)
    ws = torch.empty(L.gyre_op_ln_linear_workspace(C_, C_, M), dtype=torch.uint8, device=DEV)
    ldvt = (Nk + 7) // 8 * 8
    out = {}
    for name, e in (("base", 0), ("scaled", kk)):
        xd, bod, eps = (x * 2.0 ** e).to(HDT).to(DEV), (bo * 2.0 ** e).to(DEV), R.eps_scaled(e)
        vt = torch.full((B, C_, ldvt), float("nan"), dtype=HDT, device=DEV)
        vt[:, :, :Nk] = (v * 2.0 ** e).permute(0, 2, 1).to(HDT).to(DEV)
        fused = torch.empty(M, C_, dtype=HDT, device=DEV)
        _lib.check(L.gyre_op_cross_attention_block(st(), vp(xd), M, tokens, C_, heads, vp(gd), vp(bed), eps, vp(wqd), vp(kd), vp(vt), Nk, ldvt,
                                                   vp(wod), vp(bod), vp(ws), ws.numel(), vp(fused), None))
        out[name] = fused.float().cpu()
        if name == "scaled":
            qd, ad, chain = (torch.empty(M, C_, dtype=HDT, device=DEV) for _ in range(3))
            _lib.check(L.gyre_op_ln_linear(st(), vp(xd), M, C_, vp(gd), vp(bed), eps, vp(wqd), C_, None, 0, 0, None, 0, None, 0, vp(ws),
                                           ws.numel(), vp(qd)))
            _lib.check(L.gyre_op_attention_ex(st(), vp(qd), C_, vp(kd), C_, vp(vt), ldvt, B, heads, tokens, Nk, D, vp(ad), C_, 1))
            _lib.check(L.gyre_op_linear(st(), vp(ad), M, C_, vp(wod), C_, vp(bod), vp(xd), 0, vp(chain)))
            a = ad.float().cpu().double()
            bound = (x.double() * 2.0 ** e).abs() + (bo.double() * 2.0 ** e).abs() + a.abs() @ wo.double().abs().t()
            ratio = check_bound(rid, out[name], chain.float().cpu(), bound, k=AX.K_XATTN, dims=("row", "channel"), enforce=False)
        release_kept()
    ref0 = R.xattn_ref(row, (x, g, be, wq, k, v, wo, bo))[0]
    R.judge_scaling(rid, HDT, exps, out["base"], out["scaled"], kk, ref0, ref0 * 2.0 ** kk, ratio)


# ---- token merging: three tokens near top / 2 into one row ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ids(("tome",)))
def test_tome_range_row(rid):
    row = RC.BY_ID[rid]
    keys, v, r = R.tome_inputs(row, HDT)
    (kk,) = exps = RC.EXPS[rid][SN]
    v1 = v * 2.0 ** kk
    order, node_idx, _, reff = X.select64(keys, r)
    u = 2.0 ** -8 if HDT == torch.bfloat16 else 2.0 ** -11
    if row["op"] == "tome_unmerge":
        L = _lib.lib()
        B, Nn, Cc = v.shape
        out = TX._merge(keys, keys, r)
        dl = X.dstlist_of(order, node_idx, reff)
        assert torch.equal(out["order"], order) and torch.equal(out["dstlist"][:, :reff], dl)
        dy = v[:, :Nn - reff]
        got = []
        for d in (dy, dy * 2.0 ** kk):
            dxb = torch.full((B, Nn, 3 * Cc), TX.SENTINEL, dtype=HDT, device=DEV)
            inv = torch.full((B, Nn // 2), -1, dtype=torch.int32, device=DEV)
            _lib.check(L.gyre_op_tome_unmerge(st(), vp(d.to(HDT).to(DEV)), B, Nn, Cc, reff, vp(out["dev"]["order"]), vp(out["dev"]["dstlist"]),
                                              vp(inv), vp(dxb.view(-1)[Cc:]), 3 * Cc))
            release_kept()
            got.append(dxb.cpu()[:, :, Cc:2 * Cc].float())
        ref0, _, _ = X.unmerge64(dy, order, dl, reff, Nn)
        ref1, _, src1 = X.unmerge64(dy * 2.0 ** kk, order, dl, reff, Nn)
        ratio = float(((got[1].double() - ref1).abs() / X.unmerge_tolerance(ref1, src1, u)).nan_to_num(nan=float("inf")).max())
        R.judge_scaling(rid, HDT, exps, got[0], got[1], kk, ref0, ref1, ratio)
        return
    out0, out1 = TX._merge(keys, v, r), TX._merge(keys, v1, r)
    for o in (out0, out1):
        assert torch.equal(o["order"], order) and torch.equal(o["node_idx"], node_idx), "lattice keys: the selection is the float64 one"
    nout = out0["nout"]
    both = lambda o: torch.cat([o["vrows"].float(), o["vt_out"][:, :, :nout].transpose(1, 2).float()])
    ref0, cnt, _ = X.merge_wavg64(v, order, node_idx, reff)
    ref1, _, absmean1 = X.merge_wavg64(v1, order, node_idx, reff)
    tol = X.merge_tolerance(ref1, cnt, absmean1, u)
    got0, got1 = both(out0), both(out1)
    ratio = float(((got1.double() - torch.cat([ref1, ref1])).abs() / torch.cat([tol, tol])).nan_to_num(nan=float("inf")).max())
    R.judge_scaling(rid, HDT, exps, got0, got1, kk, torch.cat([ref0, ref0]), torch.cat([ref1, ref1]), ratio)


# ---- boundary and element-wise kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ids(("elem",)))
def test_elementwise_range_row(rid):
    L = _lib.lib()
    row = RC.BY_ID[rid]
    op = row["op"]
    exps = RC.EXPS[rid][SN]
    if op == "nchw_to_nhwc":
        x = R.cast_image(row["src"], (2, 9, 240))
        xd = x.to(DEV)
        y = torch.full((2, 240, 16), 7.0, dtype=HDT, device=DEV)
        _lib.check(L.gyre_op_nchw_to_nhwc(st(), vp(xd), _lib.dtype_code(xd), 2, 9, 240, 16, vp(y)))
        release_kept()
        want = torch.zeros(2, 240, 16, dtype=HDT)                        # padding channels are zero
        want[:, :, :9] = x.to(HDT).permute(0, 2, 1)
        diff = R.same_bits(y, want)
    elif op == "pixel_unshuffle8":
        B, c, H, W = 2, 2, 16, 24
        x = R.cast_image(row["src"], (B, c, H, W))
        xd = x.to(DEV)
        y = torch.zeros((B, H // 8, W // 8, 64 * c), dtype=HDT, device=DEV)
        _lib.check(L.gyre_op_pixel_unshuffle8(st(), vp(xd), _lib.dtype_code(xd), B, c, H, W, vp(y)))
        release_kept()
        xs = x.to(HDT)
        want = xs.reshape(B, c, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(B, H // 8, W // 8, 64 * c)      # F.pixel_unshuffle, NHWC
        diff = R.same_bits(y, want)
    elif op == "relu":
        x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(HDT)       # every bit pattern of the storage type
        xd = x.to(DEV)
        want = torch.relu(x.to(DEV)).cpu()
        _lib.check(L.gyre_op_relu(st(), vp(xd), xd.numel()))
        release_kept()
        diff = R.same_bits(xd, want)
    elif op == "t2i_copy":
        # the feature maps of the tiny adapter at three image scales, copied out as f32 (exact: every 16-bit value is an fp32 value),
        # bf16 and f16: the 16-bit copies must be torch's cast of the f32 copy - inf where an fp16 output cannot hold a bf16 feature
        cfg = gcfg.tiny_t2i("main")
        net, _ = TTX.make(cfg, HDT)
        net(torch.rand((2, 3, 64, 96)).to(DEV))                             # uploads the weights, creates the handle
        h = C.c_void_p(net._handle)
        need = L.gyre_t2i_workspace_bytes(h, 2, 64, 96)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
        diff = 0
        for e in ((0, 6, -12) if HDT == torch.float16 else (0, 18, -40)):
            img = (torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(8)) * 2.0 ** e).to(DEV)
            shapes = [tuple(t.shape) for t in net(img)]
            outs = {}
            for code, dt in ((0, torch.float32), (1, torch.bfloat16), (2, torch.float16)):
                outs[dt] = [torch.full(sh, 7.0, dtype=dt, device=DEV) for sh in shapes]
                arr = (C.c_void_p * 4)(*[o.data_ptr() for o in outs[dt]])
                _lib.check(L.gyre_t2i_forward(h, st(), vp(img), 0, 2, 64, 96, C.c_void_p((ws.data_ptr() + 255) & ~255), need, arr, 4, code))
                torch.cuda.synchronize()
            for f32, b16, h16 in zip(outs[torch.float32], outs[torch.bfloat16], outs[torch.float16]):
                f = f32.cpu()
                assert torch.equal(f.to(HDT).float(), f) or bool(torch.isnan(f).any()), "the f32 copy holds storage values"
                diff += R.same_bits(b16, f.to(torch.bfloat16)) + R.same_bits(h16, f.to(torch.float16))
            print(f"[range] {rid}: image x 2^{e}: largest feature {max(float(o.abs().max()) for o in outs[torch.float32]):.4g}")
        release_kept()
    elif op == "residual_add":
        cfg = gcfg.tiny_unet()
        sd = weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 0)
        net = GyreHipUNet(cfg)
        net.load_state_dict(sd)
        net = net.to(HDT).to(DEV)
        x, t = randn(2, 4, 16, 16, seed=1).to(DEV), torch.tensor([901, 77]).to(DEV)
        ctx = randn(2, 77, cfg.cross_attention_dim, seed=2).to(DEV)
        # one adapter state per down level (shapes by the rule of GyreHipUNet.forward); the LAST level adds its state at its end, right in
        # front of the "down<last>" tap, so the tap reads the sum itself
        boc, last = cfg.block_out_channels, len(cfg.block_out_channels) - 1
        shapes, ah = [], 16
        for i in range(last + 1):
            nh = ah if i == last else (ah + 1) // 2
            shapes.append((2, boc[i], ah, ah) if (cfg.attn_levels[i] or i == last) else (2, boc[i], nh, nh))
            ah = nh
        tap = f"down{last}".encode()
        sdt = R.SRC_DT[row["src"]]

        def tap_last(state0):
            states = [torch.zeros(sh, dtype=sdt, device=DEV) for sh in shapes[:-1]] + [state0.to(DEV)]
            buf = torch.empty(shapes[-1], dtype=torch.float32, device=DEV)
            if not hasattr(net, "_handle") or not net._handle:
                net(x, t, encoder_hidden_states=ctx)                    # uploads the weights, creates the handle
            _lib.check(L.gyre_unet_debug_tap(C.c_void_p(net._handle), tap, C.c_void_p(buf.data_ptr()), buf.numel() * 4))
            net(x, t, encoder_hidden_states=ctx, adapter_states=states)
            torch.cuda.synchronize()
            return buf.cpu()
        skip = tap_last(torch.zeros(shapes[-1], dtype=sdt))
        assert torch.equal(skip.to(HDT).float(), skip) and float(skip.abs().max()) > 0
        diff = 0
        for r in (R.cast_image(row["src"], shapes[-1], seed=3), R.residual_targets(skip, row["src"])):
            got = tap_last(r)
            diff += R.same_bits(got.to(HDT), R.residual_expected(skip, r, HDT))
    else:
        assert op == "avgpool2"
        x = R.avgpool_inputs(row, HDT)
        (kk,) = exps
        got = []
        for t in (x, x * 2.0 ** kk):
            B, H, W, Cn = t.shape
            y = torch.zeros((B, H // 2, W // 2, Cn), dtype=HDT, device=DEV)
            _lib.check(L.gyre_op_avgpool2(st(), vp(t.to(HDT).to(DEV)), B, H, W, Cn, vp(y)))
            release_kept()
            got.append(y.float().cpu())
        ref0, _ = R.avgpool_ref(x)
        ref1, mabs1 = R.avgpool_ref(x * 2.0 ** kk)
        ratio = float(((got[1].double() - ref1).abs() / R.avgpool_tolerance(ref1, mabs1, HDT)).nan_to_num(nan=float("inf")).max())
        sub = row["prop"] == "sub_out"
        R.judge_scaling(rid, HDT, exps, got[0], got[1], kk, ref0, ref1, ratio, exclude=not sub, exact=GR.rne(ref1, HDT) if sub else None)
        return
    R.report(rid, HDT, exps, 0, diff, 0.0)
    assert diff == 0, f"{rid}: {diff} elements differ from torch's cast bit for bit"


# ---- time-embedding path: subnormal 16-bit weights against fp32 activations --------------------------------------------------------------------
@pytest.mark.parametrize("rid", ids(("temb",)))
def test_temb_range_row(rid):
    row = RC.BY_ID[rid]
    s = row["shape"]
    x, W, bias = R.temb_inputs(row, HDT)
    (kk,) = exps = RC.EXPS[rid][SN]
    W1, bias1 = W * 2.0 ** kk, bias * 2.0 ** kk
    dev16 = lambda t: t.to(HDT).to(DEV)
    if row["op"] == "rowvec_linear":
        got0, _ = EX._linear(x, dev16(W), bias.to(DEV), s["N"], False)
        got1, _ = EX._linear(x, dev16(W1), bias1.to(DEV), s["N"], False)
        ref0, _ = T.linear64(x, W, bias, False)
        ref1, bound1 = T.linear64(x, W1, bias1, False)
    else:
        t = T.timesteps(s["B"], 2)
        got0 = EX._timestep_linear(t, s["K"], 1, 0.0, dev16(W), bias.to(DEV), s["N"])
        got1 = EX._timestep_linear(t, s["K"], 1, 0.0, dev16(W1), bias1.to(DEV), s["N"])
        e64, a = T.embedding64(t, s["K"], 1, 0.0)
        ref0, _ = T.linear64(e64, W, bias, False)
        ref1, bound1 = T.linear64(e64, W1, bias1, False)
        bound1 = bound1 + (T.embedding_tolerance(a) / T.U32) @ W1.double().abs().t()
    release_kept()
    ratio = check_bound(rid, got1, ref1, bound1, k=1.0, hdt=torch.float32, dims=("row", "column"), enforce=False)
    R.judge_scaling(rid, HDT, exps, got0, got1, kk, ref0, ref1, ratio, odt=torch.float32)


# ---- LoRA / LyCORIS merge: merged weights at the top of the range and in the subnormals ------------------------------------------------------------
@pytest.mark.parametrize("rid", ids(("lora",)))
def test_lora_range_row(rid):
    import numpy as np
    row = RC.BY_ID[rid]
    (kk,) = exps = RC.EXPS[rid][SN]
    if row["op"] == "lyco_core":
        core, right = R.lyco_core_inputs(row)
        core1 = core * np.float32(2.0 ** kk)
        got0 = YX.gpu_core(core, right, torch.float16, torch.float32)
        got1 = YX.gpu_core(core1, right, torch.float16, torch.float32)
        want0, want1 = LY.core64(core, right), LY.core64(core1, right)
        tol = core.shape[1] * LY.U32 * LY.core64(np.abs(core1), np.abs(right)) * (1 + 2.0 ** -10)
        ratio = float(np.max(np.abs(got1.astype(np.float64) - want1) / tol))
        R.judge_scaling(rid, HDT, exps, torch.from_numpy(got0), torch.from_numpy(got1), kk, torch.from_numpy(want0), torch.from_numpy(want1),
                        ratio, odt=torch.float32)
        return
    case, base, terms = R.lora_inputs(row, HDT)
    name, O, I, KH, KW, I_pad, geglu, scale_p = case[:8]
    base1, terms1 = R.lora_scaled(row, base, terms, kk)
    run = LX.run_op if row["op"] == "repack_lora" else YX.run_op
    got0, got1 = run(base, terms, I_pad, geglu, scale_p), run(base1, terms1, I_pad, geglu, scale_p)
    ref0, _, _ = R.lora_ref(row, case, base, terms, HDT)
    ref1, tol1, _ = R.lora_ref(row, case, base1, terms1, HDT)
    assert not got0[..., I:].any() and not got1[..., I:].any(), "pad columns are zero"
    got0, got1 = got0[..., :I], got1[..., :I]
    r0, r1 = torch.from_numpy(ref0[..., :I].copy()), torch.from_numpy(ref1[..., :I].copy())
    ratio = LRF.worst_ratio(rid, got1, r1.numpy(), tol1[..., :I])
    lattice = row["data"] == "lattice"
    R.judge_scaling(rid, HDT, exps, got0, got1, kk, r0, r1, ratio, exclude=not lattice, exact=r1 if lattice else None)
