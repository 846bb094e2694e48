"""Range-edge tests of the image-model kernels (-m gpu): values at 65504 and in the fp16 subnormals, and +-inf / NaN among O(1) data,
for the kernels that came after tests/test_gpu_range.py - the ControlNet hand-off, the RRDB dense-block convolution and its epilogue,
the SwinIR / HAT window attention, element-wise and normalisation passes, the line-art hinter's instance normalisation and 7 x 7
convolutions, the HED tail and fuse kernels, the plain-matrix delta merge, the four-parity upsampler convolution.  Walks
tests/range_image_cases.py; builders, the derivation of every exponent, the judges and the host emulations are in
tests/range_image_ref.py, and tests/test_range_image_ref_host.py shows on the CPU that every row meets its conditions and that the
seeded mistakes (16-bit pool partials, a variance without the shift, a narrowing before the residual, flushed subnormals, a scale
folded into 16-bit q, a doubly narrowed P, a NaN dropped by a max) fail these checks.

Scaling rows run the kernel on the base problem and on the scaled one: check 1, the scaled output equals 2^k times the base output bit
for bit; check 2, the scaled output against float64 under the kernel's own bound.  Specials rows run it with and without the specials:
every element in the class torch's CPU evaluation gives, clean samples bit-identical.  One `[range]` line per row and storage.

Both storage flavours run in this process (STORAGES, as in tests/test_gpu_hat_kernels.py)."""
import ctypes as C

import pytest
import torch

import range_image_cases as IC
import range_image_ref as Q
import range_ref as R
from gyre_amd import _lib
from gpu_util import DEV

pytestmark = pytest.mark.gpu
STORAGES = [(_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)]
CODE = {torch.float32: 0, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def params(pred):
    return [pytest.param(r["id"], st, sdt, id=f"{r['id']}-{R.NAME[sdt]}") for r in IC.ROWS if pred(r) for st, sdt in STORAGES
            if R.NAME[sdt] in r["only"]]


def _st():
    return C.c_void_p(_lib.stream_ptr(torch.device(DEV)))


def _p(t):
    """the device pointer of a tensor the CALLER keeps alive"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(t, dt):
    return t.to(dt).contiguous().to(DEV)


# ---- one launch per op: P (range_image_ref problem) -> {output name: tensor on the host} ------------------------------------------------------
def run_hed_tail(lib, sdt, row, P):
    xd, wd, bd = _dev(P["x"], sdt), P["w"].to(DEV), P["b"].to(DEV)
    B, Hs, Ws, C_ = xd.shape
    po = torch.full((B, -(-Hs // 2), -(-Ws // 2), C_), float("nan"), dtype=sdt, device=DEV)
    so = torch.full((B, Hs, Ws), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_hed_tail(_st(), _p(xd), B, Hs, Ws, C_, _p(wd), _p(bd), _p(po), _p(so)), lib)
    torch.cuda.synchronize()
    return {"pool": po.cpu(), "so": so.cpu()}


def run_inorm(lib, sdt, row, P):
    """gyre_op_inorm_stats + gyre_op_inorm_apply in the row's form: plain, the pad-3 write (with the ReLU, as the graph runs it), or the
    shuffled source with a residual"""
    import lineart_ref as LA
    x = P["x"].to(sdt)
    B, H, W, C_ = x.shape
    form = P["form"]
    src = _dev(LA.shuffle_rows(x) if form == "shuffled_res" else x, sdt)
    rows = H * W
    part = torch.empty(max(1, lib.gyre_op_inorm_workspace(B, rows, C_)), dtype=torch.uint8, device=DEV)
    stats = torch.full((B, C_, 2), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.gyre_op_inorm_stats(_st(), _p(src), C_, B, rows, C_, P["eps"], _p(part), _p(stats)), lib)
    pad = 3 if form == "pad3" else 0
    out = torch.full((B, H + 2 * pad, W + 2 * pad, C_), float("nan"), dtype=sdt, device=DEV)
    res = _dev(P["res"], sdt) if "res" in P else None
    a = _lib.InormApplyArgs(x=src.data_ptr(), stats=stats.data_ptr(), res=None if res is None else res.data_ptr(), out=out.data_ptr(),
                            B=B, H=H, W=W, C=C_, shuffled=int(form == "shuffled_res"), relu=P["relu"], res_pad=0, pad=pad, patch=0)
    _lib.check(lib.gyre_op_inorm_apply(_st(), C.byref(a)), lib)
    torch.cuda.synchronize()
    s = stats.cpu()
    return {"mean": s[..., 0].contiguous(), "rstd": s[..., 1].contiguous(), "out": out.cpu()}


def run_ln_live(lib, sdt, row, P):
    M, C_ = P["x"].shape
    ld = row["ld"]
    src = torch.full((M, ld), float("nan"), dtype=sdt)               # NaN in the source padding must not leak
    src[:, :C_] = P["x"].to(sdt)
    sd, g, b = src.to(DEV), P["gamma"].float().to(DEV), P["beta"].float().to(DEV)
    y = torch.full((M, ld), float("nan"), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_ln_live(_st(), _p(sd), ld, M, C_, _p(g), _p(b), P["eps"], _p(y), ld), lib)
    torch.cuda.synchronize()
    return {"out": y.cpu()}


def _pool(lib, c2d, B, HW, C_, ld):
    need = lib.gyre_op_chan_pool_workspace(B, HW, C_)
    part = torch.full((need // 4 + 4,), float("nan"), device=DEV)
    pool = torch.full((B * C_ + 4,), float("nan"), device=DEV)
    _lib.check(lib.gyre_op_chan_pool(_st(), _p(c2d), ld, B, HW, C_, _p(part), _p(pool)), lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(pool[B * C_:]).all()) and bool(torch.isnan(part[need // 4:]).all()), "the pool wrote past its outputs"
    return pool


def run_chan_pool(lib, sdt, row, P):
    c2d = _dev(P["c2"], sdt)
    B, HW, ld = c2d.shape
    return {"pool": _pool(lib, c2d, B, HW, P["C"], ld)[:B * P["C"]].cpu().view(B, P["C"])}


def run_scale_add(lib, sdt, row, P):
    yd, c2d, sd = _dev(P["y"], sdt), _dev(P["c2"], sdt), P["s"].contiguous().to(DEV)
    B, HW, ld = yd.shape
    _lib.check(lib.gyre_op_scale_add(_st(), _p(yd), ld, _p(c2d), ld, _p(sd), ld, B, HW, ld), lib)
    torch.cuda.synchronize()
    return {"y": yd.cpu()}


def run_cab(lib, sdt, row, P):
    c2d, yd = _dev(P["c2"], sdt), _dev(P["y"], sdt)
    B, HW, ld = c2d.shape
    C_, Cs = P["C"], P["Cs"]
    pool = _pool(lib, c2d, B, HW, C_, ld)
    gate = torch.full((B, ld), float("nan"), device=DEV)
    w = {k: P[k].contiguous().to(DEV) for k in ("w1", "b1", "w2", "b2")}
    _lib.check(lib.gyre_op_chan_gate(_st(), _p(pool), B, C_, Cs, _p(w["w1"]), _p(w["b1"]), _p(w["w2"]), _p(w["b2"]), P["scale"], _p(gate), ld), lib)
    _lib.check(lib.gyre_op_scale_add(_st(), _p(yd), ld, _p(c2d), ld, _p(gate), ld, B, HW, ld), lib)
    torch.cuda.synchronize()
    return {"pool": pool[:B * C_].cpu().view(B, C_), "gate": gate.cpu(), "y": yd.cpu()}


def run_act(lib, sdt, row, P):
    x = P["x"].to(sdt)
    n = x.numel()
    buf = torch.cat([x, torch.full((8,), float("nan"), dtype=sdt)]).to(DEV)
    if row["op"] == "silu":
        _lib.check(lib.gyre_op_silu(_st(), _p(buf), n), lib)
    else:
        _lib.check(lib.gyre_op_swin_act(_st(), _p(buf), n, P["mode"], P["slope"]), lib)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool(torch.isnan(got[n:].float()).all()), "elements past n were touched"
    return {"x": got[:n]}


def run_rdb_epilogue(lib, sdt, row, P):
    d, db = _dev(P["buf"], sdt), P["bias"].to(DEV)
    live, c0, ldo = P["live"], P["c0"], P["ldo"]

    def resid(r):                                                       # [npix, live] inside a NaN buffer of stride 64
        if r is None:
            return None
        base = torch.full((r.shape[0], 64), float("nan"), dtype=sdt)
        base[:, :live] = r.to(sdt)
        return base.to(DEV)
    d1, d2 = resid(P["r1"]), resid(P["r2"])
    epi = _lib.RdbEpilogue()
    epi.bias, epi.alpha, epi.act = db.data_ptr(), P["alpha"], P["act"]
    epi.r1, epi.ldr1, epi.beta1 = d1.data_ptr(), 64, P["beta1"]
    if d2 is not None:
        epi.r2, epi.ldr2, epi.beta2 = d2.data_ptr(), 64, P["beta2"]
    _lib.check(lib.gyre_op_rdb_epilogue(_st(), _p(d), c0, ldo, live, d.shape[0], C.byref(epi)), lib)
    torch.cuda.synchronize()
    got = d.cpu()
    rest = torch.ones(ldo, dtype=torch.bool)
    rest[c0:c0 + live] = False
    assert R.same_bits(got[:, rest], P["buf"].to(sdt)[:, rest]) == 0, "bytes outside the slice changed"
    return {"slice": got[:, c0:c0 + live].contiguous()}


def run_hed_fuse(lib, sdt, row, P, odt):
    import hed_ref as HD
    H, W = P["H"], P["W"]
    B = P["so"][0].shape[0]
    sod, wfd, bfd = [s.float().contiguous().to(DEV) for s in P["so"]], P["wf"].float().to(DEV), P["bf"].float().to(DEV)
    out = torch.full((6, B, 1, H, W), float("nan"), dtype=odt, device=DEV)
    a = _lib.HedFuseArgs(wf=wfd.data_ptr(), bf=bfd.data_ptr(), out=out.data_ptr(), out_dtype=CODE[odt], B=B, H=H, W=W)
    sh, sw, oy, ox = HD.stage_sizes(H), HD.stage_sizes(W), HD.crop_offsets(H), HD.crop_offsets(W)
    for k in range(5):
        assert tuple(sod[k].shape) == (B, sh[k], sw[k])
        a.so[k], a.Hk[k], a.Wk[k], a.oy[k], a.ox[k] = sod[k].data_ptr(), sh[k], sw[k], oy[k], ox[k]
    _lib.check(lib.gyre_op_hed_fuse(_st(), C.byref(a)), lib)
    torch.cuda.synchronize()
    return {"out": out.cpu()}


def run_conv7_out(lib, sdt, row, P, odt):
    xd, wd, bd = _dev(P["xp"], sdt), _dev(P["w"], sdt), P["b"].float().to(DEV)
    B, Hp, Wp, _ = xd.shape
    H, W = Hp - 6, Wp - 6
    scratch = torch.empty(49 * 64, dtype=sdt, device=DEV)
    out = torch.full((B, 1, H, W), float("nan"), dtype=odt, device=DEV)
    _lib.check(lib.gyre_op_conv7_out(_st(), _p(xd), B, H, W, _p(wd), CODE[sdt], _p(scratch), _p(bd), P["sigmoid"], _p(out), CODE[odt]), lib)
    torch.cuda.synchronize()
    return {"out": out.cpu()}


def run_ctrl_emit(lib, sdt, row, P):
    f, out = P["f"].to(sdt), P["out"]
    B, HW, Cpad = f.shape
    fd, od = f.to(DEV), out.to(DEV)
    _lib.check(lib.gyre_op_ctrl_emit(_st(), _p(fd), B, P["C"], HW, Cpad, P["scale"], int(P["accumulate"]), _p(od), CODE[od.dtype],
                                     od.shape[0], P["b0"]), lib)
    torch.cuda.synchronize()
    return {"out": od.cpu()}


def run_attn(lib, sdt, row, P):
    """gyre_op_win_attn / gyre_op_hat_attn through the runners of their own test modules; the live columns of the output"""
    import test_gpu_hat_kernels as HX
    import test_gpu_swin_kernels as SX
    L = P["L"]
    got = (SX if row["op"] == "win_attn" else HX).run_attn(L, lib)
    n = 30 * L["heads"]
    assert R.same_bits(got[:, n:], L["o"][:, n:]) == 0, "an element outside the live columns changed"
    return {"o": got[:, :n].contiguous()}


def run_rdb_conv(lib, sdt, row, P):
    """gyre_op_rdb_conv through the runner of its own test module (weights through the kernel's own pack pass); the written slice"""
    import rrdb_ref as RB
    import test_gpu_rdb_kernels as RX
    L = P["L"]
    got = RX.run_conv(L, lib)
    assert RB.verdict(L, got)[1], "bytes outside the written slice changed"
    return {"slice": got[..., L["c0"]:L["c0"] + L["live"]].contiguous()}


def run_conv7_in(lib, sdt, row, P):
    """the NCHW image through gyre_op_nchw_to_nhwc into the 8-channel entry tensor, then gyre_op_conv7_in (weights through its own pack)"""
    x, wd, bd = P["x"].to(sdt).to(DEV), _dev(P["w"], sdt), P["b"].float().to(DEV)
    B, _, H, W = x.shape
    x8 = torch.empty((B, H, W, 8), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_nchw_to_nhwc(_st(), _p(x), CODE[sdt], B, 3, H * W, 8, _p(x8)), lib)
    scratch = torch.empty(64 * 49 * 8, dtype=sdt, device=DEV)
    out = torch.full((B, H, W, 64), float("nan"), dtype=sdt, device=DEV)
    _lib.check(lib.gyre_op_conv7_in(_st(), _p(x8), B, H, W, _p(wd), CODE[sdt], _p(scratch), _p(bd), _p(out)), lib)
    torch.cuda.synchronize()
    return {"out": out.cpu()}


def run_merge_delta(lib, sdt, row, P):
    """gyre_op_merge_delta through the runner of its own test module: an fp32 base, the output in the row's dtype"""
    import test_gpu_merge_delta as MX
    return {"out": MX.run_op(lib, P["base"], P["terms"], torch.float32, R.SRC_DT[row["out"]])}


def run_ups4(lib, sdt, row, P):
    """gyre_op_upsample_conv_test under tuning bit 30 (config 24 whatever the tile count), as tests/test_gpu_ups4_conv.py calls it, on
    the library of the row's flavour; the composed weights go through launch_compose_ups4 into the scratch on every call"""
    B, Hi, Wi, Cin = P["x"].shape
    N = P["w"].shape[0]
    M = B * 4 * Hi * Wi
    canary = -3.0
    out = torch.full((M + 4, N), canary, dtype=sdt, device=DEV)
    xd, wd, bd = _dev(P["x"], sdt), _dev(P["w"], sdt), P["bias"].float().to(DEV)
    scratch = torch.empty(16 * N * Cin + 64, dtype=sdt, device=DEV)
    ws = torch.empty(M * N + 64, dtype=torch.float32, device=DEV)
    a = _lib.UpsampleConvTestArgs()
    a.B, a.Hi, a.Wi, a.Cin, a.N, a.splits = B, Hi, Wi, Cin, N, 1
    a.x, a.w, a.bias, a.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    a.scratch, a.scratch_bytes = scratch.data_ptr(), 16 * N * Cin * scratch.element_size()
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    old = lib.gyre_debug_gemm_ablation(Q.UPS4_ALL)
    try:
        q = (C.c_int32 * 4)()
        _lib.check(lib.gyre_debug_ups4_plan(B, Hi, Wi, Cin, N, 0, 0, 0, 0, q), lib)
        assert tuple(q)[:3] == (1, 24, 1), tuple(q)
        _lib.check(lib.gyre_op_upsample_conv_test(_st(), C.byref(a)), lib)
        torch.cuda.synchronize()
    finally:
        lib.gyre_debug_gemm_ablation(old)
    assert bool((out[M:].float() == canary).all()), "rows after M were written"
    return {"out": out[:M].cpu()}


RUNNERS = {
    "hed_tail": run_hed_tail, "inorm": run_inorm, "ln_live": run_ln_live, "chan_pool": run_chan_pool, "scale_add": run_scale_add,
    "cab": run_cab, "win_attn": run_attn, "hat_attn": run_attn, "rdb_conv": run_rdb_conv, "conv7_in": run_conv7_in,
    "merge_delta": run_merge_delta, "ups4": run_ups4, "swin_act": run_act, "silu": run_act, "rdb_epilogue": run_rdb_epilogue,
    "ctrl_emit_acc": run_ctrl_emit,
}


def launch(lib, sdt, row, P):
    op = row["op"]
    if op in ("hed_fuse", "conv7_out"):
        odt = R.SRC_DT[row["out"]] if "out" in row else torch.float32
        return (run_hed_fuse if op == "hed_fuse" else run_conv7_out)(lib, sdt, row, P, odt)
    return RUNNERS[op](lib, sdt, row, P)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,storage,sdt", params(lambda r: r["family"] in Q.SCALING_FAMILIES))
def test_scaling_row(rid, storage, sdt):
    row = IC.BY_ID[rid]
    lib = _lib.lib(storage)
    exps = IC.IMAGE_EXPS[rid][R.NAME[sdt]]
    P0, P1 = Q.problems(row, sdt, exps)
    got0, got1 = launch(lib, sdt, row, P0), launch(lib, sdt, row, P1)
    Q.judge(row, sdt, exps, P0, P1, got0, got1)


@pytest.mark.parametrize("rid,storage,sdt", params(lambda r: r["family"] == "act"))
def test_activation_row(rid, storage, sdt):
    row = IC.BY_ID[rid]
    P = Q.OPS[row["op"]].base(row, sdt)
    Q.judge_single(row, sdt, P, launch(_lib.lib(storage), sdt, row, P))


@pytest.mark.parametrize("rid,storage,sdt", params(lambda r: r["family"] == "cast"))
def test_cast_row(rid, storage, sdt):
    """bit-equal to torch's own cast (range_ref.cast_specials: ties, 65504, 65519.99, 65520, +-inf, NaN, the subnormal ends, +-0); the
    zero blocks, pad channels and borders are +0"""
    row = IC.BY_ID[rid]
    lib = _lib.lib(storage)
    op = row["op"]
    P, want = Q.cast_problem(row, sdt)
    if op in ("ctrl_emit", "ctrl_emit_acc"):
        got = run_ctrl_emit(lib, sdt, row, P)["out"]
    elif op == "pixel_unshuffle":
        xd = P["x"].to(DEV)
        B, c, H, W = xd.shape
        y = torch.full(want.shape, float("nan"), dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_pixel_unshuffle(_st(), _p(xd), _lib.dtype_code(xd), B, c, H, W, row["r"], _p(y)), lib)
        got = y.cpu()
    elif op == "tconv_compose":
        wd = P["w"].to(DEV)
        cin, cout = wd.shape[:2]
        y = torch.full((4 * cout, 4 * cin), float("nan"), dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_tconv_compose(_st(), _p(wd), _lib.dtype_code(wd), cin, cout, _p(y)), lib)
        got = y.cpu()
    elif op == "swin_entry":
        xd, mean = P["x"].to(DEV), torch.zeros(3)
        B, _, HW = xd.shape
        y = torch.full((B, HW, 8), float("nan"), dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_swin_entry(_st(), _p(xd), _lib.dtype_code(xd), B, HW, _p(mean), 1.0, _p(y)), lib)
        got = y.cpu()
    elif op == "swin_exit":
        xd, mean = P["x"].to(DEV), torch.zeros(3)
        B, HW, ld = xd.shape
        y = torch.full((B, 3, HW), float("nan"), dtype=want.dtype, device=DEV)
        _lib.check(lib.gyre_op_swin_exit(_st(), _p(xd), ld, B, HW, _p(mean), 1.0, _p(y), CODE[want.dtype]), lib)
        got = y.cpu()
    else:
        assert op == "hed_entry"
        xd = P["x"].to(DEV)
        B, _, H, W = xd.shape
        y = torch.full((B, H + 68, W + 68, 8), float("nan"), dtype=sdt, device=DEV)
        _lib.check(lib.gyre_op_hed_entry(_st(), _p(xd), _lib.dtype_code(xd), B, H, W, _p(y)), lib)
        got = y.cpu()
    torch.cuda.synchronize()
    diff = R.same_bits(got, want)
    R.report(rid, sdt, (), 0, diff, 0.0)
    assert diff == 0, f"{rid}: {diff} elements differ from torch's cast bit for bit"


@pytest.mark.parametrize("rid,storage,sdt", params(lambda r: r["prop"] == "specials"))
def test_specials_row(rid, storage, sdt):
    row = IC.BY_ID[rid]
    lib = _lib.lib(storage)
    op = Q.OPS[row["op"]]
    P = op.base(row, sdt)
    Ps = op.specials(row, P, sdt)
    Q.judge_specials(row, sdt, P, Ps, launch(lib, sdt, row, P), launch(lib, sdt, row, Ps))
