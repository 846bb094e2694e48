"""A Transformer2D's proj_out folded into the FF2 of its last block (-m gpu): out = [ff | h] [Wp W2 | Wp]^T + (Wp b2 + bp) + x as ONE
launch on weights composed once per weight version (csrc/model_impl.h Exec::proj_out_folded, Store::pf_lookup).

  1. the composed weights (gyre_op_compose_proj_out) against float64, bounds from tests/proj_out_fold_ref.py;
  2. the second source of the pipelined kernel's linear mode (k_gemm4s, A | A2 split at C1), unsplit and in K slices whose boundary
     falls inside the second source: the bits of k_gemm8 on the same problem, and the float64 element bound of tests/gemm_ref.py;
  3. fold on / off (tuning bit 28) on a small two-level UNet with a depth-2 transformer: one launch fewer per transformer, both
     inside the project's gate against the fp32 oracle, the fold no further from it than the two launches (the rule
     tests/test_gpu_models.py uses for the fused cross-attention kernel);
  4. weight updates: after gyre_unet_set_weight on ff.net.2 / proj_out and after a native LoRA merge and its removal the forward pass
     equals a fresh handle's bit for bit (stale composed weights would not);
  5. batch independence under gyre_set_batch_invariant with the fold on.

Operator tests run on both storage flavours in this process (two libraries, _lib.lib(storage)); model tests reach the fp16 library
through ``.to(torch.float16)``.
"""
import ctypes as C

import pytest
import torch

import gemm_ref as GR
import proj_out_fold_ref as R
from gyre_amd import _lib, config as gcfg, lora as LR, weights
from gyre_amd.modules import GyreHipUNet, set_batch_invariant
from gpu_util import DEV, check_bound, randn, rel_l2, release_kept, report, st, vp
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
F64 = torch.float64
NO_FOLD = 0x10000000                 # tuning bit 28 of gyre_debug_gemm_ablation: proj_out stays its own launch
FLAVOURS = [_lib.BF16, _lib.F16]


@pytest.fixture(autouse=True)
def _release():
    yield
    release_kept()


def _hdt(storage):
    return _lib.STORAGE_TORCH_DTYPE[storage]


# ---- 1. composed weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", FLAVOURS, ids=["bf16", "f16"])
@pytest.mark.parametrize("C_", [64, 192])
def test_composed_weights_against_float64(C_, storage):
    L, hdt = _lib.lib(storage), _hdt(storage)
    Wp, W2, b2, bp = R.operands(C_, 11 + C_, hdt)
    wc = torch.full((C_, 5 * C_), -3.0, dtype=hdt, device=DEV)
    bc = torch.full((C_,), -3.0, dtype=torch.float32, device=DEV)
    _lib.check(L.gyre_op_compose_proj_out(st(), vp(Wp.to(hdt).to(DEV)), vp(W2.to(hdt).to(DEV)), vp(b2.float().to(DEV)),
                                          vp(bp.float().to(DEV)), C_, vp(wc), vp(bc)), L)
    torch.cuda.synchronize()
    ref_w, ref_b = R.compose(Wp, W2, b2, bp)
    tw, tb = R.wc_bound(Wp, W2, hdt), R.bc_bound(Wp, b2, bp)
    dw, db = (wc.cpu().to(F64) - ref_w).abs(), (bc.cpu().to(F64) - ref_b).abs()
    rw = float((dw[:, :4 * C_] / tw[:, :4 * C_]).max())
    print(f"[compose] C={C_} {hdt}: worst |Wc - ref| / bound {rw:.3f}, worst |bc - ref| / bound {float((db / tb).max()):.3f}")
    assert torch.isfinite(wc.float()).all() and torch.isfinite(bc).all()
    assert bool((dw <= tw).all())
    assert torch.equal(wc.cpu()[:, 4 * C_:].to(F64), Wp)                  # the copied columns: exact
    assert bool((db <= tb).all())
    with pytest.raises(ValueError):
        _lib.check(L.gyre_op_compose_proj_out(st(), vp(wc), vp(wc), None, None, 72, vp(wc), vp(bc)), L)


# ---- 2. two-source pipelined linear -------------------------------------------------------------------------------------------------
def _two_source_problem(hdt):
    Mr, N, K, C1 = 300, 320, 1280 + 320, 1280
    a, w = GR.gauss_operands((Mr, K), (N, K), K, 71, hdt)
    bias, res = GR.gauss_addend((N,), 72), GR.gauss_addend((Mr, N), 73, hdt)
    value, bound = GR.reference(a, w, bias, None, 1, res)
    return dict(M=Mr, N=N, K=K, C1=C1, a=a, w=w, bias=bias, res=res, value=value, bound=bound)


def _run_two_source(L, hdt, p, cfg, splits):
    Mr, N, K, C1 = p["M"], p["N"], p["K"], p["C1"]
    # separate buffers of their own widths, as the model hands them over: ff [M][4C], h [M][C]
    a1 = p["a"][:, :C1].contiguous().to(hdt).to(DEV)
    a2 = p["a"][:, C1:].contiguous().to(hdt).to(DEV)
    w = p["w"].to(hdt).to(DEV)
    bias, res = p["bias"].float().to(DEV), p["res"].to(hdt).to(DEV)
    rows = GR.CANARY_ROWS
    out = torch.full((Mr + rows, N), GR.CANARY, dtype=hdt, device=DEV)
    ws = torch.zeros(max(1, splits) * Mr * N, dtype=torch.float32, device=DEV)
    a = _lib.GemmTestArgs()
    a.conv, a.M, a.K, a.N = 0, Mr, K, N
    a.A, a.lda, a.A2, a.lda2, a.C1 = a1.data_ptr(), C1, a2.data_ptr(), K - C1, C1
    a.W, a.bias, a.residual, a.ldr, a.out, a.ldc = w.data_ptr(), bias.data_ptr(), res.data_ptr(), N, out.data_ptr(), N
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    old = L.gyre_debug_force_gemm_cfg(cfg | (splits << 8))
    try:
        rc, plan = GR.plan_query(L, a)
        assert rc == 0 and plan["cfg"] == cfg and plan["splits"] == max(1, splits), plan
        _lib.check(L.gyre_op_gemm_test(st(), C.byref(a)), L)
        torch.cuda.synchronize()
    finally:
        L.gyre_debug_force_gemm_cfg(old)
    del a1, a2, w, bias, res, ws
    assert bool((out[Mr:] == GR.CANARY).all()), "rows past M were written"
    return out[:Mr].cpu()


@pytest.mark.parametrize("storage", FLAVOURS, ids=["bf16", "f16"])
def test_two_source_pipelined_linear_has_the_8_wave_kernels_bits(storage):
    """M = 300 (ragged), N = 320, K = 1280 + 320 split at C1 = 1280 (K step 20 of 25).  Four K slices are steps 0-6, 7-13, 14-20, 21-24: the
    third slice crosses C1 in its last step and the boundary at step 21 lies strictly inside the second source.  Tile config 24
    (8-wave 256x320, the pipelined form that takes a second source) against config 4 (k_gemm8, 256x320) with the same slicing."""
    L, hdt = _lib.lib(storage), _hdt(storage)
    p = _two_source_problem(hdt)
    per = -(-(p["K"] // 64) // 4)                          # K steps per slice, as the launchers cut them
    assert p["C1"] < 3 * per * 64 < p["K"] and 2 * per * 64 < p["C1"]
    for splits in (0, 4):
        ref8 = _run_two_source(L, hdt, p, 4, splits)
        check_bound(f"k_gemm8 two sources, splits {splits}", ref8, p["value"], p["bound"], k=GR.gauss_k(p["K"], hdt), hdt=hdt,
                    dims=("m", "n"))
        for cfg in (24,):
            got = _run_two_source(L, hdt, p, cfg, splits)
            check_bound(f"k_gemm4s cfg {cfg} two sources, splits {splits}", got, p["value"], p["bound"], k=GR.gauss_k(p["K"], hdt),
                        hdt=hdt, dims=("m", "n"))
            assert torch.equal(got, ref8), f"cfg {cfg}, splits {splits}: bits differ from k_gemm8"


# ---- 3 - 5: the small UNet ----------------------------------------------------------------------------------------------------------
def small_cfg():
    return gcfg.UNetConfig(block_out_channels=(64, 128), attn_levels=(True, True), num_heads=(2, 4), transformer_depth=(1, 2),
                           cross_attention_dim=64, sample_size=16)


def n_transformers(cfg):
    n = sum(cfg.layers_per_block + (cfg.layers_per_block + 1) for lvl in cfg.attn_levels if lvl)
    return n + 1                                                          # + the middle block's


def make_net(cfg, dtype=None, seed=0, sd=None):
    net = GyreHipUNet(cfg)
    sd = sd if sd is not None else weights.synthetic_state_dict(weights.unet_param_shapes(cfg), seed)
    net.load_state_dict(sd)
    if dtype is not None:
        net = net.to(dtype)
    return net.to(DEV), sd


@pytest.fixture(scope="module")
def small():
    """Config, state dict, inputs (batch 3: M = 768 / 192 rows, ragged for every tile) and the fp32 oracle's answer - computed once."""
    cfg = small_cfg()
    sd = weights.synthetic_state_dict(weights.unet_param_shapes(cfg), 0)
    x, t, ctx = randn(3, 4, 16, 16, seed=61), torch.tensor([640, 640, 640]), randn(3, 77, cfg.cross_attention_dim, seed=62)
    return cfg, sd, (x, t, ctx), M.unet_forward(sd, cfg, x, t, ctx)


def fwd(net, inp):
    x, t, ctx = inp
    return net(x.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV)).sample.clone()


@pytest.mark.parametrize("dtype", [None, torch.float16], ids=["default", "f16"])
def test_fold_on_and_off_on_a_small_unet(small, dtype):
    cfg, sd, inp, ref = small
    net, _ = make_net(cfg, dtype, sd=sd)
    L = net._L()
    outs, launches = {}, {}
    for bits in (NO_FOLD, 0):
        old = L.gyre_debug_gemm_ablation(bits)
        try:
            fwd(net, inp)                                   # first call: the per-handle weight copies (composed weights included)
            outs[bits] = fwd(net, inp).float().cpu()
            launches[bits] = L.gyre_last_launch_count()
        finally:
            L.gyre_debug_gemm_ablation(old)
    # one launch per TRANSFORMER, not per block: the depth-2 transformers of the second level fold their last block only
    assert launches[NO_FOLD] - launches[0] == n_transformers(cfg), (launches, n_transformers(cfg))
    assert not torch.equal(outs[0], outs[NO_FOLD])          # (one rounding fewer: the folded path really ran)
    report("small UNet, proj_out folded into FF2", outs[0], ref, 3e-2)
    report("small UNet, FF2 and proj_out as two launches", outs[NO_FOLD], ref, 3e-2)
    e_fold, e_two = rel_l2(outs[0], ref), rel_l2(outs[NO_FOLD], ref)
    print(f"[fold] e_fold {e_fold:.4e} e_two_launch {e_two:.4e}")
    assert e_fold < 1.3 * e_two + 1e-3, (e_fold, e_two)
    assert torch.equal(outs[0], fwd(net, inp).float().cpu())               # deterministic


def _set_weight(net, key, tensor):
    """gyre_unet_set_weight of one key on the live handle, and the same value into the module's parameter (for the fresh twin)."""
    L = net._L()
    t = tensor.to(DEV).contiguous()
    shape = (C.c_int64 * t.ndim)(*t.shape)
    _lib.check(L.gyre_unet_set_weight(C.c_void_p(net._handle), key.encode(), C.c_void_p(t.data_ptr()), _lib.dtype_code(t), shape, t.ndim,
                                      st()), L)
    _lib.check(L.gyre_unet_finalize(C.c_void_p(net._handle), st()), L)          # (gyre_unet_set_weight leaves the handle un-finalized)
    torch.cuda.synchronize()
    net._ctx_slots = []                                     # the native context cache went with the weight version
    with torch.no_grad():
        dict(net.named_parameters())[key].copy_(t)


def _lora(net, names, r=4, seed=0):
    params = dict(net.named_parameters())
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in names:
        w = params[name + ".weight"]
        O, I = w.shape[:2]
        tail = tuple(w.shape[2:])
        k = "lora_unet_" + name.replace(".", "_")
        out[k + ".lora_up.weight"] = (torch.randn(O, r, generator=g) * 0.3).reshape((O, r) + (1,) * len(tail))
        out[k + ".lora_down.weight"] = (torch.randn(r, I, generator=g) * 0.3).reshape((r, I) + tail)
        out[k + ".alpha"] = torch.tensor(float(r))
    return out


def test_composed_weights_follow_weight_updates(small):
    cfg, sd, inp, _ = small
    net, _ = make_net(cfg, sd=sd)
    base = fwd(net, inp)                                    # composed weights of every transformer exist from here on
    site = "up_blocks.0.attentions.1"                       # second level: depth 2, the LAST block's FF2 is the folded one
    k_ff2, k_po = site + ".transformer_blocks.1.ff.net.2.weight", site + ".proj_out.weight"
    cur = {k: v.clone() for k, v in sd.items()}

    def fresh():
        twin, _ = make_net(cfg, sd=cur)
        return fwd(twin, inp)
    last = base
    for i, key in enumerate((k_ff2, k_po)):
        cur[key] = (sd[key].float() * (1.5 if i == 0 else -0.75) + randn(*sd[key].shape, seed=80 + i) * 0.02).to(sd[key].dtype)
        _set_weight(net, key, cur[key])
        got = fwd(net, inp)
        assert not torch.equal(got, last), f"{key}: the update did not change the output"
        assert torch.equal(got, fresh()), f"{key}: stale composed weights"
        last = got
    # a native LoRA on the same two matrices, and its exact removal
    lora = _lora(net, [k_ff2[:-len('.weight')], k_po[:-len('.weight')]])
    assert LR.attach_lora(net, lora, "x", 0.5) == 2
    merged = fwd(net, inp)
    assert not torch.equal(merged, last)
    twin, _ = make_net(cfg, sd=cur)
    assert LR.attach_lora(twin, lora, "x", 0.5) == 2
    assert torch.equal(merged, fwd(twin, inp)), "stale composed weights after the LoRA merge"
    LR.detach_loras(net)
    assert torch.equal(fwd(net, inp), last) and torch.equal(last, fresh()), "stale composed weights after the LoRA was taken off"


def test_fold_is_batch_independent_under_batch_invariant_planning(small):
    cfg, sd, _, _ = small
    net, _ = make_net(cfg, sd=sd)
    x, t, ctx = randn(4, 4, 16, 16, seed=91), torch.tensor([500] * 4), randn(4, 77, cfg.cross_attention_dim, seed=92)
    prev = set_batch_invariant(4)
    try:
        fwd(net, (x, t, ctx))                               # first call: the per-handle weight copies
        full = fwd(net, (x, t, ctx))
        n_fold = net._L().gyre_last_launch_count()
        for lo, hi in ((0, 2), (2, 4)):
            part = fwd(net, (x[lo:hi].contiguous(), t[lo:hi], ctx[lo:hi].contiguous()))
            assert net._L().gyre_last_launch_count() == n_fold
            assert torch.equal(part, full[lo:hi]), (lo, hi)
        old = net._L().gyre_debug_gemm_ablation(NO_FOLD)
        try:
            fwd(net, (x, t, ctx))
            assert net._L().gyre_last_launch_count() == n_fold + n_transformers(cfg)       # the fold was on above
        finally:
            net._L().gyre_debug_gemm_ablation(old)
    finally:
        set_batch_invariant(prev)
