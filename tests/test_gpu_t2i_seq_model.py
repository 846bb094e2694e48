"""The native style adapter and co-adapter fuser (-m gpu; model_t2i_seq.hip behind gyre_amd.t2i.GyreHipT2IStyleAdapter / GyreHipT2IFuser)
against the float64 restatement of the reference's networks (tests/t2i_seq_ref.py, held to what the reference's own classes computed by
tests/test_t2i_seq_host.py), in both storage flavours: tiny and default-size calls, two forwards, batch invariance, workspace sizing,
and the checkpoint's initial state (zeroed spatial_ch_projs / seq_proj), which must return the inputs bit for bit.

The gate of a case is twice the distance (max-abs and rel-L2) of the CPU emulation - the same net in fp32 with every stored tensor
rounded to the storage type at the graph's narrowing points - from the float64 net on that case: the emulation models the roundings,
not the summation order.  The emulation's figures are the constants of EMULATION below; tests/test_t2i_seq_host.py recomputes them and
holds them to these constants, so an emulation that grows looser cannot widen the gate unnoticed."""
import ctypes as C

import pytest
import torch

import t2i_seq_ref as R
from gyre_amd import _lib, config as gcfg, weights
from gyre_amd.modules import set_batch_invariant
from gyre_amd.t2i import GyreHipT2IFuser, GyreHipT2IStyleAdapter
from gpu_util import DEV

pytestmark = pytest.mark.gpu
SDTS = [torch.bfloat16, torch.float16]
_MODEL = {}
DEFAULT_HW = [(8, 8), (4, 4), (2, 2), (1, 1)]                       # the states of a 64 x 64 hint image
# label -> (max-abs, rel-L2) of the storage emulation against the float64 net, as measured (printed again by every run)
EMULATION = {
    "style tiny N=1 S=1 torch.bfloat16": (1.331e-02, 4.621e-03),
    "style tiny N=1 S=1 torch.float16": (2.019e-03, 6.494e-04),
    "style tiny N=3 S=1 torch.bfloat16": (1.769e-02, 5.098e-03),
    "style tiny N=3 S=1 torch.float16": (1.642e-03, 6.509e-04),
    "style tiny N=1 S=5 torch.bfloat16": (1.653e-02, 6.307e-03),
    "style tiny N=1 S=5 torch.float16": (2.502e-03, 6.765e-04),
    "style tiny N=3 S=5 torch.bfloat16": (2.052e-02, 5.573e-03),
    "style tiny N=3 S=5 torch.float16": (2.557e-03, 5.900e-04),
    "style tiny N=1 S=50 torch.bfloat16": (1.685e-02, 4.882e-03),
    "style tiny N=1 S=50 torch.float16": (1.526e-03, 6.261e-04),
    "style tiny N=3 S=50 torch.bfloat16": (1.529e-02, 4.368e-03),
    "style tiny N=3 S=50 torch.float16": (2.108e-03, 6.352e-04),
    "style default N=1 S=257 torch.bfloat16": (2.153e-02, 4.840e-03),
    "style default N=1 S=257 torch.float16": (2.492e-03, 5.866e-04),
    "fuser one_spatial torch.bfloat16 maps[0]": (3.805e-02, 4.499e-03),
    "fuser one_spatial torch.bfloat16 maps[1]": (3.649e-02, 3.117e-03),
    "fuser one_spatial torch.bfloat16 maps[2]": (2.778e-02, 3.762e-03),
    "fuser one_spatial torch.bfloat16 maps[3]": (3.898e-02, 3.819e-03),
    "fuser one_spatial torch.float16 maps[0]": (5.799e-03, 5.142e-04),
    "fuser one_spatial torch.float16 maps[1]": (4.028e-03, 4.612e-04),
    "fuser one_spatial torch.float16 maps[2]": (4.803e-03, 5.269e-04),
    "fuser one_spatial torch.float16 maps[3]": (4.097e-03, 3.589e-04),
    "fuser two_spatial_one_style torch.bfloat16 maps[0]": (6.894e-02, 3.571e-03),
    "fuser two_spatial_one_style torch.bfloat16 maps[1]": (4.948e-02, 4.003e-03),
    "fuser two_spatial_one_style torch.bfloat16 maps[2]": (2.996e-02, 4.185e-03),
    "fuser two_spatial_one_style torch.bfloat16 maps[3]": (4.651e-02, 4.368e-03),
    "fuser two_spatial_one_style torch.bfloat16 tokens[0]": (4.113e-02, 3.959e-03),
    "fuser two_spatial_one_style torch.float16 maps[0]": (8.585e-03, 4.553e-04),
    "fuser two_spatial_one_style torch.float16 maps[1]": (5.963e-03, 4.745e-04),
    "fuser two_spatial_one_style torch.float16 maps[2]": (4.992e-03, 5.264e-04),
    "fuser two_spatial_one_style torch.float16 maps[3]": (4.559e-03, 5.974e-04),
    "fuser two_spatial_one_style torch.float16 tokens[0]": (3.873e-03, 4.211e-04),
    "fuser two_token_inputs torch.bfloat16 tokens[0]": (3.997e-02, 3.691e-03),
    "fuser two_token_inputs torch.float16 tokens[0]": (2.687e-03, 3.876e-04),
    "fuser default torch.bfloat16 maps[0]": (5.851e-02, 4.198e-03),
    "fuser default torch.bfloat16 maps[1]": (6.028e-02, 3.849e-03),
    "fuser default torch.bfloat16 maps[2]": (4.740e-02, 4.082e-03),
    "fuser default torch.bfloat16 maps[3]": (4.483e-02, 3.816e-03),
    "fuser default torch.bfloat16 tokens[0]": (4.703e-02, 3.738e-03),
    "fuser default torch.float16 maps[0]": (6.646e-03, 5.277e-04),
    "fuser default torch.float16 maps[1]": (6.424e-03, 4.811e-04),
    "fuser default torch.float16 maps[2]": (6.103e-03, 4.604e-04),
    "fuser default torch.float16 maps[3]": (4.466e-03, 4.333e-04),
    "fuser default torch.float16 tokens[0]": (4.546e-03, 4.516e-04),
}
STYLE_SHAPES = [("tiny", 1, 1), ("tiny", 3, 1), ("tiny", 1, 5), ("tiny", 3, 5), ("tiny", 1, 50), ("tiny", 3, 50), ("default", 1, 257)]
DEFAULT_FUSER_SPEC = [("sketch", "spatial", 0, 51), ("style", "tokens", 8, 52)]


def _cfg(kind, size):
    return {("style", "tiny"): gcfg.tiny_t2i_style, ("style", "default"): gcfg.t2i_style_config,
            ("fuser", "tiny"): gcfg.tiny_t2i_fuser, ("fuser", "default"): gcfg.t2i_fuser_config}[(kind, size)]()


def state_dict(kind, size, sdt, zero=()):
    """(configuration, state dict with every tensor rounded to sdt: what a module moved to sdt holds)"""
    cfg = _cfg(kind, size)
    shapes = weights.t2i_style_param_shapes(cfg) if kind == "style" else weights.t2i_fuser_param_shapes(cfg)
    sd = {k: v.to(sdt).float() for k, v in weights.synthetic_state_dict(shapes, 31 if kind == "style" else 32).items()}
    for k in sd:
        if zero and k.startswith(zero):
            sd[k] = torch.zeros_like(sd[k])
    return cfg, sd


def _model(kind, size, sdt, zero=()):
    """(module on the GPU, its configuration, its state dict) - one per file"""
    key = (kind, size, sdt, zero)
    if key not in _MODEL:
        cfg, sd = state_dict(kind, size, sdt, zero)
        m = (GyreHipT2IStyleAdapter if kind == "style" else GyreHipT2IFuser)(cfg)
        m.load_state_dict(sd, strict=True)
        _MODEL[key] = (m.to(sdt).to(DEV), cfg, sd)
    return _MODEL[key]


def emulation_distance(emu, ref):
    return float((emu.double() - ref).abs().max()), R.rel_l2(emu, ref)


def stored(feats, sdt):
    return [(n, [m.to(sdt).float() for m in v] if isinstance(v, list) else v) for n, v in feats]


def _gate(label, got, ref, emu):
    ma, rl = emulation_distance(got, ref)
    ema, erl = EMULATION[label]
    now = emulation_distance(emu, ref)
    print(f"[t2i_seq] {label}: max-abs {ma:.3e} (emulation {now[0]:.3e}, stored {ema:.3e}), rel-L2 {rl:.3e} (emulation {now[1]:.3e}, stored {erl:.3e})")
    return ma <= 2 * ema and rl <= 2 * erl


def _to_dev(feats, sdt):
    """fuser inputs on the GPU: the states in the storage type (what the native adapters emit), the tokens in fp32"""
    return [(n, [m.to(sdt).to(DEV) for m in v] if isinstance(v, list) else v.to(DEV)) for n, v in feats]


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("size,N,S", STYLE_SHAPES)
def test_style_adapter_against_the_fp64_net(size, N, S, sdt):
    m, cfg, sd = _model("style", size, sdt)
    x = R.style_input(N, S, cfg["width"])
    ref = R.style_net(sd, cfg, x, compute=torch.float64)
    emu = R.style_net(sd, cfg, x, store=sdt)
    got = m(x.to(DEV))
    assert got.dtype == sdt and tuple(got.shape) == (N, cfg["num_token"], cfg["context_dim"]) and got.is_contiguous()
    assert _gate(f"style {size} N={N} S={S} {sdt}", got.float().cpu(), ref, emu), "outside twice the emulation's distance"
    assert torch.equal(R.bits(got.cpu()), R.bits(m(x.to(DEV)).cpu())), "two forwards differ"


def _fuser_check(label, m, cfg, sd, feats, sdt):
    st = stored(feats, sdt)
    ref = R.fuser_net(sd, cfg, st, compute=torch.float64)
    emu = R.fuser_net(sd, cfg, st, store=sdt)
    got = m(_to_dev(feats, sdt))
    again = m(_to_dev(feats, sdt))
    ok = True
    for part, g, r, e, a in zip(("maps", "tokens"), got, ref, emu, again):
        assert (g is None) == (r is None)
        if g is None:
            continue
        gl, rl, el, al = (g, r, e, a) if part == "maps" else ([g], [r], [e], [a])
        for i, (gi, ri, ei, ai) in enumerate(zip(gl, rl, el, al)):
            assert tuple(gi.shape) == tuple(ri.shape) and gi.dtype == (sdt if part == "maps" else torch.float32)
            ok &= _gate(f"fuser {label} {sdt} {part}[{i}]", gi.float().cpu(), ri, ei)
            assert torch.equal(R.bits(gi.cpu()), R.bits(ai.cpu())), "two forwards differ"
    assert ok, "outside twice the emulation's distance"


@pytest.mark.parametrize("sdt", SDTS)
@pytest.mark.parametrize("name", list(R.FUSER_CASES))
def test_fuser_against_the_fp64_net(name, sdt):
    m, cfg, sd = _model("fuser", "tiny", sdt)
    _fuser_check(name, m, cfg, sd, R.fuser_inputs(R.FUSER_CASES[name], cfg), sdt)


@pytest.mark.parametrize("sdt", SDTS)
def test_fuser_at_the_default_size(sdt):
    m, cfg, sd = _model("fuser", "default", sdt)
    _fuser_check("default", m, cfg, sd, R.fuser_inputs(DEFAULT_FUSER_SPEC, cfg, N=1, hw=DEFAULT_HW), sdt)


def test_an_empty_fuser_input_returns_none():
    m, _, _ = _model("fuser", "tiny", torch.bfloat16)
    assert m({}) == (None, None)


@pytest.mark.parametrize("sdt", SDTS)
def test_zeroed_projections_return_the_inputs_bit_for_bit(sdt):
    """spatial_ch_projs (zero_module) and seq_proj (zeros) as a fresh checkpoint has them: alpha = 0 and x @ seq_proj = 0 exactly"""
    m, cfg, _ = _model("fuser", "tiny", sdt, zero=("spatial_ch_projs", "seq_proj"))
    feats = _to_dev(R.fuser_inputs(R.FUSER_CASES["two_spatial_one_style"][1:], cfg), sdt)          # the style tokens and one spatial input
    maps, seq = m(feats)
    assert torch.equal(R.bits(seq.cpu()), R.bits(feats[0][1].cpu()))
    assert all(torch.equal(R.bits(a.cpu()), R.bits(b.cpu())) for a, b in zip(maps, feats[1][1]))


@pytest.mark.parametrize("N", [3, 5])                               # (the channel-gain row-vector product takes another kernel above a batch of 4)
@pytest.mark.parametrize("sdt", SDTS)
def test_results_do_not_depend_on_the_batch_under_batch_invariant_planning(sdt, N):
    ms, cs, _ = _model("style", "tiny", sdt)
    mf, cf, _ = _model("fuser", "tiny", sdt)
    prev = set_batch_invariant(16)
    try:
        x = R.style_input(N, 5, cs["width"]).to(DEV)
        batch = ms(x)
        feats = _to_dev(R.fuser_inputs(R.FUSER_CASES["two_spatial_one_style"], cf, N=N), sdt)
        fmaps, fseq = mf(feats)
        for i in range(N):
            assert torch.equal(R.bits(ms(x[i:i + 1]).cpu()), R.bits(batch[i:i + 1].cpu())), f"style sample {i}"
            one = [(n, [t[i:i + 1].contiguous() for t in v] if isinstance(v, list) else v[i:i + 1].contiguous()) for n, v in feats]
            omaps, oseq = mf(one)
            assert torch.equal(R.bits(oseq.cpu()), R.bits(fseq[i:i + 1].cpu())), f"fuser tokens, sample {i}"
            assert all(torch.equal(R.bits(a.cpu()), R.bits(b[i:i + 1].cpu())) for a, b in zip(omaps, fmaps)), f"fuser maps, sample {i}"
    finally:
        set_batch_invariant(prev)


def test_workspace_dry_run_equals_use():
    m, cfg, _ = _model("style", "tiny", torch.bfloat16)
    L, dev = m._L(), torch.device(DEV)
    N, S = 3, 50
    x = R.style_input(N, S, cfg["width"]).to(DEV)
    want = m(x)
    h = C.c_void_p(m._handle)
    need = L.gyre_t2i_seq_workspace_bytes(h, N, S, 0)
    assert need > 0
    out = torch.empty_like(want)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes, s=S: L.gyre_t2i_style_forward(h, C.c_void_p(_lib.stream_ptr(dev)), C.c_void_p(x.data_ptr()), 0, N, s, C.c_void_p(wp),
                                                        nbytes, C.c_void_p(out.data_ptr()), _lib.BF16)
    _lib.check(call(need), L)                                       # exactly the dry-run size is enough ...
    torch.cuda.synchronize()
    assert torch.equal(R.bits(out.cpu()), R.bits(want.cpu()))
    with pytest.raises(_lib.GyreError):                             # ... and one byte less is refused, not overrun
        _lib.check(call(need - 1), L)
    with pytest.raises(ValueError):
        _lib.check(call(need, 0), L)
    torch.cuda.synchronize()
    limit = R.MAX_LEN[cfg["width"] // cfg["num_head"]]
    assert L.gyre_t2i_seq_workspace_bytes(h, 1, limit - cfg["num_token"], 0) > 0
    assert L.gyre_t2i_seq_workspace_bytes(h, 1, limit - cfg["num_token"] + 1, 0) == 0     # past what the attention kernel holds: refused
    with pytest.raises(NotImplementedError):
        m(torch.zeros((1, limit, cfg["width"]), device=DEV))


def test_fuser_workspace_dry_run_equals_use():
    """the dry run sizes with one pixel per map and no token dtype: neither enters the arena, so its peak is exactly what a call with
    real maps (4 x 6 ... 1 x 1) and fp32 tokens needs"""
    mf, cf, _ = _model("fuser", "tiny", torch.bfloat16)
    L, dev = mf._L(), torch.device(DEV)
    feats = _to_dev(R.fuser_inputs(R.FUSER_CASES["two_spatial_one_style"], cf), torch.bfloat16)
    wmaps, wseq = mf(feats)
    hf = C.c_void_p(mf._handle)
    need = L.gyre_t2i_seq_workspace_bytes(hf, R.FUSER_N, 3, 2)
    assert need > 0 and L.gyre_t2i_seq_workspace_bytes(hf, 2, 0, 0) == 0
    arr = (_lib.FuserInput * 3)()
    for e, (name, v) in zip(arr, feats):
        e.task = R.EXTRA_CONDITION[name]
        if isinstance(v, list):
            for i, m in enumerate(v):
                e.in_[i], e.h[i], e.w[i] = m.data_ptr(), m.shape[2], m.shape[3]
        else:
            e.tokens, e.in_[0] = v.shape[1], v.data_ptr()
    maps, seq = [torch.empty_like(m) for m in wmaps], torch.empty_like(wseq)
    mp = (C.c_void_p * 4)(*[m.data_ptr() for m in maps])
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    call = lambda nbytes: L.gyre_t2i_fuser_forward(hf, C.c_void_p(_lib.stream_ptr(dev)), arr, 3, _lib.F32, R.FUSER_N, C.c_void_p(wp), nbytes, mp,
                                                   C.c_void_p(seq.data_ptr()))
    _lib.check(call(need), L)
    torch.cuda.synchronize()
    assert torch.equal(R.bits(seq.cpu()), R.bits(wseq.cpu())) and all(torch.equal(R.bits(a.cpu()), R.bits(b.cpu())) for a, b in zip(maps, wmaps))
    with pytest.raises(_lib.GyreError):
        _lib.check(call(need - 1), L)
    torch.cuda.synchronize()


def test_refusals():
    with pytest.raises(NotImplementedError):
        gcfg.t2i_style_config(width=80, num_head=2)                 # head dim 40
    L, h = _lib.lib(_lib.BF16), C.c_void_p()
    bad = _lib.T2ISeqCfg(kind=0, width=80, num_head=2, n_layers=1, num_token=2, context_dim=16)
    with pytest.raises(NotImplementedError):
        _lib.check(L.gyre_t2i_seq_create(C.byref(bad), 0, C.byref(h)), L)
    m, cfg, _ = _model("style", "tiny", torch.bfloat16)
    with pytest.raises(ValueError):
        m(torch.zeros((1, 4, cfg["width"] + 8), device=DEV))
    with pytest.raises(_lib.GyreError):
        m(torch.zeros((1, 4, cfg["width"])))                        # CPU tensor: no fallback
    mf, _, _ = _model("fuser", "tiny", torch.bfloat16)
    with pytest.raises(ValueError):
        mf({"nonsense": torch.zeros((1, 2, 64), device=DEV)})
