"""The case table of tests/test_gpu_range.py, as data (no GPU import; tests/test_range_ref_host.py builds every row on the CPU and
asserts the conditions its property needs from the float64 reference alone).

The family puts values at the two ends of the 16-bit storage type's range - fp16 ends at 65504 and goes subnormal below 2^-14,
bf16 shares fp32's exponents - where the rest of the suite (lattice integers, randn, randn / sqrt(K): all O(1)) never goes.

A row is a dict:
  id      unique name
  family  gemm | conv | norm | attn | xattn | tome | elem | temb | lora       (which runner of tests/test_gpu_range.py)
  op      the entry point's form: for gemm / conv rows the `op` of tests/gemm_cases.py (linear, linear_t, qkv, conv, conv_nchw)
  base    gemm / conv rows: the tests/gemm_cases.py-style row (shape, feats, kind, cfg, splits, abl) of the O(1) BASE problem
  prop    the range property the row stands for (PROPS below)
  only    storage types the row is built for: ("f16",) for the rows that need headroom between storage and accumulator
  exps    storage name -> exponents.  gemm / conv rows: (ka, kw) - the A operand is scaled by 2^ka, the weights by 2^kw, every
          addend (bias, row bias, residual) by 2^(ka + kw); the other families: (k,).  Derived, never guessed:
          tests/range_ref.py:derive_exps computes them from the float64 reference of the base problem, EXPS below records the
          answers and the host test asserts that record and derivation agree and that the scaled maximum lies in (top / 2, top].

Shapes are the ones tests/gemm_cases.py argues for: M tail of 33 rows, K tail of 8, N tail of 8 (VARIANT_BASE), the 3 x 9 x 7 image."""
from gemm_cases import AR, BY_ID as GEMM_ROWS, SM, VARIANT_BASE, ZFILL, kind_of

PROPS = {
    "top": "outputs scaled so that the largest lies in (top / 2, top]: a result narrowed too early, or summed in 16 bits, is inf",
    "cancel": "K holds +2^18 and -2^18 (+ the in-range lattice value): the fp32 partial sums leave fp16, the result does not",
    "bias_back": "accumulator at 2^17, brought back into range by the fp32 bias",
    "rowbias_back": "accumulator at 2^17, brought back into range by the fp32 row bias",
    "res_order": "accumulator 2^15 + bias 49152 = 81920 > 65504, residual -49152: in range only if the sum is narrowed once, at the end",
    "geglu": "value half beyond 65504 times a small gelu(gate): in range only if the product is formed before the narrowing",
    "sub_act": "every non-zero activation is subnormal in fp16, weights x 2^j: the outputs are normal",
    "sub_w": "every non-zero weight is subnormal in fp16 (through the repack kernels), activations x 2^j: the outputs are normal",
    "sub_act_gauss": "Gaussian activations on the quantum 2^-6 (10-bit significands) x 2^-18: fp16 subnormals whose sums are NOT exact in fp32",
    "sub_w_gauss": "Gaussian weights on the quantum 2^-10 x 2^-14: fp16 subnormals whose sums are NOT exact in fp32",
    "sub_out": "lattice outputs that are integers x 2^-24: fp16 subnormal results must come back exact",
    "invariant": "x -> 2^k x with eps -> 4^k eps: a normalisation's output is unchanged bit for bit, at both ends of the range",
    "fold": "x scaled down: the folded weights W rstd gamma, stored in 16 bits, reach the top of the range (and the bias does not move)",
    "convex": "V scaled to the top / into the subnormals: an attention output is a convex combination, it scales exactly",
    "mean3": "three tokens near top / 2 are merged: their fp32 sum exceeds the top, their mean does not",
    "cast": "bit-equal to torch's cast at ties, 65504, 65519.99, 65520, +-inf, NaN and the subnormal ends",
}
F16_ONLY = ("f16",)
BOTH = ("f16", "bf16")
ROWS = []


def row(id, family, op, prop, only=BOTH, **kw):
    assert all(r["id"] != id for r in ROWS), id
    assert prop in PROPS, prop
    ROWS.append(dict(id=id, family=family, op=op, prop=prop, only=tuple(only), **kw))


def base(op, kind, cfg=0, splits=0, abl=0, **kw):
    """A tests/gemm_cases.py-style row of the base problem (gemm_ref.build_case reads it)."""
    shape = {k: kw.pop(k) for k in ("M", "K", "N", "B", "H", "W", "Cin", "Cout") if k in kw}
    return dict(op=op, kind=kind, cfg=cfg, splits=splits, abl=abl, rc=0, why="", plan={}, covers=(), shape=shape, feats=kw)


def _gemm_row(id, family, op, prop, kind, only=BOTH, **kw):
    b = base(op, kind, **kw)
    b["id"] = "range-" + id              # (the seed of the data comes from the id)
    row(id, family, op, prop, only=only, base=b)


# the offset rows: which addends the base problem carries
_ADDENDS = {"cancel": dict(bias=1), "bias_back": dict(bias=1), "rowbias_back": dict(bias=1, rowbias=1, rps=17), "res_order": dict(bias=1, res=1)}

# ---- GEMM / linear through gyre_op_gemm_test, one forced config per kernel family ---------------------------------------------------
for c, (M, K, N) in VARIANT_BASE.items():
    fam = kind_of(c)
    _gemm_row(f"lin-top-cfg{c}", "gemm", "linear", "top", "gauss", cfg=c, M=M, K=K, N=N, bias=1, res=1)
    for prop, ft in _ADDENDS.items():
        if prop == "rowbias_back" and fam not in ("4w", "8w", "4s"):
            continue                      # small / A-resident kernels have no row bias (gemm_cases: lin-rowbias-*-refused)
        _gemm_row(f"lin-{prop}-cfg{c}", "gemm", "linear", prop, "lattice", only=F16_ONLY, cfg=c, M=M, K=K, N=N, **ft)
    _gemm_row(f"lin-sub_act-cfg{c}", "gemm", "linear", "sub_act", "lattice", cfg=c, M=M, K=K, N=N, bias=1)
    _gemm_row(f"lin-sub_w-cfg{c}", "gemm", "linear", "sub_w", "lattice", cfg=c, M=M, K=K, N=N, bias=1)
    _gemm_row(f"lin-sub_out-cfg{c}", "gemm", "linear", "sub_out", "lattice", cfg=c, M=M, K=K, N=N, bias=1, res=1)
# subnormal operands with full significands: the lattice rows above are exact in any arithmetic; these see HOW the matrix instruction
# accumulates subnormal operands (outputs are normal; check 1 demands the bits of the O(1) run)
for c, (M, K, N) in VARIANT_BASE.items():
    _gemm_row(f"lin-sub_act_gauss-cfg{c}", "gemm", "linear", "sub_act_gauss", "gauss", cfg=c, M=M, K=K, N=N, bias=1)
    _gemm_row(f"lin-sub_w_gauss-cfg{c}", "gemm", "linear", "sub_w_gauss", "gauss", cfg=c, M=M, K=K, N=N, bias=1)
# forced split-K: slice 0 holds +2^18, slice 4 holds -2^18 (36 steps in 5 slices); and subnormal weights through the blocked pack
for c in (4, 5, 6, 7, 8, 24):
    N = 256 if c in (6, 7) else 320
    _gemm_row(f"splitk-cancel-cfg{c}", "gemm", "linear", "cancel", "lattice", only=F16_ONLY, cfg=c, splits=5, M=289, K=2304, N=N, bias=1)
_gemm_row("splitk-top-cfg8", "gemm", "linear", "top", "gauss", cfg=8, splits=5, M=289, K=2304, N=320, bias=1, res=1)
_gemm_row("blocked-sub_w-cfg8", "gemm", "linear", "sub_w", "lattice", cfg=8, splits=5, M=289, K=2304, N=320, bias=1, wblk=1)
_gemm_row("blocked-sub_act-cfg32", "gemm", "linear", "sub_act", "lattice", cfg=SM, M=289, K=1088, N=320, bias=1, wblk=1)
# GEGLU on one GEGLU-capable tile of each family (the small kernel has none)
for c in (1, 6, 22, AR):
    _gemm_row(f"geglu-top-cfg{c}", "gemm", "linear", "geglu", "gauss", cfg=c, M=289, K=320 if c == AR else 192, N=192 if c == AR else 176,
              bias=1, geglu=1)
    _gemm_row(f"geglu-sub_w-cfg{c}", "gemm", "linear", "sub_w", "lattice", cfg=c, M=289, K=320 if c == AR else 192,
              N=192 if c == AR else 176, bias=1, geglu=1)
# transposed output and the fused Q | K | V^T
_gemm_row("lin-transposed-top-cfg1", "gemm", "linear_t", "top", "gauss", cfg=1, M=154, K=72, N=36, bias=1, tokens=77, ldt=80)
for c, C, tok in ((5, 320, 40), (SM, 64, 40), (AR, 320, 64)):
    _gemm_row(f"qkv-top-cfg{c}", "gemm", "qkv", "top", "gauss", cfg=c, M=2 * tok, K=C, N=3 * C, tokens=tok, ldt=tok + 8)
    _gemm_row(f"qkv-sub_act-cfg{c}", "gemm", "qkv", "sub_act", "lattice", cfg=c, M=2 * tok, K=C, N=3 * C, tokens=tok, ldt=tok + 8)

# fused column and row statistics at the top of the range: the rows of tests/gemm_cases.py the planner fuses (M is the planner's)
for gid in ("colstats-linear-cfg8", "colstats-conv-splitk", "rowstats-linear-cfg8"):
    b = dict(GEMM_ROWS[gid], id="range-" + gid)
    row(f"{gid}-top", "gemm", b["op"], "top", base=b)
# subnormal operands for the remaining forms: transposed output, Q | K | V^T weights, GEGLU activations
_gemm_row("lin-transposed-sub_act-cfg1", "gemm", "linear_t", "sub_act", "lattice", cfg=1, M=154, K=72, N=36, bias=1, tokens=77, ldt=80)
for c, C, tok in ((5, 320, 40), (SM, 64, 40), (AR, 320, 64)):
    _gemm_row(f"qkv-sub_w-cfg{c}", "gemm", "qkv", "sub_w", "lattice", cfg=c, M=2 * tok, K=C, N=3 * C, tokens=tok, ldt=tok + 8)
for c in (1, 6, 22, AR):
    _gemm_row(f"geglu-sub_act-cfg{c}", "gemm", "linear", "sub_act", "lattice", cfg=c, M=289, K=320 if c == AR else 192,
              N=192 if c == AR else 176, bias=1, geglu=1)

# ---- 3x3 convolutions: configs 1, 5, 12, 24, each with and without zero-fill -----------------------------------------------------------
for c in (1, 5, 12, 24):
    for abl in (0, ZFILL):
        tag = f"cfg{c}" + ("z" if abl else "")
        Cout = 136 if c == 12 else 328
        g = dict(cfg=c, abl=abl, B=3, H=9, W=7, Cin=64, Cout=Cout)
        _gemm_row(f"conv-top-{tag}", "conv", "conv", "top", "gauss", bias=1, res=1, **g)
        for prop in ("cancel", "bias_back", "res_order"):
            # cancel: two 64-channel chunks, so that chunk-major kernels hold the sum of up to nine taps (9 x 2^15) between them
            gp = dict(g, Cin=128) if prop == "cancel" else g
            _gemm_row(f"conv-{prop}-{tag}", "conv", "conv", prop, "lattice", only=F16_ONLY, **gp, **_ADDENDS[prop])
        _gemm_row(f"conv-sub_act-{tag}", "conv", "conv", "sub_act", "lattice", bias=1, **g)
        _gemm_row(f"conv-sub_w-{tag}", "conv", "conv", "sub_w", "lattice", bias=1, **g)
        if not abl:
            _gemm_row(f"conv-sub_act_gauss-{tag}", "conv", "conv", "sub_act_gauss", "gauss", bias=1, **g)
for c in (1, 5, 12, 24):
    Cout = 136 if c == 12 else 328
    if True:
        _gemm_row(f"conv-sub_out-cfg{c}", "conv", "conv", "sub_out", "lattice", bias=1, res=1, cfg=c, B=3, H=9, W=7, Cin=64, Cout=Cout)
# the folded 1x1 shortcut (gyre_op_conv3x3_shortcut) at the top of the range: the rows of tests/gemm_cases.py the planner folds
for gid in ("shortcut-two-sources", "shortcut-one-source"):
    row(f"{gid}-top", "conv", "shortcut", "top", base=dict(GEMM_ROWS[gid], id="range-" + gid))
# the output convolution and its tile twin, all three NCHW output dtypes (an f16 output of the bf16 flavour becomes inf above 65520)
for dt, dn in ((0, "f32"), (1, "bf16"), (2, "f16")):
    for ft in (0, 1):
        _gemm_row(f"convout-top-{dn}" + ("-tiles" if ft else ""), "conv", "conv_nchw", "top", "lattice", B=2, H=13, W=21, Cin=64, Cout=4,
                  bias=1, dtype=dt, force_tiles=ft)
        _gemm_row(f"convout-sub_act-{dn}" + ("-tiles" if ft else ""), "conv", "conv_nchw", "sub_act", "lattice", B=2, H=13, W=21, Cin=64,
                  Cout=4, bias=1, dtype=dt, force_tiles=ft)

# ---- GroupNorm / LayerNorm: x -> 2^k x, eps -> 4^k eps to both ends -----------------------------------------------------------------------
# (B, H, W, C, C1, G, silu): k_gn_small, k_gn_small with two sources, the large path with 1 / 2 / 4 vectors per thread, two sources
for i, (B, H, W, C, C1, G, silu) in enumerate([(2, 16, 16, 384, 0, 32, 1), (2, 16, 16, 384, 200, 32, 0), (2, 33, 33, 320, 0, 32, 1),
                                               (2, 33, 33, 960, 640, 32, 1), (2, 17, 17, 2560, 1280, 32, 0), (2, 17, 17, 8192, 0, 32, 1)]):
    for end in ("up", "down"):
        row(f"gn-{end}-{B}x{H}x{W}x{C}-C1-{C1}", "norm", "groupnorm", "invariant", shape=dict(B=B, H=H, W=W, C=C, C1=C1, G=G), silu=silu,
            end=end, seed=10 * i)
for M, C in ((7, 320), (3, 520), (33, 1280)):
    for end in ("up", "down"):
        row(f"ln-{end}-{M}x{C}", "norm", "layernorm", "invariant", shape=dict(M=M, C=C), end=end, seed=M + C)
for end in ("up", "down"):
    row(f"gn-colstats-{end}", "norm", "groupnorm_colstats", "invariant", shape=dict(B=2, H=32, W=32, C=640, C1=320, G=32), silu=1, end=end,
        seed=77, unit=10, rows=(256, 16))

# the LayerNorm folded into its consuming GEMM, plain and GEGLU, at the smallest M the planner keeps folded (the host test asks it)
for tag, M, N, geglu in (("plain", 10113, 320, 0), ("geglu", 1921, 1280, 1)):
    for end in ("up", "down"):
        row(f"ln_linear-{end}-{tag}", "norm", "ln_linear", "invariant", shape=dict(M=M, C=320), N=N, geglu=geglu, end=end, seed=320 + geglu)
# ... and with the row statistics of the producing GEMM (one part: sum and sum of squares per row) in place of the statistics pass
for end in ("up", "down"):
    row(f"ln_linear-{end}-parts", "norm", "ln_linear", "invariant", shape=dict(M=10113, C=320), N=320, geglu=0, parts=1, end=end, seed=321)
# the GroupNorm fold: x scaled down until the folded weights W rstd gamma reach the top of the range
for B, H, W, C, N, producer in ((3, 33, 33, 64, 8, 1), (2, 17, 17, 1280, 38, 0)):
    row(f"gn_fold-{B}x{H}x{W}x{C}-N{N}-producer{producer}", "norm", "gn_fold", "fold", shape=dict(B=B, H=H, W=W, C=C, C1=0, G=32), N=N,
        producer=producer, unit=2, end="down", seed=C + N)

# ---- attention forward: V at the top and in the subnormals, one D per kernel family plus D = 512 ---------------------------------------------
# branch (tests/attn_cases.BRANCHES), D, (Nq, Nk)
for branch, D, shp in (("k_attn", 8, (65, 65)), ("k_attn", 512, (65, 65)), ("auto_plain", 64, (129, 77)), ("attn2_plain", 40, (129, 77)),
                       ("attn2_plain_q64", 32, (129, 77)), ("attn2_folded", 40, (129, 77)), ("prescaled_no_folded_form", 80, (129, 77)),
                       ("attn3_optimistic", 40, (63, 257)), ("attn3_checked", 64, (63, 257)), ("attn3_short_keys", 80, (129, 77))):
    for end in ("up", "down"):
        row(f"attn-{end}-{branch}-D{D}", "attn", "attention", "convex", branch=branch, D=D, shape=dict(Nq=shp[0], Nk=shp[1]), end=end)

# the fused cross-attention block (its only shape): x, V and the output bias scaled together - LayerNorm(x) and so q do not move, the
# attention output, re-packed as the operand of the output projection, and the stored result scale by 2^k
row("xattn-block-top-Nk77", "xattn", "cross_attention_block", "top", shape=dict(B=8, tokens=4096, C=320, heads=8, Nk=77))

# ---- ToMe: three tokens near top / 2 merged into one ----------------------------------------------------------------------------------------
for case in ((2, 136, 64, 17), (2, 137, 320, 40)):
    row("tome-mean3-" + "x".join(map(str, case)), "tome", "tome_merge", "mean3", shape=dict(zip(("B", "N", "C", "r"), case)))

row("tome-unmerge-top-2x136x64x17", "tome", "tome_unmerge", "top", shape=dict(B=2, N=136, C=64, r=17))

# ---- boundary and element-wise kernels, bit-equal to torch casts ------------------------------------------------------------------------------
for src in ("f32", "bf16", "f16"):
    row(f"elem-nchw_to_nhwc-{src}", "elem", "nchw_to_nhwc", "cast", src=src)
    row(f"elem-pixel_unshuffle8-{src}", "elem", "pixel_unshuffle8", "cast", src=src)
row("elem-avgpool2-top", "elem", "avgpool2", "top")
row("elem-avgpool2-sub", "elem", "avgpool2", "sub_out")
row("elem-relu-bits", "elem", "relu", "cast")
# the T2I adapter's NHWC -> NCHW copy of its features to all three dtypes, through the tiny adapter; the hint-residual add
# (adapter state into the tiny UNet's last down level, whose tap reads the sum itself) from all three dtypes
row("elem-t2i_copy", "elem", "t2i_copy", "cast")
for src in ("f32", "bf16", "f16"):
    row(f"elem-residual_add-{src}", "elem", "residual_add", "cast", src=src)

# ---- time-embedding path: subnormal 16-bit weights against fp32 activations ------------------------------------------------------------------
for K, N in ((320, 1280), (8, 4)):
    row(f"temb-rowvec-sub_w-{K}x{N}", "temb", "rowvec_linear", "sub_w", shape=dict(B=2, K=K, N=N))
row("temb-timestep-sub_w-320x1280", "temb", "timestep_linear", "sub_w", shape=dict(B=2, K=320, N=1280))

# ---- LoRA / LyCORIS merge: base and the up factor (LyCORIS: base and the term's scale) scaled together to both ends ----------------------
for case in ("conv3x3", "geglu", "two_pairs"):
    for end in ("up", "down"):
        row(f"lora-{end}-{case}", "lora", "repack_lora", "top" if end == "up" else "sub_out", case=case, data="lattice", end=end)
row("lora-up-conv3x3-gauss", "lora", "repack_lora", "top", case="conv3x3", data="gaussian", end="up")
for case in ("loha_conv_r33_r4", "lokr_lowrank_conv_pad_r33", "loha_t_r4", "full_geglu"):
    for end in ("up", "down"):
        row(f"lyco-{end}-{case}", "lora", "repack_delta", "top" if end == "up" else "sub_out", case=case, data="lattice", end=end)
row("lyco-core-sub_w", "lora", "lyco_core", "sub_w", shape=dict(A=5, B=7, C=9, tail=(3, 3)))

BY_ID = {r["id"]: r for r in ROWS}

# ---- the exponents, as derived by tests/range_ref.py:derive_exps (tests/test_range_ref_host.py asserts record == derivation) -----------------
EXPS = {
    'lin-top-cfg1': {'f16': (6, 6), 'bf16': (60, 61)},
    'lin-cancel-cfg1': {'f16': (4, 4)},
    'lin-bias_back-cfg1': {'f16': (4, 4)},
    'lin-rowbias_back-cfg1': {'f16': (4, 4)},
    'lin-res_order-cfg1': {'f16': (3, 4)},
    'lin-sub_act-cfg1': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg1': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg1': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-top-cfg5': {'f16': (6, 7), 'bf16': (60, 61)},
    'lin-cancel-cfg5': {'f16': (4, 4)},
    'lin-bias_back-cfg5': {'f16': (4, 4)},
    'lin-rowbias_back-cfg5': {'f16': (4, 4)},
    'lin-res_order-cfg5': {'f16': (3, 4)},
    'lin-sub_act-cfg5': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg5': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg5': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-top-cfg8': {'f16': (6, 7), 'bf16': (60, 61)},
    'lin-cancel-cfg8': {'f16': (4, 4)},
    'lin-bias_back-cfg8': {'f16': (4, 4)},
    'lin-rowbias_back-cfg8': {'f16': (4, 4)},
    'lin-res_order-cfg8': {'f16': (3, 4)},
    'lin-sub_act-cfg8': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg8': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg8': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-top-cfg22': {'f16': (6, 7), 'bf16': (60, 61)},
    'lin-cancel-cfg22': {'f16': (4, 4)},
    'lin-bias_back-cfg22': {'f16': (4, 4)},
    'lin-rowbias_back-cfg22': {'f16': (4, 4)},
    'lin-res_order-cfg22': {'f16': (3, 4)},
    'lin-sub_act-cfg22': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg22': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg22': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-top-cfg32': {'f16': (6, 7), 'bf16': (60, 61)},
    'lin-cancel-cfg32': {'f16': (4, 4)},
    'lin-bias_back-cfg32': {'f16': (4, 4)},
    'lin-res_order-cfg32': {'f16': (3, 4)},
    'lin-sub_act-cfg32': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg32': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg32': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-top-cfg30': {'f16': (6, 7), 'bf16': (60, 61)},
    'lin-cancel-cfg30': {'f16': (4, 4)},
    'lin-bias_back-cfg30': {'f16': (4, 4)},
    'lin-res_order-cfg30': {'f16': (3, 4)},
    'lin-sub_act-cfg30': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'lin-sub_w-cfg30': {'f16': (14, -24), 'bf16': (14, -24)},
    'lin-sub_out-cfg30': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'lin-sub_act_gauss-cfg1': {'f16': (-18, 17), 'bf16': (-18, 17)},
    'lin-sub_w_gauss-cfg1': {'f16': (13, -14), 'bf16': (13, -14)},
    'lin-sub_act_gauss-cfg5': {'f16': (-18, 17), 'bf16': (-18, 17)},
    'lin-sub_w_gauss-cfg5': {'f16': (13, -14), 'bf16': (13, -14)},
    'lin-sub_act_gauss-cfg8': {'f16': (-18, 17), 'bf16': (-18, 17)},
    'lin-sub_w_gauss-cfg8': {'f16': (13, -14), 'bf16': (13, -14)},
    'lin-sub_act_gauss-cfg22': {'f16': (-18, 17), 'bf16': (-18, 17)},
    'lin-sub_w_gauss-cfg22': {'f16': (13, -14), 'bf16': (13, -14)},
    'lin-sub_act_gauss-cfg32': {'f16': (-18, 17), 'bf16': (-18, 17)},
    'lin-sub_w_gauss-cfg32': {'f16': (13, -14), 'bf16': (13, -14)},
    'lin-sub_act_gauss-cfg30': {'f16': (-18, 18), 'bf16': (-18, 18)},
    'lin-sub_w_gauss-cfg30': {'f16': (13, -14), 'bf16': (13, -14)},
    'splitk-cancel-cfg4': {'f16': (4, 4)},
    'splitk-cancel-cfg5': {'f16': (4, 4)},
    'splitk-cancel-cfg6': {'f16': (4, 4)},
    'splitk-cancel-cfg7': {'f16': (4, 4)},
    'splitk-cancel-cfg8': {'f16': (4, 4)},
    'splitk-cancel-cfg24': {'f16': (4, 4)},
    'splitk-top-cfg8': {'f16': (6, 7), 'bf16': (60, 60)},
    'blocked-sub_w-cfg8': {'f16': (14, -24), 'bf16': (14, -24)},
    'blocked-sub_act-cfg32': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'geglu-top-cfg1': {'f16': (0, 17), 'bf16': (0, 122)},
    'geglu-sub_w-cfg1': {'f16': (15, -24), 'bf16': (15, -24)},
    'geglu-top-cfg6': {'f16': (0, 17), 'bf16': (0, 122)},
    'geglu-sub_w-cfg6': {'f16': (15, -24), 'bf16': (15, -24)},
    'geglu-top-cfg22': {'f16': (0, 17), 'bf16': (0, 122)},
    'geglu-sub_w-cfg22': {'f16': (15, -24), 'bf16': (15, -24)},
    'geglu-top-cfg30': {'f16': (0, 17), 'bf16': (0, 121)},
    'geglu-sub_w-cfg30': {'f16': (15, -24), 'bf16': (15, -24)},
    'lin-transposed-top-cfg1': {'f16': (6, 7), 'bf16': (61, 61)},
    'qkv-top-cfg5': {'f16': (6, 7), 'bf16': (61, 61)},
    'qkv-sub_act-cfg5': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'qkv-top-cfg32': {'f16': (6, 7), 'bf16': (61, 61)},
    'qkv-sub_act-cfg32': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'qkv-top-cfg30': {'f16': (6, 7), 'bf16': (61, 61)},
    'qkv-sub_act-cfg30': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'colstats-linear-cfg8-top': {'f16': (5, 6), 'bf16': (27, 28)},
    'colstats-conv-splitk-top': {'f16': (5, 6), 'bf16': (28, 28)},
    'rowstats-linear-cfg8-top': {'f16': (5, 6), 'bf16': (28, 28)},
    'lin-transposed-sub_act-cfg1': {'f16': (-24, 14), 'bf16': (-24, 14)},
    'qkv-sub_w-cfg5': {'f16': (14, -24), 'bf16': (14, -24)},
    'qkv-sub_w-cfg32': {'f16': (14, -24), 'bf16': (14, -24)},
    'qkv-sub_w-cfg30': {'f16': (14, -24), 'bf16': (14, -24)},
    'geglu-sub_act-cfg1': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'geglu-sub_act-cfg6': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'geglu-sub_act-cfg22': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'geglu-sub_act-cfg30': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'conv-top-cfg1': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg1': {'f16': (4, 4)},
    'conv-bias_back-cfg1': {'f16': (4, 4)},
    'conv-res_order-cfg1': {'f16': (3, 4)},
    'conv-sub_act-cfg1': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg1': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-sub_act_gauss-cfg1': {'f16': (-18, 18), 'bf16': (-18, 18)},
    'conv-top-cfg1z': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg1z': {'f16': (4, 4)},
    'conv-bias_back-cfg1z': {'f16': (4, 4)},
    'conv-res_order-cfg1z': {'f16': (3, 4)},
    'conv-sub_act-cfg1z': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg1z': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-top-cfg5': {'f16': (6, 6), 'bf16': (60, 61)},
    'conv-cancel-cfg5': {'f16': (4, 4)},
    'conv-bias_back-cfg5': {'f16': (4, 4)},
    'conv-res_order-cfg5': {'f16': (3, 4)},
    'conv-sub_act-cfg5': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg5': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-sub_act_gauss-cfg5': {'f16': (-18, 18), 'bf16': (-18, 18)},
    'conv-top-cfg5z': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg5z': {'f16': (4, 4)},
    'conv-bias_back-cfg5z': {'f16': (4, 4)},
    'conv-res_order-cfg5z': {'f16': (3, 4)},
    'conv-sub_act-cfg5z': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg5z': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-top-cfg12': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg12': {'f16': (4, 4)},
    'conv-bias_back-cfg12': {'f16': (4, 5)},
    'conv-res_order-cfg12': {'f16': (4, 4)},
    'conv-sub_act-cfg12': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg12': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-sub_act_gauss-cfg12': {'f16': (-18, 18), 'bf16': (-18, 18)},
    'conv-top-cfg12z': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg12z': {'f16': (4, 4)},
    'conv-bias_back-cfg12z': {'f16': (4, 4)},
    'conv-res_order-cfg12z': {'f16': (3, 4)},
    'conv-sub_act-cfg12z': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg12z': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-top-cfg24': {'f16': (6, 6), 'bf16': (60, 61)},
    'conv-cancel-cfg24': {'f16': (4, 5)},
    'conv-bias_back-cfg24': {'f16': (4, 4)},
    'conv-res_order-cfg24': {'f16': (3, 4)},
    'conv-sub_act-cfg24': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg24': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-sub_act_gauss-cfg24': {'f16': (-18, 18), 'bf16': (-18, 18)},
    'conv-top-cfg24z': {'f16': (6, 7), 'bf16': (60, 61)},
    'conv-cancel-cfg24z': {'f16': (4, 4)},
    'conv-bias_back-cfg24z': {'f16': (4, 4)},
    'conv-res_order-cfg24z': {'f16': (3, 4)},
    'conv-sub_act-cfg24z': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'conv-sub_w-cfg24z': {'f16': (14, -16), 'bf16': (14, -16)},
    'conv-sub_out-cfg1': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'conv-sub_out-cfg5': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'conv-sub_out-cfg12': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'conv-sub_out-cfg24': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'shortcut-two-sources-top': {'f16': (4, 4), 'bf16': (56, 57)},
    'shortcut-one-source-top': {'f16': (4, 4), 'bf16': (56, 57)},
    'convout-top-f32': {'f16': (4, 5), 'bf16': (58, 59)},
    'convout-sub_act-f32': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'convout-top-f32-tiles': {'f16': (4, 5), 'bf16': (58, 59)},
    'convout-sub_act-f32-tiles': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'convout-top-bf16': {'f16': (4, 5), 'bf16': (58, 59)},
    'convout-sub_act-bf16': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'convout-top-bf16-tiles': {'f16': (4, 5), 'bf16': (58, 59)},
    'convout-sub_act-bf16-tiles': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'convout-top-f16': {'f16': (4, 5), 'bf16': (5, 5)},
    'convout-sub_act-f16': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'convout-top-f16-tiles': {'f16': (4, 5), 'bf16': (5, 5)},
    'convout-sub_act-f16-tiles': {'f16': (-16, 14), 'bf16': (-16, 14)},
    'gn-up-2x16x16x384-C1-0': {'f16': (12,), 'bf16': (55,)},
    'gn-down-2x16x16x384-C1-0': {'f16': (-19,), 'bf16': (-54,)},
    'gn-up-2x16x16x384-C1-200': {'f16': (12,), 'bf16': (54,)},
    'gn-down-2x16x16x384-C1-200': {'f16': (-19,), 'bf16': (-54,)},
    'gn-up-2x33x33x320-C1-0': {'f16': (12,), 'bf16': (54,)},
    'gn-down-2x33x33x320-C1-0': {'f16': (-19,), 'bf16': (-54,)},
    'gn-up-2x33x33x960-C1-640': {'f16': (12,), 'bf16': (53,)},
    'gn-down-2x33x33x960-C1-640': {'f16': (-19,), 'bf16': (-54,)},
    'gn-up-2x17x17x2560-C1-1280': {'f16': (12,), 'bf16': (53,)},
    'gn-down-2x17x17x2560-C1-1280': {'f16': (-19,), 'bf16': (-54,)},
    'gn-up-2x17x17x8192-C1-0': {'f16': (12,), 'bf16': (52,)},
    'gn-down-2x17x17x8192-C1-0': {'f16': (-19,), 'bf16': (-54,)},
    'ln-up-7x320': {'f16': (12,), 'bf16': (55,)},
    'ln-down-7x320': {'f16': (-19,), 'bf16': (-54,)},
    'ln-up-3x520': {'f16': (12,), 'bf16': (55,)},
    'ln-down-3x520': {'f16': (-19,), 'bf16': (-54,)},
    'ln-up-33x1280': {'f16': (11,), 'bf16': (54,)},
    'ln-down-33x1280': {'f16': (-19,), 'bf16': (-54,)},
    'gn-colstats-up': {'f16': (12,), 'bf16': (53,)},
    'gn-colstats-down': {'f16': (-19,), 'bf16': (-54,)},
    'ln_linear-up-plain': {'f16': (11,), 'bf16': (55,)},
    'ln_linear-down-plain': {'f16': (-19,), 'bf16': (-54,)},
    'ln_linear-up-geglu': {'f16': (11,), 'bf16': (55,)},
    'ln_linear-down-geglu': {'f16': (-19,), 'bf16': (-54,)},
    'ln_linear-up-parts': {'f16': (11,), 'bf16': (55,)},
    'ln_linear-down-parts': {'f16': (-19,), 'bf16': (-54,)},
    'gn_fold-3x33x33x64-N8-producer1': {'f16': (-15,), 'bf16': (-54,)},
    'gn_fold-2x17x17x1280-N38-producer0': {'f16': (-16,), 'bf16': (-54,)},
    'attn-up-k_attn-D8': {'f16': (14,), 'bf16': (58,)},
    'attn-down-k_attn-D8': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-k_attn-D512': {'f16': (14,), 'bf16': (58,)},
    'attn-down-k_attn-D512': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-auto_plain-D64': {'f16': (14,), 'bf16': (58,)},
    'attn-down-auto_plain-D64': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn2_plain-D40': {'f16': (14,), 'bf16': (58,)},
    'attn-down-attn2_plain-D40': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn2_plain_q64-D32': {'f16': (14,), 'bf16': (58,)},
    'attn-down-attn2_plain_q64-D32': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn2_folded-D40': {'f16': (14,), 'bf16': (58,)},
    'attn-down-attn2_folded-D40': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-prescaled_no_folded_form-D80': {'f16': (14,), 'bf16': (58,)},
    'attn-down-prescaled_no_folded_form-D80': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn3_optimistic-D40': {'f16': (14,), 'bf16': (56,)},
    'attn-down-attn3_optimistic-D40': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn3_checked-D64': {'f16': (14,), 'bf16': (56,)},
    'attn-down-attn3_checked-D64': {'f16': (-18,), 'bf16': (-18,)},
    'attn-up-attn3_short_keys-D80': {'f16': (14,), 'bf16': (58,)},
    'attn-down-attn3_short_keys-D80': {'f16': (-18,), 'bf16': (-18,)},
    'xattn-block-top-Nk77': {'f16': (11,), 'bf16': (55,)},
    'tome-mean3-2x136x64x17': {'f16': (14,), 'bf16': (122,)},
    'tome-mean3-2x137x320x40': {'f16': (13,), 'bf16': (122,)},
    'tome-unmerge-top-2x136x64x17': {'f16': (14,), 'bf16': (124,)},
    'elem-nchw_to_nhwc-f32': {'f16': (), 'bf16': ()},
    'elem-pixel_unshuffle8-f32': {'f16': (), 'bf16': ()},
    'elem-nchw_to_nhwc-bf16': {'f16': (), 'bf16': ()},
    'elem-pixel_unshuffle8-bf16': {'f16': (), 'bf16': ()},
    'elem-nchw_to_nhwc-f16': {'f16': (), 'bf16': ()},
    'elem-pixel_unshuffle8-f16': {'f16': (), 'bf16': ()},
    'elem-avgpool2-top': {'f16': (14,), 'bf16': (122,)},
    'elem-avgpool2-sub': {'f16': (-18,), 'bf16': (-18,)},
    'elem-relu-bits': {'f16': (), 'bf16': ()},
    'elem-t2i_copy': {'f16': (), 'bf16': ()},
    'elem-residual_add-f32': {'f16': (), 'bf16': ()},
    'elem-residual_add-bf16': {'f16': (), 'bf16': ()},
    'elem-residual_add-f16': {'f16': (), 'bf16': ()},
    'temb-rowvec-sub_w-320x1280': {'f16': (-14,), 'bf16': (-14,)},
    'temb-rowvec-sub_w-8x4': {'f16': (-14,), 'bf16': (-14,)},
    'temb-timestep-sub_w-320x1280': {'f16': (-14,), 'bf16': (-14,)},
    'lora-up-conv3x3': {'f16': (14,), 'bf16': (125,)},
    'lora-down-conv3x3': {'f16': (-22,), 'bf16': (-22,)},
    'lora-up-geglu': {'f16': (14,), 'bf16': (125,)},
    'lora-down-geglu': {'f16': (-22,), 'bf16': (-22,)},
    'lora-up-two_pairs': {'f16': (15,), 'bf16': (125,)},
    'lora-down-two_pairs': {'f16': (-21,), 'bf16': (-21,)},
    'lora-up-conv3x3-gauss': {'f16': (17,), 'bf16': (127,)},
    'lyco-up-loha_conv_r33_r4': {'f16': (14,), 'bf16': (116,)},
    'lyco-down-loha_conv_r33_r4': {'f16': (-22,), 'bf16': (-22,)},
    'lyco-up-lokr_lowrank_conv_pad_r33': {'f16': (14,), 'bf16': (117,)},
    'lyco-down-lokr_lowrank_conv_pad_r33': {'f16': (-21,), 'bf16': (-21,)},
    'lyco-up-loha_t_r4': {'f16': (14,), 'bf16': (116,)},
    'lyco-down-loha_t_r4': {'f16': (-22,), 'bf16': (-22,)},
    'lyco-up-full_geglu': {'f16': (14,), 'bf16': (117,)},
    'lyco-down-full_geglu': {'f16': (-22,), 'bf16': (-22,)},
    'lyco-core-sub_w': {'f16': (-18,), 'bf16': (-18,)},
}
