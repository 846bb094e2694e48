"""The case table of tests/test_gpu_gemm_exact.py, as data (no GPU import; tests/test_gemm_ref_host.py builds every row on the CPU,
checks its lattice conditions and checks the planner's answers for the unforced rows).

A row is a dict:
  id      unique name                     op     linear | linear_t | qkv | conv | conv_nchw | colstats_linear | colstats_conv |
                                                 rowstats | shortcut           (which entry point runs it, gemm_ref.build_case)
  shape   linear forms: M, K, N (N = output columns); conv forms: B, H, W, Cin, Cout
  feats   bias, res, rowbias, rps, geglu, lda_pad / lda2_pad / ldc_pad / ldr_pad (elements beyond the logical width), C1 (second source
          from column / channel C1), out_off (bytes the output pointer is moved off its 16-byte alignment), stride, pad, ups,
          crop (the 2H - 1 x 2W - 1 upsample), wrap, tokens / ldt, dtype (NCHW output: 0 f32, 1 bf16, 2 f16), force_tiles, unit, C1s / C2s
  kind    lattice | wide | gauss | stat   (gemm_ref: which data, which comparison)
  cfg     forced tile config (0: the planner's), splits (forced K slices, 0 / 1: none), abl (tuning bits, e.g. zfill)
  rc      expected status: 0, or the error code a kernel that lacks the form must answer (-6 unsupported, -1 invalid) - `why` says which rule
  plan    unforced rows: the planner's answer the row relies on (subset of gemm_ref.PLAN_FIELDS)
  covers  names of the coverage list (COVERAGE below) this row stands for, checked against the plan query where it can tell

Shapes are the smallest at which the path can still go wrong: an M tail of 33 rows, a K tail of 8 after three full 64-steps, an N tail
of 8 columns; a 3-sample image of 9 x 7 pixels (M = 189: one tile spans three samples, odd sizes).  Where a kernel's own
*_supports rule forces another shape the row says so in `why`."""

FOUR_WAVE = (1, 2, 3)
EIGHT_WAVE = (4, 5, 6, 7, 8)          # (12: convolutions only)
PIPELINED = (20, 21, 22, 23, 24)
AR, SM = 30, 32
GEGLU_TILES = (1, 2, 3, 6, 7, 20, 21, 22, 23, 24, 30)
ZFILL = 0x200                         # GEMM_DBG_CONV_ZERO_PAGE

COVERAGE = ("direct epilogue", "staged epilogue", "uniform tap", "non-uniform tap", "ring depth 2", "ring depth 3", "ring depth 4",
            "split-K", "blocked weights", "zfill 0", "zfill 1", "column statistics", "row statistics", "shortcut fold",
            "transposed output", "fused V^T", "NCHW f32", "NCHW bf16", "NCHW f16", "wrap", "cropped upsample", "row bias", "two sources")

ROWS = []


def row(id, op, kind="lattice", cfg=0, splits=0, abl=0, rc=0, why="", plan=None, covers=(), **kw):
    assert all(r["id"] != id for r in ROWS), id
    shape = {k: kw.pop(k) for k in ("M", "K", "N", "B", "H", "W", "Cin", "Cout") if k in kw}
    ROWS.append(dict(id=id, op=op, kind=kind, cfg=cfg, splits=splits, abl=abl, rc=rc, why=why, plan=plan or {}, covers=tuple(covers),
                     shape=shape, feats=kw))


def kind_of(cfg):
    return "4w" if cfg in FOUR_WAVE else "8w" if cfg in EIGHT_WAVE or cfg == 12 else "4s" if cfg in PIPELINED else "ar" if cfg == AR else "sm"


# ---- linear, forced configs: M tail 33, K tail 8 after three full steps, N tail 8 ---------------------------------------------------
for c in FOUR_WAVE + EIGHT_WAVE:
    row(f"lin-tails-cfg{c}", "linear", cfg=c, M=289, K=200, N=328, bias=1, res=1, covers=("staged epilogue",) if c in EIGHT_WAVE else ())
row("lin-cfg12-refused", "linear", cfg=12, M=289, K=200, N=328, rc=-6, why="the 256x128 tile is a convolution config")
for c in PIPELINED:
    row(f"lin-tails-cfg{c}", "linear", cfg=c, M=289, K=192, N=328, bias=1, res=1, why="gemm4s_supports: K % 64 == 0")
row("lin-tails-cfg32", "linear", cfg=SM, M=289, K=192, N=320, bias=1, res=1, why="gemm_sm_supports: K % 64 == 0, N % 64 == 0")
# the smallest problem: N % 8 != 0 takes the direct epilogue of every kernel that has one
for c in FOUR_WAVE + EIGHT_WAVE:
    row(f"lin-1x8x4-cfg{c}", "linear", cfg=c, M=1, K=8, N=4, bias=1, covers=("direct epilogue",))
for c in PIPELINED + (AR, SM, 12):
    row(f"lin-1x8x4-cfg{c}-refused", "linear", cfg=c, M=1, K=8, N=4, bias=1, rc=-6,
        why="pipelined / small / A-resident kernels have the staged epilogue only (N % 8, K % 64, K = 320); 12 is a convolution config")
# ring depth against step count (8-wave: depth 2 - 4 by tile, pipelined and small kernels: fixed rings)
for c in EIGHT_WAVE + PIPELINED + (SM,):
    for s in range(1, 6):
        row(f"lin-ring-cfg{c}-steps{s}", "linear", cfg=c, M=257, K=64 * s, N=320, bias=1)
# A-resident kernel (config 30), packed weights through gyre_debug_set_ar_workspace
row("lin-ar-289x320x192", "linear", cfg=AR, M=289, K=320, N=192, bias=1, res=1)
row("lin-ar-600x320x576", "linear", cfg=AR, M=600, K=320, N=576, bias=1, res=1)
row("lin-ar-geglu-k640", "linear", cfg=AR, M=289, K=640, N=160, bias=1, geglu=1)
row("lin-ar-k640-plain-refused", "linear", cfg=AR, M=289, K=640, N=192, rc=-6, why="gemm_ar_supports: K = 640 has the GEGLU form only")

# variants on one M / N-tail shape per kernel family
VARIANT_BASE = {1: (289, 200, 328), 5: (289, 200, 328), 8: (289, 200, 328), 22: (289, 192, 328), SM: (289, 192, 320), AR: (289, 320, 192)}
for c, (M, K, N) in VARIANT_BASE.items():
    fam = kind_of(c)
    row(f"lin-plain-cfg{c}", "linear", cfg=c, M=M, K=K, N=N)
    row(f"lin-strides-cfg{c}", "linear", cfg=c, M=M, K=K, N=N, bias=1, res=1, lda_pad=8, ldc_pad=8, ldr_pad=16)
    ok = fam in ("4w", "8w")
    row(f"lin-outoff8-cfg{c}", "linear", cfg=c, M=M, K=K, N=N, bias=1, res=1, out_off=8, rc=0 if ok else -6,
        why="" if ok else "staged-epilogue-only kernels need a 16-byte aligned output", covers=("direct epilogue",) if fam == "8w" else ())
    for C1 in (64, 72):
        ok = fam in ("4w", "8w") or (fam == "sm" and C1 % 64 == 0)
        row(f"lin-two-sources-C1-{C1}-cfg{c}", "linear", cfg=c, M=M, K=K, N=N, bias=1, C1=C1, lda_pad=8, lda2_pad=16, rc=0 if ok else -6,
            why="" if ok else "pipelined / A-resident: one source in linear mode; small kernel: C1 % 64 == 0", covers=("two sources",) if ok else ())
    rb_ok = fam in ("4w", "8w", "4s")
    row(f"lin-rowbias-cfg{c}", "linear", cfg=c, M=M, K=K, N=N, bias=1, rowbias=1, rps=17, rc=0 if rb_ok else -6,
        why="" if rb_ok else "small / A-resident kernels have no row bias", covers=("row bias",) if rb_ok else ())
    row(f"lin-wide-cfg{c}", "linear", kind="wide", cfg=c, M=M, K=K, N=N, bias=1, res=1)
    row(f"lin-gauss-cfg{c}", "linear", kind="gauss", cfg=c, M=M, K=K, N=N, bias=1, res=1)

# transposed output (4-wave configs), pad columns stay untouched
for c in FOUR_WAVE:
    row(f"lin-transposed-cfg{c}", "linear_t", cfg=c, M=154, K=72, N=36, bias=1, tokens=77, ldt=80, covers=("transposed output",))
row("lin-transposed-cfg5-refused", "linear_t", cfg=5, M=154, K=72, N=36, bias=1, tokens=77, ldt=80, rc=-6, why="transposed output needs a 4-wave config")

# fused Q | K | V with V transposed: the smallest C each tile's vt_align admits
for c, C, tok in ((4, 320, 40), (5, 320, 40), (8, 320, 40), (6, 256, 40), (7, 256, 40), (SM, 64, 40), (AR, 320, 64)):
    row(f"qkv-cfg{c}", "qkv", cfg=c, M=2 * tok, K=C, N=3 * C, tokens=tok, ldt=tok + 8, covers=("fused V^T",),
        why="A-resident: tokens % 32 == 0, K = 320" if c == AR else "")
row("qkv-cfg1-refused", "qkv", cfg=1, M=80, K=320, N=960, tokens=40, ldt=48, rc=-6, why="4-wave configs have no transposing epilogue")

# GEGLU on every GEGLU-capable tile: exact 16-row value / gate pairing on the lattice, generic gates with the bound
for c in GEGLU_TILES:
    K = 320 if c == AR else 192
    row(f"geglu-lattice-cfg{c}", "linear", cfg=c, M=289, K=K, N=176 if c != AR else 192, bias=1, geglu=1)
    row(f"geglu-gauss-cfg{c}", "linear", kind="gauss", cfg=c, M=289, K=K, N=176 if c != AR else 192, bias=1, geglu=1)
row("geglu-cfg5-refused", "linear", cfg=5, M=289, K=192, N=176, bias=1, geglu=1, rc=-6, why="GEGLU needs an even fragment count per wave (GemmTile::geglu)")

# ---- 3x3 convolutions, forced configs -------------------------------------------------------------------------------------------------
GEOMS = {"s1": dict(), "s2": dict(stride=2), "s2asym": dict(stride=2, pad=0), "ups": dict(ups=1), "upscrop": dict(ups=1, crop=1),
         "wrap1": dict(wrap=1), "wrap2": dict(wrap=2), "wrap3": dict(wrap=3)}
CONV_CFGS = ((1, 0), (3, 0), (5, 0), (8, 0), (12, 0), (22, 0), (22, ZFILL), (24, 0), (24, ZFILL))
for c, abl in CONV_CFGS:
    fam = kind_of(c)
    tag = f"cfg{c}" + ("z" if abl else "")
    Cout = 136 if c == 12 else 328
    for g, gk in GEOMS.items():
        wrap = gk.get("wrap", 0)
        for Cin in (8, 72, 64, 192):
            if fam == "4s" and Cin % 64:
                continue                      # (refusal asserted once below)
            if wrap and (Cin != 64 or (fam != "4w" and (wrap != 1 or abl))):
                continue                      # wrap: one channel count; the refusal of the other kernels once per config
            imgs = ((3, 9, 7), (1, 17, 17)) if g in ("s1", "upscrop") and Cin in (8, 64) else ((3, 9, 7),)
            for B, H, W in imgs:
                ok = not wrap or fam == "4w"
                cov = ["uniform tap" if Cin % 64 == 0 else "non-uniform tap"] if fam != "4s" else []
                cov += ["wrap"] if wrap and ok else []
                cov += ["cropped upsample"] if g == "upscrop" else []
                cov += [f"zfill {1 if abl else 0}"] if fam == "4s" else []
                row(f"conv-{g}-{B}x{H}x{W}-cin{Cin}-{tag}", "conv", cfg=c, abl=abl, B=B, H=H, W=W, Cin=Cin, Cout=Cout, bias=1,
                    rc=0 if ok else -6, why="" if ok else "circular padding exists in the 4-wave tile configs only", covers=cov, **gk)
    if fam == "4s" and not abl:
        row(f"conv-s1-cin72-{tag}-refused", "conv", cfg=c, B=3, H=9, W=7, Cin=72, Cout=Cout, bias=1, rc=-6, why="gemm4s_supports: Cin % 64 == 0")
    for name, ft in (("rowbias", dict(rowbias=1)), ("res", dict(res=1)), ("rowbias-res", dict(rowbias=1, res=1))):
        row(f"conv-{name}-{tag}", "conv", cfg=c, abl=abl, B=3, H=9, W=7, Cin=64, Cout=Cout, bias=1, covers=("row bias",) if "rowbias" in ft else (), **ft)
    if not abl:
        row(f"conv-two-sources-{tag}", "conv", cfg=c, B=3, H=9, W=7, Cin=128, Cout=Cout, bias=1, C1=64, lda_pad=8, lda2_pad=16, covers=("two sources",))
        row(f"conv-wide-{tag}", "conv", kind="wide", cfg=c, B=3, H=9, W=7, Cin=64, Cout=Cout, bias=1, res=1)
        row(f"conv-gauss-{tag}", "conv", kind="gauss", cfg=c, B=3, H=9, W=7, Cin=64, Cout=Cout, bias=1, res=1)

# ---- split K, forced (cfg | splits << 8): uneven slices - 36 steps in 5 slices ------------------------------------------------------------
for c in (4, 5, 6, 7, 8, 24):
    N = 256 if c in (6, 7) else 320
    row(f"splitk-conv-cfg{c}", "conv", cfg=c, splits=5, B=2, H=8, W=8, Cin=256, Cout=N, bias=1, res=1, covers=("split-K",))
    row(f"splitk-linear-cfg{c}", "linear", cfg=c, splits=5, M=289, K=2304, N=N, bias=1, res=1, rowbias=1, rps=17, covers=("split-K",))
    row(f"splitk-blocked-cfg{c}", "linear", cfg=c, splits=5, M=289, K=2304, N=N, bias=1, wblk=1, plan=dict(w_block=1), covers=("split-K", "blocked weights"))
row("splitk-wide-cfg8", "conv", kind="wide", cfg=8, splits=5, B=2, H=8, W=8, Cin=256, Cout=320, bias=1, res=1)
row("splitk-cfg32-refused", "linear", cfg=SM, splits=5, M=289, K=2304, N=320, rc=-6, why="the small-problem kernel has no split-K form")
row("blocked-conv-cfg8", "conv", cfg=8, B=3, H=9, W=7, Cin=128, Cout=328, bias=1, wblk=1, plan=dict(w_block=1), covers=("blocked weights",))
row("blocked-linear-cfg32", "linear", cfg=SM, M=289, K=1088, N=320, bias=1, wblk=1, plan=dict(w_block=1), covers=("blocked weights",))

# ---- the output convolution (k_conv_out) and its tile-kernel twin ---------------------------------------------------------------------------
for Cout in (4, 1, 3, 16):
    for dt, dn in ((0, "f32"), (1, "bf16"), (2, "f16")):
        for ft in (0, 1):
            row(f"convout-cout{Cout}-{dn}" + ("-tiles" if ft else ""), "conv_nchw", B=2, H=13, W=21, Cin=64, Cout=Cout, bias=1, dtype=dt,
                force_tiles=ft, covers=(f"NCHW {dn}",))
row("convout-wide-f32", "conv_nchw", kind="wide", B=2, H=13, W=21, Cin=64, Cout=4, bias=1, dtype=0, force_tiles=0)
row("convout-wide-bf16", "conv_nchw", kind="wide", B=2, H=13, W=21, Cin=64, Cout=4, bias=1, dtype=1, force_tiles=0)
row("convout-wide-f16-tiles", "conv_nchw", kind="wide", B=2, H=13, W=21, Cin=64, Cout=4, bias=1, dtype=2, force_tiles=1)
row("convout-gauss-f32", "conv_nchw", kind="gauss", B=2, H=13, W=21, Cin=64, Cout=4, bias=1, dtype=0, force_tiles=0)

# ---- fusions a forced config switches off: the smallest shapes the planner sends to each (gyre_debug_gemm_plan) -----------------------------
# >= 160 workgroups of the tile are the planner's condition for every fusing kernel, so M is what it is; the lattice reference is exact
# in fp32 and cheap on the CPU
row("colstats-linear-cfg8", "colstats_linear", kind="stat", M=20480, K=64, N=160, bias=1, res=1, rps=1024, unit=10,
    plan=dict(cfg=8, splits=1, colstat_rows=128), covers=("column statistics",))
row("colstats-linear-cfg4", "colstats_linear", kind="stat", M=65536, K=64, N=320, bias=1, rps=1024, unit=10,
    plan=dict(cfg=4, splits=1, colstat_rows=256), covers=("column statistics",))
row("colstats-conv-cfg8", "colstats_conv", kind="stat", B=5, H=64, W=64, Cin=64, Cout=160, bias=1, res=1, unit=10,
    plan=dict(cfg=8, splits=1, colstat_rows=128, uni=1, nst=4), covers=("column statistics",))
row("colstats-conv-cfg24", "colstats_conv", kind="stat", B=8, H=64, W=64, Cin=192, Cout=640, bias=1, unit=10,
    plan=dict(cfg=24, splits=1, colstat_rows=256, w_block=1), covers=("column statistics",))
row("colstats-conv-splitk", "colstats_conv", kind="stat", B=2, H=8, W=8, Cin=256, Cout=320, bias=1, res=1, unit=10,
    plan=dict(cfg=8, splits=4, colstat_rows=16), covers=("column statistics", "split-K"))
row("rowstats-linear-cfg8", "rowstats", kind="stat", M=20480, K=64, N=160, bias=1, res=1,
    plan=dict(cfg=8, splits=1, rowstat_parts=1), covers=("row statistics",))
row("rowstats-linear-cfg8-4parts", "rowstats", kind="stat", M=20480, K=64, N=640, bias=1,
    plan=dict(cfg=8, splits=1, rowstat_parts=4), covers=("row statistics",))
row("rowstats-linear-cfg4", "rowstats", kind="stat", M=65536, K=64, N=320, bias=1, res=1,
    plan=dict(cfg=4, splits=1, rowstat_parts=1), covers=("row statistics",))
# (the folded shortcut lives in the pipelined 256x320 tile, which the planner takes from 160 workgroups and 20 K steps on)
row("shortcut-two-sources", "shortcut", B=8, H=64, W=64, Cin=128, Cout=640, bias=1, C1s=64, C2s=64,
    plan=dict(cfg=24, splits=1, shortcut_fold=1), covers=("shortcut fold",))
row("shortcut-one-source", "shortcut", B=8, H=64, W=64, Cin=128, Cout=640, bias=1, C1s=128, C2s=0,
    plan=dict(cfg=24, splits=1, shortcut_fold=1), covers=("shortcut fold",))
# unforced rows of the plain operators: what the planner answers for the small shapes above
row("plan-small-linear", "linear", M=289, K=192, N=320, bias=1, plan=dict(cfg=32, splits=1))
row("plan-small-linear-ktail", "linear", M=289, K=200, N=328, bias=1, res=1, plan=dict(splits=1))
row("plan-conv-wrap", "conv", B=3, H=9, W=7, Cin=64, Cout=328, bias=1, wrap=3, plan=dict(splits=1, uni=1), covers=("wrap",))
row("plan-conv-cfg12", "conv", kind="stat", B=16, H=64, W=64, Cin=64, Cout=128, bias=1, plan=dict(cfg=12, splits=1, nst=3, uni=1), covers=("ring depth 3",))

BY_ID = {r["id"]: r for r in ROWS}
