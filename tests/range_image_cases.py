"""The case table of tests/test_gpu_range_image.py, as data (no GPU import; tests/test_range_image_ref_host.py builds every row on the
CPU and asserts the conditions its property needs from the float64 reference alone).

The second range family: the kernels of the image models (ControlNet hand-off, RRDBNet, SwinIR, HAT, line-art hinter, HED) that came
after tests/range_cases.py.  Same idea - values at the two ends of the 16-bit storage type's range, the kernel run on the O(1) BASE
problem and on the SCALED one, check 1 (the scaled output is 2^k times the base output bit for bit) and check 2 (the scaled output
against float64 under the kernel's own bound) - and a third kind of row, `specials`: a few +inf, -inf and NaN among O(1) inputs, every
output element in the class (finite / +inf / -inf / NaN) torch's fp32 CPU evaluation of the same operation gives, clean samples with
the bits of a run without the specials.

A row is a dict in the shape of tests/range_cases.py: id, family, op, prop, only, exps (IMAGE_EXPS below, derived by
tests/range_image_ref.py:derive and asserted equal by the host test) and the parameters of its builder.  Shapes are the smallest at
which the kernel still has a tail or a second chunk; the tolerances are the bounds of the per-kernel references (hed_ref, lineart_ref,
hat_ref, swinir_ref, ctrl_ref, rrdb_ref, norm_fwd_ref)."""
from range_cases import PROPS as BASE_PROPS

PROPS = dict(BASE_PROPS)
PROPS.update({
    "epi_back": "alpha (acc + bias) lies beyond 65504, beta1 r1 (and beta2 r2) bring it back: in range only if the chain is narrowed once, at the end",
    "gate_back": "c2 at the top of the range times a small fp32 gate, added to y in fp32 and narrowed once (the geglu-style property)",
    "saturate": "logits scaled until the sigmoid saturates: every output exactly 0 or 1 in the output dtype, never NaN",
    "specials": "+inf, -inf and NaN among O(1) inputs: every output in the class torch's CPU evaluation gives, clean samples bit-identical",
})
F16_ONLY = ("f16",)
BOTH = ("f16", "bf16")
ROWS = []


def row(id, family, op, prop, only=BOTH, **kw):
    assert all(r["id"] != id for r in ROWS), id
    assert prop in PROPS, prop
    ROWS.append(dict(id=id, family=family, op=op, prop=prop, only=tuple(only), **kw))


def _x(t):
    return "x".join(map(str, t))


# ---- HED stage tail: x at the top and in the subnormals, zero bias: the pool is bit-exact, the score 2^k times the base run ------------
for size in ((5, 5), (2, 3)):
    for C in (64, 512):
        for end, prop in (("up", "top"), ("down", "sub_act")):
            row(f"hed_tail-{end}-{_x(size)}-C{C}", "hed", "hed_tail", prop, size=size, C=C, B=3, end=end)

# ---- instance normalisation: x -> 2^k x, eps -> 4^k eps; one chunk, and 15 chunks across the eight slices ------------------------------------
for shape in ((3, 13, 18, 64), (1, 96, 80, 128)):
    for form in ("plain", "pad3", "shuffled_res"):
        if form == "shuffled_res" and shape[1] % 2:
            shape_f = (shape[0], shape[1] + 1, shape[2], shape[3])     # a shuffled source has even sides: 14 x 18
        else:
            shape_f = shape
        for end in ("up", "down"):
            row(f"inorm-{end}-{_x(shape_f)}-{form}", "inorm", "inorm", "invariant", shape=shape_f, form=form, end=end)

# ---- the live-channel LayerNorm --------------------------------------------------------------------------------------------------------------
for C, ld in ((60, 64), (180, 192)):
    for end in ("up", "down"):
        row(f"ln_live-{end}-C{C}-ld{ld}", "norm", "ln_live", "invariant", shape=dict(M=37, C=C), ld=ld, end=end, seed=C)

# ---- channel attention: hat_ref.CAB_CASES[0] and [2] ---------------------------------------------------------------------------------------
for i in (0, 2):
    row(f"chan_pool-top-cab{i}", "cab", "chan_pool", "top", cab=i)
    row(f"scale_add-gate_back-cab{i}", "cab", "scale_add", "gate_back", cab=i)
    row(f"scale_add-sub_out-cab{i}", "cab", "scale_add", "sub_out", cab=i)

# ---- activations: f(65504) is 65504 and not inf; subnormals in, subnormals out ----------------------------------------------------------------
for name, mode, slope in (("gelu", 0, 0.0), ("lrelu0.2", 1, 0.2), ("lrelu0.01", 1, 0.01)):
    for prop in ("top", "sub_out"):
        row(f"swin_act-{name}-{prop}", "act", "swin_act", prop, mode=mode, slope=slope)
for prop in ("top", "sub_out"):
    row(f"silu-{prop}", "act", "silu", prop)

# ---- the RRDB epilogue in place: block form (r1) and rrdb form (r1 and r2) -----------------------------------------------------------------------
for form in ("block", "rrdb"):
    row(f"rdb_epilogue-top-{form}", "epi", "rdb_epilogue", "top", form=form)
    row(f"rdb_epilogue-epi_back-{form}", "epi", "rdb_epilogue", "epi_back", only=F16_ONLY, form=form)

# ---- sigmoid outputs: logits scaled until every one saturates, all three output dtypes ----------------------------------------------------------
for dn in ("f32", "bf16", "f16"):
    row(f"hed_fuse-saturate-{dn}", "sat", "hed_fuse", "saturate", geometry="5x7", out=dn)
    row(f"conv7_out-saturate-{dn}", "sat", "conv7_out", "saturate", shape=(2, 9, 18), out=dn)
row("conv7_out-top-f16", "sat", "conv7_out", "top", shape=(2, 9, 18), out="f16")

# ---- boundary kernels, bit-equal to torch's cast (range_ref.cast_specials) ------------------------------------------------------------------------
for src in ("f32", "bf16", "f16"):
    for r in (1, 2, 4):
        row(f"cast-pixel_unshuffle{r}-{src}", "cast", "pixel_unshuffle", "cast", src=src, r=r)
    row(f"cast-tconv_compose-{src}", "cast", "tconv_compose", "cast", src=src)
    row(f"cast-swin_entry-{src}", "cast", "swin_entry", "cast", src=src)
    row(f"cast-swin_exit-{src}", "cast", "swin_exit", "cast", src=src)
    row(f"cast-hed_entry-{src}", "cast", "hed_entry", "cast", src=src)
    row(f"cast-ctrl_emit-{src}", "cast", "ctrl_emit", "cast", src=src)
# out (f16) + scale f: the product alone is beyond 65504, the sum is not
row("ctrl_emit-res_order", "cast", "ctrl_emit_acc", "res_order", only=F16_ONLY)

# ---- non-finite values: the element-wise and normalisation kernels ------------------------------------------------------------------------------------
# torch: what torch's fp32 CPU evaluation gives where that is not obvious - the row follows it
row("specials-hed_tail", "specials", "hed_tail", "specials", size=(5, 5), C=64, B=3,
    torch="relu and max_pool2d return a NaN operand; relu(-inf) = 0, so a -inf adds nothing to the score and a NaN makes it NaN")
for relu in (0, 1):
    row(f"specials-inorm-relu{relu}", "specials", "inorm", "specials", shape=(3, 13, 18, 64), relu=relu,
        torch="an inf or NaN anywhere in a plane makes the variance NaN: instance_norm returns NaN for the whole plane, relu keeps it")
row("specials-ln_live", "specials", "ln_live", "specials", shape=dict(M=37, C=60), ld=64,
    torch="layer_norm returns NaN for a whole row that holds an inf or a NaN")
for name, mode, slope in (("gelu", 0, 0.0), ("lrelu0.2", 1, 0.2)):
    row(f"specials-swin_act-{name}", "specials", "swin_act", "specials", mode=mode, slope=slope,
        torch="gelu(-inf) = -inf * 0 = NaN on every path.  gelu(+inf): torch's fp32 CPU answer depends on the element count - +inf on its "
              "scalar path (and in float64), NaN on its vectorised path.  The gelu row DEPARTS from the vectorised fp32 path: it is judged "
              "against torch's float64 evaluation, +inf, which is also the limit of the function.  leaky_relu maps +-inf to +-inf")
row("specials-silu", "specials", "silu", "specials", torch="silu(-inf) = -inf * 0 = NaN, silu(+inf) = +inf")
row("specials-cab", "specials", "cab", "specials", cab=0,
    torch="mean over HW of a column with +inf is +inf (with both infinities or a NaN: NaN); relu keeps a NaN hidden unit, which makes every "
          "gate of the sample NaN; +inf hidden units give sigmoid(+-inf) = 1 / 0 or, times a zero weight, NaN")
row("specials-rdb_epilogue", "specials", "rdb_epilogue", "specials", form="rrdb",
    torch="leaky_relu keeps +-inf and NaN; inf + (-inf) from a residual is NaN")
row("specials-ctrl_emit", "specials", "ctrl_emit_acc", "specials", torch="out + scale * f in fp32: inf - inf = NaN")
row("specials-conv7_out", "specials", "conv7_out", "specials", shape=(2, 9, 18),
    torch="a NaN or an inf of both signs under the 7 x 7 window makes the logit NaN and sigmoid(NaN) = NaN; sigmoid(+-inf) = 1 / 0")
row("specials-hed_fuse", "specials", "hed_fuse", "specials", geometry="5x7",
    torch="a NaN / inf score reaches every pixel whose bilinear taps read it (0 * inf = NaN where the tap weight is zero is not formed: "
          "taps outside the map are skipped, inside weights are > 0)")

# ---- window attention: V at the top and in the subnormals (convex); q up and k down by the same power of two, and the reverse (logit_shift) --
PROPS["logit_shift"] = ("q times 2^k to the top of the range and k times 2^-k into the subnormals (and the reverse), both on a lattice that keeps "
                        "them storage values: the output has the base run's bits - the scale is applied to the fp32 dot product")
for op, cases in (("win_attn", ((2, 16, 24, 2, 4), (1, 8, 8, 8, 0))), ("hat_attn", (("sa", 2, 32, 48, 2, 8), ("oca", 1, 16, 16, 6, 0)))):
    for case in cases:
        tag = "-".join(map(str, case))
        for end in ("up", "down"):
            row(f"{op}-convex-{end}-{tag}", "attn", op, "convex", case=case, end=end)
        for d in ("q_up", "k_up"):
            row(f"{op}-logit_shift-{d}-{tag}", "attn", op, "logit_shift", case=case, dir=d)

# ---- the RRDB dense-block convolution: three of its forms on the (th + 1) x (2 tw + 1) image, B = 2 ----------------------------------------------
PROPS["cancel"] = PROPS["cancel"] + " (convolutions: the first channel's taps add 2^15 each, the last channel's take them back)"
for case in ("plain", "rrdb", "act-ups1"):
    row(f"rdb_conv-top-{case}", "rdb", "rdb_conv", "top", case=case)
    row(f"rdb_conv-cancel-{case}", "rdb", "rdb_conv", "cancel", only=F16_ONLY, case=case)
    for prop in ("sub_act", "sub_w", "sub_out"):
        row(f"rdb_conv-{prop}-{case}", "rdb", "rdb_conv", prop, case=case)
row("rdb_conv-epi_back-rrdb", "rdb", "rdb_conv", "epi_back", only=F16_ONLY, case="rrdb")

# ---- the first 7 x 7 convolution of the line-art hinter -------------------------------------------------------------------------------------------
for prop in ("top", "sub_act", "sub_w"):
    row(f"conv7_in-{prop}", "sat", "conv7_in", prop, shape=(2, 9, 18))

# ---- the plain-matrix delta merge: one LoRA and one Kronecker case of merge_delta_ref.CASES, each of the three output dtypes ---------------------
for case in ("lora_r33", "lokr_lowrank_r33"):
    for dn in ("f32", "bf16", "f16"):
        row(f"merge_delta-up-{case}-{dn}", "merge", "merge_delta", "top", case=case, out=dn, end="up")
        row(f"merge_delta-down-{case}-{dn}", "merge", "merge_delta", "sub_out", case=case, out=dn, end="down")

# ---- window attention with a peaked softmax: P is rounded once (the seeded mistake: through the other 16-bit type first) ---------------------------
for op, case in (("win_attn", (2, 16, 24, 2, 4)), ("hat_attn", ("sa", 2, 32, 48, 2, 8)), ("hat_attn", ("oca", 1, 16, 16, 6, 0))):
    row(f"{op}-convex-peaked-{'-'.join(map(str, case))}", "attn", op, "convex", case=case, end="up", peaked=1)

# ---- the four-parity upsampler convolution on config 24, at the smallest shape gyre_debug_ups4_plan accepts ------------------------------------------
row("ups4-top", "ups4", "ups4", "top")
row("ups4-cancel", "ups4", "ups4", "cancel", only=F16_ONLY)
row("ups4-sub_act", "ups4", "ups4", "sub_act")
row("ups4-sub_w", "ups4", "ups4", "sub_w")

BY_ID = {r["id"]: r for r in ROWS}

# ---- the exponents, as derived by tests/range_image_ref.py:derive (tests/test_range_image_ref_host.py asserts record == derivation) ------------
IMAGE_EXPS = {
    'hed_tail-up-5x5-C64': {'f16': (14,), 'bf16': (124,)},
    'hed_tail-down-5x5-C64': {'f16': (-18,), 'bf16': (-18,)},
    'hed_tail-up-5x5-C512': {'f16': (13,), 'bf16': (122,)},
    'hed_tail-down-5x5-C512': {'f16': (-18,), 'bf16': (-18,)},
    'hed_tail-up-2x3-C64': {'f16': (14,), 'bf16': (124,)},
    'hed_tail-down-2x3-C64': {'f16': (-18,), 'bf16': (-18,)},
    'hed_tail-up-2x3-C512': {'f16': (13,), 'bf16': (122,)},
    'hed_tail-down-2x3-C512': {'f16': (-18,), 'bf16': (-18,)},
    'inorm-up-3x13x18x64-plain': {'f16': (8,), 'bf16': (58,)},
    'inorm-down-3x13x18x64-plain': {'f16': (-22,), 'bf16': (-54,)},
    'inorm-up-3x13x18x64-pad3': {'f16': (8,), 'bf16': (58,)},
    'inorm-down-3x13x18x64-pad3': {'f16': (-22,), 'bf16': (-54,)},
    'inorm-up-3x14x18x64-shuffled_res': {'f16': (8,), 'bf16': (58,)},
    'inorm-down-3x14x18x64-shuffled_res': {'f16': (-22,), 'bf16': (-54,)},
    'inorm-up-1x96x80x128-plain': {'f16': (8,), 'bf16': (55,)},
    'inorm-down-1x96x80x128-plain': {'f16': (-22,), 'bf16': (-54,)},
    'inorm-up-1x96x80x128-pad3': {'f16': (8,), 'bf16': (55,)},
    'inorm-down-1x96x80x128-pad3': {'f16': (-22,), 'bf16': (-54,)},
    'inorm-up-1x96x80x128-shuffled_res': {'f16': (8,), 'bf16': (55,)},
    'inorm-down-1x96x80x128-shuffled_res': {'f16': (-22,), 'bf16': (-54,)},
    'ln_live-up-C60-ld64': {'f16': (12,), 'bf16': (56,)},
    'ln_live-down-C60-ld64': {'f16': (-19,), 'bf16': (-54,)},
    'ln_live-up-C180-ld192': {'f16': (12,), 'bf16': (55,)},
    'ln_live-down-C180-ld192': {'f16': (-19,), 'bf16': (-54,)},
    'chan_pool-top-cab0': {'f16': (16,), 'bf16': (117,)},
    'scale_add-gate_back-cab0': {'f16': (13,), 'bf16': (123,)},
    'scale_add-sub_out-cab0': {'f16': (-18,), 'bf16': (-18,)},
    'chan_pool-top-cab2': {'f16': (16,), 'bf16': (120,)},
    'scale_add-gate_back-cab2': {'f16': (13,), 'bf16': (123,)},
    'scale_add-sub_out-cab2': {'f16': (-18,), 'bf16': (-18,)},
    'rdb_epilogue-top-block': {'f16': (13,), 'bf16': (124,)},
    'rdb_epilogue-epi_back-block': {'f16': (7,)},
    'rdb_epilogue-top-rrdb': {'f16': (13,), 'bf16': (123,)},
    'rdb_epilogue-epi_back-rrdb': {'f16': (7,)},
    'hed_fuse-saturate-f32': {'f16': (16,), 'bf16': (16,)},
    'conv7_out-saturate-f32': {'f16': (6, 6), 'bf16': (5, 6)},
    'hed_fuse-saturate-bf16': {'f16': (16,), 'bf16': (16,)},
    'conv7_out-saturate-bf16': {'f16': (6, 6), 'bf16': (5, 6)},
    'hed_fuse-saturate-f16': {'f16': (16,), 'bf16': (16,)},
    'conv7_out-saturate-f16': {'f16': (6, 6), 'bf16': (5, 6)},
    'conv7_out-top-f16': {'f16': (7, 7), 'bf16': (7, 7)},
    'win_attn-convex-peaked-2-16-24-2-4': {'f16': (14,), 'bf16': (124,)},
    'hat_attn-convex-peaked-sa-2-32-48-2-8': {'f16': (14,), 'bf16': (124,)},
    'hat_attn-convex-peaked-oca-1-16-16-6-0': {'f16': (14,), 'bf16': (124,)},
    'ups4-top': {'f16': (7, 7), 'bf16': (61, 61)},
    'ups4-cancel': {'f16': (4, 4)},
    'ups4-sub_act': {'f16': (-24, 12), 'bf16': (-24, 12)},
    'ups4-sub_w': {'f16': (14, -24), 'bf16': (14, -24)},
    'merge_delta-up-lora_r33-f32': {'f16': (117,), 'bf16': (117,)},
    'merge_delta-down-lora_r33-f32': {'f16': (-22,), 'bf16': (-22,)},
    'merge_delta-up-lora_r33-bf16': {'f16': (117,), 'bf16': (117,)},
    'merge_delta-down-lora_r33-bf16': {'f16': (-22,), 'bf16': (-22,)},
    'merge_delta-up-lora_r33-f16': {'f16': (14,), 'bf16': (14,)},
    'merge_delta-down-lora_r33-f16': {'f16': (-22,), 'bf16': (-22,)},
    'merge_delta-up-lokr_lowrank_r33-f32': {'f16': (117,), 'bf16': (117,)},
    'merge_delta-down-lokr_lowrank_r33-f32': {'f16': (-21,), 'bf16': (-21,)},
    'merge_delta-up-lokr_lowrank_r33-bf16': {'f16': (117,), 'bf16': (117,)},
    'merge_delta-down-lokr_lowrank_r33-bf16': {'f16': (-21,), 'bf16': (-21,)},
    'merge_delta-up-lokr_lowrank_r33-f16': {'f16': (14,), 'bf16': (14,)},
    'merge_delta-down-lokr_lowrank_r33-f16': {'f16': (-21,), 'bf16': (-21,)},
    'conv7_in-top': {'f16': (7, 7), 'bf16': (61, 62)},
    'conv7_in-sub_act': {'f16': (-20, 16), 'bf16': (-20, 16)},
    'conv7_in-sub_w': {'f16': (16, -20), 'bf16': (16, -20)},
    'rdb_conv-top-plain': {'f16': (6, 7), 'bf16': (60, 61)},
    'rdb_conv-cancel-plain': {'f16': (5, 6)},
    'rdb_conv-sub_act-plain': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'rdb_conv-sub_w-plain': {'f16': (14, -24), 'bf16': (14, -24)},
    'rdb_conv-sub_out-plain': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'rdb_conv-top-rrdb': {'f16': (6, 7), 'bf16': (61, 62)},
    'rdb_conv-cancel-rrdb': {'f16': (5, 6)},
    'rdb_conv-sub_act-rrdb': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'rdb_conv-sub_w-rrdb': {'f16': (14, -24), 'bf16': (14, -24)},
    'rdb_conv-sub_out-rrdb': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'rdb_conv-top-act-ups1': {'f16': (6, 7), 'bf16': (60, 61)},
    'rdb_conv-cancel-act-ups1': {'f16': (5, 6)},
    'rdb_conv-sub_act-act-ups1': {'f16': (-24, 15), 'bf16': (-24, 15)},
    'rdb_conv-sub_w-act-ups1': {'f16': (14, -24), 'bf16': (14, -24)},
    'rdb_conv-sub_out-act-ups1': {'f16': (-12, -12), 'bf16': (-12, -12)},
    'rdb_conv-epi_back-rrdb': {'f16': (4, 5)},
    'win_attn-convex-up-2-16-24-2-4': {'f16': (14,), 'bf16': (124,)},
    'win_attn-convex-down-2-16-24-2-4': {'f16': (-18,), 'bf16': (-18,)},
    'win_attn-logit_shift-q_up-2-16-24-2-4': {'f16': (18,), 'bf16': (18,)},
    'win_attn-logit_shift-k_up-2-16-24-2-4': {'f16': (18,), 'bf16': (18,)},
    'win_attn-convex-up-1-8-8-8-0': {'f16': (14,), 'bf16': (124,)},
    'win_attn-convex-down-1-8-8-8-0': {'f16': (-18,), 'bf16': (-18,)},
    'win_attn-logit_shift-q_up-1-8-8-8-0': {'f16': (18,), 'bf16': (18,)},
    'win_attn-logit_shift-k_up-1-8-8-8-0': {'f16': (18,), 'bf16': (18,)},
    'hat_attn-convex-up-sa-2-32-48-2-8': {'f16': (14,), 'bf16': (124,)},
    'hat_attn-convex-down-sa-2-32-48-2-8': {'f16': (-18,), 'bf16': (-18,)},
    'hat_attn-logit_shift-q_up-sa-2-32-48-2-8': {'f16': (18,), 'bf16': (18,)},
    'hat_attn-logit_shift-k_up-sa-2-32-48-2-8': {'f16': (18,), 'bf16': (18,)},
    'hat_attn-convex-up-oca-1-16-16-6-0': {'f16': (14,), 'bf16': (124,)},
    'hat_attn-convex-down-oca-1-16-16-6-0': {'f16': (-18,), 'bf16': (-18,)},
    'hat_attn-logit_shift-q_up-oca-1-16-16-6-0': {'f16': (18,), 'bf16': (18,)},
    'hat_attn-logit_shift-k_up-oca-1-16-16-6-0': {'f16': (18,), 'bf16': (18,)},
}
# the single-run rows (activations at the edge itself, casts, specials) have no exponent
for _r in ROWS:
    IMAGE_EXPS.setdefault(_r["id"], {s: () for s in _r["only"]})
