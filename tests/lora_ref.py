"""Reference, data families and error bound for the fused LoRA delta-merge repack (gyre_amd/csrc/kernels_lyco.hip with LORA terms,
gyre_op_repack_lora / gyre_unet_set_weight_lora):

    out[o][ky][kx][ci] = round_storage( scale_p * ( base[so,ci,ky,kx] + sum_j s_j * sum_r up_j[so,r] * down_j[r,ci,ky,kx] ) )

so = o, or the source row of the 16-row value / gate interleave for the GEGLU projection (new row 32p+i = value row 16p+i, new
row 32p+16+i = gate row F+16p+i, F = O/2); pad columns ci >= I are zero.  A *pair* here is ``(up [O, r], down [r, I, KH, KW], s)``
as numpy arrays (down may be [r, I] for a matrix).

The kernel's stated operation order (header of kernels_lyco.hip, LORA terms), restated by ``emulate``:

    acc = base
    for j in argument order:   d = 0;  for r ascending: d = fma(up_j[so,r], down_j[r,...], d)
                               acc = fma(s_j, d, acc)
    out = round_storage(acc * scale_p)

Error bound (``bound``), derived from that order with u32 = 2^-24 (fp32 unit roundoff), A_j = sum_r |up_j down_j| and J pairs:
  * d_j: r_j fused multiply-adds, one rounding each, every partial sum bounded by A_j  ->  |err| <= r_j u32 A_j
  * s_j arrives as an fp32 number (one rounding of the caller's double)                   ->  u32 |s_j| A_j
  * acc after pair j is one rounding of a number bounded by |base| + sum_{i<=j} |s_i| A_i; summed over j = 1..J that is
    u32 ( J |base| + sum_j (J - j + 1) |s_j| A_j )
  * the multiplication by scale_p scales all of this by |scale_p| and rounds once: u32 |ref|;  the storage rounding: u |ref|
  =>  |err| <= u32 ( sum_j |s_j| (r_j + 1 + (J - j + 1)) A_j + J |base| ) |scale_p| + u32 |ref| + u |ref|
For one pair this is the form  2^-24 (|s| (r + 2) A + |base|) |scale_p| + 2^-24 |ref| + u |ref|; with several pairs the
accumulator is rounded once per pair, which is where the (J - j + 1) and the J come from.  The terms above are first order; the
factor (1 + 2^-10) covers the products of roundings (r u32 < 2^-16 for every rank used), and the fp16 flavour gets its
subnormal floor 2^-25.  base and the factors are exact inputs: 16-bit ones convert to fp32 without error and the float64
reference is computed from the same rounded values.

Lattice family (``lattice``): base in {-4..4}/4, up in {0, +-1, +-2} with at most two non-zeros per row, down in {0, +-1}, so
every rank sum is an integer of magnitude <= 4; alpha / r and the user scale are powers of two, so s_j d_j is a multiple of
1/4.  Every merged value has magnitude <= 8 and at most 6 significant bits: exact in fp32 whatever the order, representable
in bf16 and fp16 - the kernel, the float64 reference and the host merge (lora_delta + ``w + d * scale``) must agree bit for bit.
A delta that is itself held in 16 bits cannot show on such values as long as every partial sum is as short as the result, so
the ``cancel`` form adds three pairs whose deltas are +512 d, +d'/4 and -512 d: the merged values are unchanged (same lattice),
fp32 holds every intermediate exactly (<= 14 bits), but a delta accumulated in 16 bits loses the quarter steps next to 512.
"""
import numpy as np
import torch

U32 = 2.0 ** -24


def unit_roundoff(dtype) -> float:
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: U32}[dtype]


def geglu_src_rows(O: int) -> np.ndarray:
    r = np.arange(O)
    p, i = r >> 5, r & 31
    return np.where(i < 16, p * 16 + i, O // 2 + p * 16 + (i - 16))


def _shape(base):
    O, I = base.shape[:2]
    KH, KW = (base.shape[2], base.shape[3]) if base.ndim == 4 else (1, 1)
    return O, I, KH, KW


def _to_dest(v, O, I, KH, KW, I_pad):
    """[O, I * KH * KW] in source (OIHW-flat) column order, rows already in destination order -> [O, KH, KW, I_pad], pad zero."""
    v = v.reshape(O, I, KH * KW).transpose(0, 2, 1)
    out = np.zeros((O, KH * KW, I_pad), dtype=v.dtype)
    out[:, :, :I] = v
    return out.reshape(O, KH, KW, I_pad)


def ref64(base, pairs, I_pad=None, geglu=False, scale_p=1.0) -> np.ndarray:
    """float64 value of the formula, [O][KH][KW][I_pad]."""
    O, I, KH, KW = _shape(base)
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    acc = base.astype(np.float64).reshape(O, -1)[rows]
    for up, down, s in pairs:
        acc = acc + float(s) * (up.astype(np.float64).reshape(O, -1)[rows] @ down.astype(np.float64).reshape(down.shape[0], -1))
    return _to_dest(float(scale_p) * acc, O, I, KH, KW, I_pad)


def bound(base, pairs, I_pad=None, geglu=False, scale_p=1.0, storage=torch.bfloat16) -> np.ndarray:
    """Element-wise tolerance of the module docstring, [O][KH][KW][I_pad] (float64)."""
    O, I, KH, KW = _shape(base)
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    J = len(pairs)
    e = J * np.abs(base.astype(np.float64)).reshape(O, -1)[rows]
    for j, (up, down, s) in enumerate(pairs, 1):
        r = down.shape[0]
        A = np.abs(up.astype(np.float64)).reshape(O, -1)[rows] @ np.abs(down.astype(np.float64)).reshape(r, -1)
        e = e + abs(float(s)) * (r + 1 + (J - j + 1)) * A
    ref = np.abs(ref64(base, pairs, I_pad, geglu, scale_p))
    u = unit_roundoff(storage)
    tol = (U32 * abs(float(scale_p)) * _to_dest(e, O, I, KH, KW, I_pad) + U32 * ref + u * ref) * (1 + 2.0 ** -10)
    return tol + (2.0 ** -25 if storage == torch.float16 else 0.0)


def _fma32(a, b, c):
    """fp32 fused multiply-add on arrays: the product of two fp32 numbers is exact in float64; the float64 sum is rounded once
    more before the fp32 rounding, which can differ from a true fma by a double-rounding case in ~2^-29 of the inputs - never on
    the lattice (everything exact), and far inside the bound elsewhere."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


MISTAKES = ("drop_last_partial_rank", "geglu_up_by_dest_row", "no_alpha_over_r", "delta_in_16_bits", "no_scale_p",
            "scale_p_on_base_only", "nonzero_pad")


def emulate(base, pairs, I_pad=None, geglu=False, scale_p=1.0, mistake=None, alpha_over_r=None, storage=torch.bfloat16):
    """numpy fp32 emulation of the kernel in its stated order -> fp32 [O][KH][KW][I_pad] BEFORE the storage rounding
    (``to_storage`` rounds).  ``mistake``: one of MISTAKES, the seeded errors the lattice comparison has to catch
    (alpha_over_r: per pair, the factor of s_j a "no_alpha_over_r" mistake forgets; storage: the 16-bit type of
    "delta_in_16_bits")."""
    assert mistake is None or mistake in MISTAKES
    O, I, KH, KW = _shape(base)
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    b32 = base.astype(np.float32).reshape(O, -1)[rows]
    acc = b32.copy()
    delta16 = np.zeros_like(acc)
    for j, (up, down, s) in enumerate(pairs):
        r = down.shape[0]
        u32 = up.astype(np.float32).reshape(O, -1)
        u32 = u32 if (mistake == "geglu_up_by_dest_row" and geglu) else u32[rows]
        d32 = down.astype(np.float32).reshape(r, -1)
        nr = r
        if mistake == "drop_last_partial_rank" and r % 32:
            nr = r - 1
        d = np.zeros_like(acc)
        for k in range(nr):                                           # r ascending
            d = _fma32(u32[:, k:k + 1], d32[k:k + 1, :], d)
        sj = np.float32(s)
        if mistake == "no_alpha_over_r":
            sj = np.float32(float(s) / float(alpha_over_r[j]))
        if mistake == "delta_in_16_bits":                             # the delta kept apart from the base, in the storage type
            delta16 = torch.from_numpy(_fma32(sj, d, delta16)).to(storage).to(torch.float32).numpy()
        else:
            acc = _fma32(sj, d, acc)
    if mistake == "delta_in_16_bits":
        acc = (acc + delta16).astype(np.float32)
    if mistake == "no_scale_p":
        out = acc
    elif mistake == "scale_p_on_base_only":
        out = ((b32 * np.float32(scale_p)).astype(np.float32) + (acc - b32)).astype(np.float32)
    else:
        out = (acc * np.float32(scale_p)).astype(np.float32)
    dest = _to_dest(out, O, I, KH, KW, I_pad)
    if mistake == "nonzero_pad" and I_pad > I:
        dest = dest.copy()
        dest[..., I:] = dest[..., :I_pad - I]                         # the gather wrapped instead of masking
    return dest


def to_storage(x: np.ndarray, storage) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(storage)


def _down_shape(r, I, KH, KW, conv):
    return (r, I, KH, KW) if conv else (r, I)


def lattice(O, I, ranks, KH=1, KW=1, conv=None, scales=None, seed=0, cancel=False):
    """(base, pairs, alpha_over_r) of the lattice family; ranks: one rank per pair; scales: per pair (user scale, alpha / r),
    powers of two with s_j >= 1/4 and sum_j 4 |s_j| <= 7 (default: user 1/2, alpha / r 1/2; further pairs user 1, alpha / r 1/4).
    cancel: see the module docstring (ranks then names the rank of the three pairs)."""
    conv = (KH * KW > 1) if conv is None else conv
    g = np.random.default_rng(seed)
    base = g.integers(-4, 5, size=(O, I, KH, KW) if conv else (O, I)).astype(np.float32) / 4
    if cancel:
        r = ranks[0]
        up_big, down_big = _lattice_pair(g, O, I, KH, KW, r, conv)
        up_q, down_q = _lattice_pair(g, O, I, KH, KW, r, conv)
        pairs = [(up_big, down_big, 512.0), (up_q, down_q, 0.25), (-up_big, down_big, 512.0)]
        return base, pairs, [1.0, 0.25, 1.0]
    if scales is None:
        scales = [(0.5, 0.5)] + [(1.0, 0.25)] * (len(ranks) - 1)
    assert sum(4 * abs(a * b) for a, b in scales) <= 7
    pairs = []
    for r, (user, aor) in zip(ranks, scales):
        up, down = _lattice_pair(g, O, I, KH, KW, r, conv)
        pairs.append((up, down, user * aor))
    return base, pairs, [aor for _, aor in scales]


def _lattice_pair(g, O, I, KH, KW, r, conv):
    up = np.zeros((O, r), dtype=np.float32)
    vals = np.array([-2, -1, 1, 2], dtype=np.float32)
    for o in range(O):                       # <= 2 non-zeros per row -> |rank sum| <= 4; the LAST rank is used by half the rows
        if g.random() < 0.5:
            up[o, r - 1] = g.choice(vals)
        up[o, g.integers(0, r)] = g.choice(vals)
    down = g.choice(np.array([-1, 0, 1], dtype=np.float32), size=_down_shape(r, I, KH, KW, conv), p=[0.3, 0.4, 0.3])
    down.reshape(r, -1)[r - 1, ::2] = 1      # ... and the last rank reaches the output
    return (up.reshape(O, r, 1, 1) if conv else up), down


def gaussian(O, I, ranks, KH=1, KW=1, conv=None, seed=0):
    """(base, pairs) with normal entries: base ~ 0.05 N, factors ~ 0.2 N, s_j = 0.8 * (j + 1) / r_j-ish (no structure)."""
    conv = (KH * KW > 1) if conv is None else conv
    g = np.random.default_rng(seed)
    base = (g.standard_normal((O, I, KH, KW) if conv else (O, I)) * 0.05).astype(np.float32)
    pairs = []
    for j, r in enumerate(ranks):
        up = (g.standard_normal((O, r, 1, 1) if conv else (O, r)) * 0.2).astype(np.float32)
        down = (g.standard_normal(_down_shape(r, I, KH, KW, conv)) * 0.2).astype(np.float32)
        pairs.append((up, down, 0.8 * (3.0 + j) / r))
    return base, pairs


def on_lattice(ref) -> bool:
    """magnitude <= 8 and at most 6 significant bits, every element"""
    m, _ = np.frexp(np.asarray(ref, dtype=np.float64))
    return bool(np.abs(ref).max() <= 8 and np.all(m * 64 == np.round(m * 64)))


def worst_ratio(name, got, ref, tol) -> float:
    """max |got - ref| / tol, printed with its place; NaN / inf count as infinite."""
    g = got.double().cpu().numpy().reshape(ref.shape) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.abs(g - ref) == 0, 0.0, np.abs(g - ref) / tol)
    ratio = np.nan_to_num(ratio, nan=np.inf)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"[lora bound] {name}: worst |err| / tol = {ratio[at]:.3g} at {tuple(int(i) for i in at)}: got {g[at]:.8g} ref {ref[at]:.8g} "
          f"tol {tol[at]:.3g}")
    return float(ratio[at])
