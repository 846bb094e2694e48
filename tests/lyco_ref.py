"""Reference, data families and error bound for the fused LyCORIS delta-merge repack (gyre_amd/csrc/kernels_lyco.hip,
gyre_op_repack_delta / gyre_op_lyco_core / gyre_unet_set_weight_delta), in the manner of lora_ref.py (whose layout helpers,
``on_lattice``, ``worst_ratio`` and ``to_storage`` are reused):

    out[o][ky][kx][ci] = round_storage( scale_p * ( base[so,ci,ky,kx] + sum_j s_j * D_j[so,ci,ky,kx] ) )

A *term* here is ``(fields, user_scale)``: ``fields`` maps the FILE's parameter keys of one module (``hada_w1_a``, ``lokr_w2``,
``lora_mid.weight``, ``diff``, ``alpha``, ``scale`` ...) to numpy arrays, exactly what a LyCORIS file holds; s_j = user_scale *
file_scale(fields).  ``ref64`` evaluates the reference's formulas (gyre/pipeline/lycoris.py:99-228, 267-285) in float64 from those
file tensors.  ``lower`` is what lycoris.upload_factors does to them (core contractions, the transpose of a t form's wa) and
``emulate`` restates the kernels' operation order (header of kernels_lyco.hip) in numpy fp32:

    core:   out[a][c][t] = 0;  for b ascending: out = fma(core[a][b][t], right[b][c], out)
    P(up, down; row, col):  p = 0;  for q ascending: p = fma(up[row, q], down[q, col, t], p)
    LORA d = P;   HADA d = P1 * P2 (P1 completely, then P2, one multiplication);   FULL d = diff
    KRON d = w1[so / O2][ci / I2] * d2,  d2 = P(up, down; so % O2, ci % I2) or the dense W2 there
    acc = base;  for j in argument order: acc = fma(s_j, d_j, acc);   out = round_storage(acc * scale_p)

Error bound (``bound``), first order in u32 = 2^-24, from that order.  For one product with A = sum_q |up| |down| (which bounds
every partial sum): r fused multiply-adds, one rounding each -> |err P| <= r u32 A.  Where down came from the core operator
(r_b fmas, each partial sum bounded by sum_b |core| |right|) its rounding enters as operand error, sum_a |up| r_b u32 sum_b |core|
|right| = r_b u32 A_t with A_t = sum_{a,b} |t| |wa| |wb|, and A <= A_t up to second order: |err P| <= (r_a + r_b) u32 A_t.
    LORA  M = A,         e = err P
    HADA  M = A1 A2,     e = A2 e1 + A1 e2 + u32 A1 A2                 (both operand errors and the rounding of the product)
    KRON  M = Aw (x) A2, e = Aw (x) e2 + ew (x) A2 + u32 Aw (x) A2     (Aw = |w1|, ew = 0 for a dense w1; |w1a| |w1b|, r u32 Aw for a
                                                                        low-rank one, built by the core operator; dense W2: e2 = 0)
    FULL  M = |diff|,    e = 0
Then as in lora_ref: s_j arrives as one fp32 rounding (u32 |s_j| M_j), the accumulator is rounded once per term against a value
bounded by |base| + sum_{i<=j} |s_i| M_i, the multiplication by scale_p rounds once and the storage type once:
    |err| <= ( sum_j |s_j| (e_j + u32 M_j + (J - j + 1) u32 M_j) + J u32 |base| ) |scale_p| + u32 |ref| + u |ref|
times (1 + 2^-10) for the products of roundings (r u32 < 2^-16 for every rank used), plus the fp16 subnormal floor 2^-25.  Operands
are exact inputs: 16-bit ones convert to fp32 without error and the float64 reference starts from the same rounded values.

Lattice family (``lattice``): every factor is a small integer (or a multiple of 1/4 for base and diff) arranged so that every
product is an integer of magnitude <= 4 (<= 2 for a LoHa's second product, a perm-diagonal +-1 core, at most two non-zeros per up
row), file scales are powers of two (LoCon / LoHa 1/4, LoKr 1/8, Full 1), so every merged value is a multiple of 1/8 (1/16 with
scale_p = 1/2) of magnitude <= 8 with at most 6 significant bits: exact in fp32 in any order and representable in bf16 and fp16.
The tests assert that with ``on_lattice`` on the reference values they use.
"""
import numpy as np
import torch

from lora_ref import U32, _fma32, _lattice_pair, _to_dest, geglu_src_rows, on_lattice, to_storage, unit_roundoff, worst_ratio  # noqa: F401

SCALARS = ("alpha", "scale")
MISTAKES = ("hadamard_as_sum", "drop_last_partial_rank_second", "wa_not_transposed", "core_ab_swapped", "kron_div_mod_swapped",
            "kron_col_per_lane", "geglu_row_by_dest", "scale_key_ignored", "lokr_alpha_without_decomposition", "nonzero_pad")


def _shape(base):
    O, I = base.shape[:2]
    KH, KW = (base.shape[2], base.shape[3]) if base.ndim == 4 else (1, 1)
    return O, I, KH, KW


def kind_of(fields) -> str:
    if any(k.startswith("hada") for k in fields):
        return "loha"
    if any(k.startswith("lokr") for k in fields):
        return "lokr"
    return "full" if "diff" in fields else "locon"


def file_scale(fields, mistake=None) -> float:
    """_calc_updown's rule: the scale key if non-zero, else alpha / dim where both exist, else 1."""
    kind = kind_of(fields)
    if "scale" in fields and float(fields["scale"]) != 0 and mistake != "scale_key_ignored":
        return float(fields["scale"])
    alpha = float(fields["alpha"]) if "alpha" in fields else None
    if kind == "locon":
        dims = [fields["lora_down.weight"].shape[0]]
    elif kind == "loha":
        dims = [fields["hada_w1_b"].shape[0], fields["hada_w2_b"].shape[0]]
    elif kind == "lokr":
        dims = [fields[k].shape[0] for k in ("lokr_w1_b", "lokr_w2_b") if k in fields]
        if "lokr_w1_a" not in fields and "lokr_w2_a" not in fields:
            if mistake == "lokr_alpha_without_decomposition" and alpha is not None:
                return alpha
            alpha = None
    else:
        dims = []
    if alpha is None or not dims:
        return 1.0
    assert len(set(dims)) == 1, "two decomposed sides of different rank: the reference's dim is ambiguous"
    return alpha / dims[0]


def _cp64(t, wa, wb):
    return np.einsum("abkl,ao,bi->oikl", t, wa, wb)


def delta64(fields, shape, absolute=False) -> np.ndarray:
    """rebuild_weight in float64 from the file tensors -> [O, I, KK] (absolute: the same sums over absolute values)."""
    O, I = shape[:2]
    KK = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    f = {k: (np.abs(v.astype(np.float64)) if absolute else v.astype(np.float64)) for k, v in fields.items() if k not in SCALARS}
    flat = lambda a: a.reshape(a.shape[0], -1)
    kind = kind_of(fields)
    if kind == "locon":
        up, down = flat(f["lora_up.weight"]), flat(f["lora_down.weight"])
        d = np.einsum("nmkl,in,mj->ijkl", f["lora_mid.weight"], up, down) if "lora_mid.weight" in f else up @ down
    elif kind == "loha":
        p = lambda n: _cp64(f[f"hada_t{n}"], f[f"hada_w{n}_a"], f[f"hada_w{n}_b"]) if f"hada_t{n}" in f else flat(f[f"hada_w{n}_a"]) @ flat(f[f"hada_w{n}_b"])
        d = p(1).reshape(O, -1) * p(2).reshape(O, -1)
    elif kind == "lokr":
        w1 = f["lokr_w1"] if "lokr_w1" in f else f["lokr_w1_a"] @ f["lokr_w1_b"]
        w2 = f["lokr_w2"] if "lokr_w2" in f else _cp64(f["lokr_t2"], f["lokr_w2_a"], f["lokr_w2_b"]) if "lokr_t2" in f else \
            f["lokr_w2_a"] @ flat(f["lokr_w2_b"])
        w2 = w2.reshape(w2.shape[0], -1, KK)
        d = np.einsum("ab,cdk->acbdk", w1, w2)
    else:
        d = f["diff"]
    return d.reshape(O, I, KK)


def ref64(base, terms, I_pad=None, geglu=False, scale_p=1.0) -> np.ndarray:
    """float64 value of the formula from the file tensors, [O][KH][KW][I_pad]."""
    O, I, KH, KW = _shape(base)
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    acc = base.astype(np.float64).reshape(O, I, KH * KW)
    for fields, user in terms:
        acc = acc + float(user) * file_scale(fields) * delta64(fields, base.shape)
    return _to_dest(float(scale_p) * acc[rows].reshape(O, -1), O, I, KH, KW, I_pad)


# ---- the kernels, restated --------------------------------------------------------------------------------------------------
def core64(core, right) -> np.ndarray:
    A, B = core.shape[:2]
    return np.einsum("abt,bc->act", core.astype(np.float64).reshape(A, B, -1), right.astype(np.float64))


def core_emulate(core, right, mistake=None) -> np.ndarray:
    """k_lyco_core: [A, B, T...] x [B, C] -> fp32 [A, C, T], b ascending with fma."""
    A, B = core.shape[:2]
    c = core.astype(np.float32).reshape(A, B, -1)
    if mistake == "core_ab_swapped":
        c = c.transpose(1, 0, 2)
    r = right.astype(np.float32)
    out = np.zeros((A, r.shape[1], c.shape[2]), dtype=np.float32)
    for b in range(B):
        out = _fma32(c[:, b, None, :], r[None, b, :, None], out)
    return out


def lower(fields, shape, core=core_emulate, mistake=None):
    """What lycoris.upload_factors hands to the kernel: (kind, [(up [R, r] | None, down [r, C, KK] | dense [R, C, KK])], w1 | None).
    ``core``: the core operator (this emulation, or the GPU one in the device tests)."""
    KK = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    kw = {"mistake": mistake} if core is core_emulate else {}
    flat = lambda a: a.reshape(a.shape[0], -1)

    def product(wa, wb, t):
        if t is None:
            return flat(wa), wb.reshape(wb.shape[0], -1, KK)
        up = wa.reshape(wa.shape[1], wa.shape[0]) if mistake == "wa_not_transposed" else wa.T       # the file's wa is [r, O]
        return np.ascontiguousarray(up, dtype=np.float32), core(t, wb, **kw)
    kind = kind_of(fields)
    if kind == "locon":
        up, down = fields["lora_up.weight"], fields["lora_down.weight"]
        if "lora_mid.weight" in fields:
            return "LORA", [(flat(up).astype(np.float32), core(fields["lora_mid.weight"], flat(down), **kw))], None
        return "LORA", [product(up, down, None)], None
    if kind == "loha":
        return "HADA", [product(fields[f"hada_w{n}_a"], fields[f"hada_w{n}_b"], fields.get(f"hada_t{n}")) for n in (1, 2)], None
    if kind == "lokr":
        if "lokr_w1" in fields:
            w1 = fields["lokr_w1"].astype(np.float32)
        else:
            w1 = core(fields["lokr_w1_a"], fields["lokr_w1_b"], **kw)[:, :, 0]
        if "lokr_w2" in fields:
            w2 = fields["lokr_w2"]
            return "KRON", [(None, w2.reshape(w2.shape[0], -1, KK))], w1
        return "KRON", [product(fields["lokr_w2_a"], fields["lokr_w2_b"], fields.get("lokr_t2"))], w1
    return "FULL", [(None, fields["diff"].reshape(shape[0], shape[1], KK))], None


def _product(up, down, rowidx, colidx, drop_partial=False):
    """P over [len(rowidx), len(colidx), KK]: q ascending, one fma each."""
    u = up.astype(np.float32)[rowidx]
    d = down.astype(np.float32)[:, colidx, :]
    r = u.shape[1]
    nr = r - r % 32 if drop_partial else r
    p = np.zeros((len(rowidx), len(colidx), d.shape[2]), dtype=np.float32)
    for q in range(nr):
        p = _fma32(u[:, q, None, None], d[None, q], p)
    return p


def emulate(base, terms, I_pad=None, geglu=False, scale_p=1.0, mistake=None, core=core_emulate):
    """numpy fp32 emulation of the kernels in their stated order -> fp32 [O][KH][KW][I_pad] BEFORE the storage rounding
    (``to_storage`` rounds).  ``mistake``: one of MISTAKES, the seeded errors the lattice comparison has to catch."""
    assert mistake is None or mistake in MISTAKES
    O, I, KH, KW = _shape(base)
    KK = KH * KW
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    oprows = np.arange(O) if (mistake == "geglu_row_by_dest" and geglu) else rows
    cols = np.arange(I)
    acc = base.astype(np.float32).reshape(O, I, KK)[rows]
    for fields, user in terms:
        kind, ops, w1 = lower(fields, base.shape, core, mistake)
        if kind == "LORA":
            d = _product(*ops[0], oprows, cols)
        elif kind == "HADA":
            d1 = _product(*ops[0], oprows, cols)
            d2 = _product(*ops[1], oprows, cols, drop_partial=mistake == "drop_last_partial_rank_second")
            d = (d1 + d2) if mistake == "hadamard_as_sum" else (d1 * d2).astype(np.float32)
        elif kind == "KRON":
            O1, I1 = w1.shape
            O2, I2 = O // O1, I // I1
            r1, r2 = oprows // O2, oprows % O2
            if mistake == "kron_div_mod_swapped":
                r1, r2 = oprows % O1, oprows // O1
            up, down = ops[0]
            d2 = down.astype(np.float32)[r2][:, cols % I2, :] if up is None else _product(up, down, r2, cols % I2)
            c1 = (cols // 4 * 4) // I2 if mistake == "kron_col_per_lane" else cols // I2
            d = (w1[r1][:, c1, None] * d2).astype(np.float32)
        else:
            d = ops[0][1].astype(np.float32)[oprows]
        s = np.float32(float(user) * file_scale(fields, mistake))
        acc = _fma32(s, d, acc)
    out = (acc * np.float32(scale_p)).astype(np.float32)
    dest = _to_dest(out.reshape(O, -1), O, I, KH, KW, I_pad)
    if mistake == "nonzero_pad" and I_pad > I:
        dest = dest.copy()
        dest[..., I:] = dest[..., :I_pad - I]                         # the gather wrapped instead of masking
    return dest


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _term_abs(fields, shape):
    """(M, e / u32) of the module docstring, [O, I, KK] in source row order."""
    KK = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    a = {k: np.abs(v.astype(np.float64)) for k, v in fields.items() if k not in SCALARS}
    flat = lambda x: x.reshape(x.shape[0], -1)

    def product(wa, wb, t, R, C):
        if t is None:
            A = (flat(wa) @ flat(wb)).reshape(R, C, KK)
            return A, wb.shape[0] * A
        A = _cp64(t, wa, wb).reshape(R, C, KK)
        return A, (t.shape[0] + t.shape[1]) * A
    kind = kind_of(fields)
    O, I = shape[:2]
    if kind == "locon":
        up, down = flat(a["lora_up.weight"]), flat(a["lora_down.weight"])
        if "lora_mid.weight" in a:
            mid = a["lora_mid.weight"]
            A = np.einsum("nmkl,in,mj->ijkl", mid, up, down).reshape(O, I, KK)
            return A, (mid.shape[0] + mid.shape[1]) * A
        A = (up @ down).reshape(O, I, KK)
        return A, up.shape[1] * A
    if kind == "loha":
        (A1, e1), (A2, e2) = (product(a[f"hada_w{n}_a"], a[f"hada_w{n}_b"], a.get(f"hada_t{n}"), O, I) for n in (1, 2))
        return A1 * A2, A2 * e1 + A1 * e2 + A1 * A2
    if kind == "lokr":
        if "lokr_w1" in a:
            Aw, ew = a["lokr_w1"], 0 * a["lokr_w1"]
        else:
            Aw = a["lokr_w1_a"] @ a["lokr_w1_b"]
            ew = a["lokr_w1_b"].shape[0] * Aw
        O2, I2 = O // Aw.shape[0], I // Aw.shape[1]
        if "lokr_w2" in a:
            A2 = a["lokr_w2"].reshape(O2, I2, KK)
            e2 = 0 * A2
        else:
            A2, e2 = product(a["lokr_w2_a"], a["lokr_w2_b"], a.get("lokr_t2"), O2, I2)
        kron = lambda x, y: np.einsum("ab,cdk->acbdk", x, y).reshape(O, I, KK)
        return kron(Aw, A2), kron(Aw, e2) + kron(ew, A2) + kron(Aw, A2)
    A = a["diff"].reshape(O, I, KK)
    return A, 0 * A


def bound(base, terms, I_pad=None, geglu=False, scale_p=1.0, storage=torch.bfloat16) -> np.ndarray:
    """Element-wise tolerance of the module docstring, [O][KH][KW][I_pad] (float64)."""
    O, I, KH, KW = _shape(base)
    I_pad = I if I_pad is None else I_pad
    rows = geglu_src_rows(O) if geglu else np.arange(O)
    J = len(terms)
    e = J * np.abs(base.astype(np.float64)).reshape(O, I, KH * KW)
    for j, (fields, user) in enumerate(terms, 1):
        M, err = _term_abs(fields, base.shape)
        e = e + abs(float(user) * file_scale(fields)) * (err + (1 + (J - j + 1)) * M)
    ref = np.abs(ref64(base, terms, I_pad, geglu, scale_p))
    u = unit_roundoff(storage)
    tol = (U32 * abs(float(scale_p)) * _to_dest(e[rows].reshape(O, -1), O, I, KH, KW, I_pad) + U32 * ref + u * ref) * (1 + 2.0 ** -10)
    return tol + (2.0 ** -25 if storage == torch.float16 else 0.0)


# ---- data families -----------------------------------------------------------------------------------------------------------
FORMS = ("lora", "locon_mid", "loha", "loha_t", "lokr_dense", "lokr_lowrank", "lokr_w1_lowrank", "lokr_t", "full")


def _perm_core(g, ra, rb, KH, KW):
    """One +-1 per row a and tap, at column (a + 1 + tap) % rb: a core that moves rows around without growing anything."""
    t = np.zeros((ra, rb, KH * KW), dtype=np.float32)
    for a in range(ra):
        for k in range(KH * KW):
            t[a, (a + 1 + k) % rb, k] = g.choice(np.array([-1, 1], dtype=np.float32))
    return t.reshape(ra, rb, KH, KW)


def lattice_fields(form, O, I, KH=1, KW=1, rank=4, rank2=None, seed=0, kron=None, scale_rule="alpha", shrink=1.0):
    """One module's file tensors on the lattice (module docstring).  rank2: the second product's rank of a LoHa (with
    scale_rule "alpha" both ranks must agree, so use "scale" there); kron = (O1, I1); scale_rule: how the file scale is given -
    "alpha" (alpha = dim * scale), "scale" (a scale key that wins over a misleading alpha), "scale0" (a zero scale key next to
    alpha), "none" (neither: 1).  shrink: a power of two on the file scale (model tests: a delta that is small next to the
    weights and still exact)."""
    g = np.random.default_rng(seed)
    conv = KH * KW > 1
    sgn = lambda up: np.sign(up).astype(np.float32)
    f, want, dim = {}, 0.25, rank

    def pair(o, i, r, t_form=False):                                      # (up [o, r], down [r, i, KH, KW] or [r, i])
        up, down = _lattice_pair(g, o, i, 1 if t_form else KH, 1 if t_form else KW, r, conv and not t_form)
        return up.reshape(o, r), down
    if form == "lora":
        up, down = pair(O, I, rank)
        f["lora_up.weight"], f["lora_down.weight"] = (up.reshape(O, rank, 1, 1) if conv else up), down
    elif form == "locon_mid":
        up, down = pair(O, I, rank, True)
        f["lora_up.weight"], f["lora_down.weight"] = up.reshape(O, rank, 1, 1), down.reshape(rank, I, 1, 1)
        f["lora_mid.weight"] = _perm_core(g, rank, rank, KH, KW)
    elif form in ("loha", "loha_t"):
        r2 = rank if rank2 is None else rank2
        for n, r in ((1, rank), (2, r2)):
            up, down = pair(O, I, r, form == "loha_t")
            up = up if n == 1 else sgn(up)                                # |P2| <= 2
            if form == "loha_t":
                f[f"hada_w{n}_a"], f[f"hada_w{n}_b"], f[f"hada_t{n}"] = np.ascontiguousarray(up.T), down, _perm_core(g, r, r, KH, KW)
            else:
                f[f"hada_w{n}_a"], f[f"hada_w{n}_b"] = up, down.reshape(r, -1)
    elif form.startswith("lokr"):
        O1, I1 = kron
        O2, I2 = O // O1, I // I1
        want = 0.125
        vals = np.array([-2, -1, 1, 2], dtype=np.float32)
        if form == "lokr_w1_lowrank":
            a = np.zeros((O1, rank), dtype=np.float32)
            a[np.arange(O1), g.integers(0, rank, O1)] = g.choice(vals, O1)
            f["lokr_w1_a"], f["lokr_w1_b"] = a, g.choice(np.array([-1, 1], dtype=np.float32), (rank, I1))
        else:
            f["lokr_w1"] = g.choice(vals, (O1, I1))
        if form in ("lokr_dense", "lokr_w1_lowrank"):
            f["lokr_w2"] = g.integers(-2, 3, (O2, I2, KH, KW) if conv else (O2, I2)).astype(np.float32)
            dim = rank if form == "lokr_w1_lowrank" else None
        else:
            up, down = pair(O2, I2, rank, form == "lokr_t")
            if form == "lokr_t":
                f["lokr_w2_a"], f["lokr_w2_b"], f["lokr_t2"] = np.ascontiguousarray(up.T), down, _perm_core(g, rank, rank, KH, KW)
            else:
                f["lokr_w2_a"], f["lokr_w2_b"] = up, down.reshape(rank, -1)
    else:
        f["diff"] = g.integers(-4, 5, (O, I, KH, KW) if conv else (O, I)).astype(np.float32) / 4
        want, dim = 1.0, None
    want *= shrink
    if dim is None:                                                       # no dim: alpha must be IGNORED (Full, undecomposed LoKr)
        f["alpha"] = np.float32(0.5)
        if want != 1.0 and scale_rule != "none":
            f["scale"] = np.float32(want)
    elif scale_rule == "alpha":
        f["alpha"] = np.float32(dim * want)
    elif scale_rule == "scale":
        f["alpha"], f["scale"] = np.float32(dim * 2.0), np.float32(want)
    elif scale_rule == "scale0":
        f["alpha"], f["scale"] = np.float32(dim * want), np.float32(0.0)
    else:
        assert scale_rule == "none"
    return f


def gaussian_fields(form, O, I, KH=1, KW=1, rank=4, rank2=None, seed=0, kron=None):
    """The same forms with normal entries (no structure); the file scale is a scale key of about 1 / rank."""
    g = np.random.default_rng(seed)
    conv = KH * KW > 1
    n = lambda *s: (g.standard_normal(s) * 0.3).astype(np.float32)
    tail = (KH, KW) if conv else ()
    f = {"scale": np.float32(0.7 / rank)}
    if form == "lora":
        f["lora_up.weight"], f["lora_down.weight"] = n(O, rank, *((1, 1) if conv else ())), n(rank, I, *tail)
    elif form == "locon_mid":
        f["lora_up.weight"], f["lora_down.weight"], f["lora_mid.weight"] = n(O, rank, 1, 1), n(rank, I, 1, 1), n(rank, rank, KH, KW)
    elif form in ("loha", "loha_t"):
        for k, r in ((1, rank), (2, rank if rank2 is None else rank2)):
            if form == "loha_t":
                f[f"hada_w{k}_a"], f[f"hada_w{k}_b"], f[f"hada_t{k}"] = n(r, O), n(r, I), n(r, r, KH, KW)
            else:
                f[f"hada_w{k}_a"], f[f"hada_w{k}_b"] = n(O, r), n(r, I * KH * KW)
        f["scale"] = np.float32(3.0 / rank)
    elif form.startswith("lokr"):
        O1, I1 = kron
        O2, I2 = O // O1, I // I1
        if form == "lokr_w1_lowrank":
            f["lokr_w1_a"], f["lokr_w1_b"] = n(O1, rank), n(rank, I1)
        else:
            f["lokr_w1"] = n(O1, I1)
        if form in ("lokr_dense", "lokr_w1_lowrank"):
            f["lokr_w2"] = n(O2, I2, *tail)
        elif form == "lokr_t":
            f["lokr_w2_a"], f["lokr_w2_b"], f["lokr_t2"] = n(rank, O2), n(rank, I2), n(rank, rank, KH, KW)
        else:
            f["lokr_w2_a"], f["lokr_w2_b"] = n(O2, rank), n(rank, I2 * KH * KW)
    else:
        f["diff"] = n(O, I, *tail)
        f["scale"] = np.float32(0.4)
    return f


def lattice_base(O, I, KH=1, KW=1, seed=0):
    return np.random.default_rng(1000 + seed).integers(-4, 5, size=(O, I, KH, KW) if KH * KW > 1 else (O, I)).astype(np.float32) / 4


def gaussian_base(O, I, KH=1, KW=1, seed=0):
    return (np.random.default_rng(1000 + seed).standard_normal((O, I, KH, KW) if KH * KW > 1 else (O, I)) * 0.05).astype(np.float32)


# (name, O, I, KH, KW, I_pad, geglu, scale_p, [(form, dict(rank=..., ...))...]): the smallest shapes that reach every edge - a partial
# second row tile and padded K (72 x 12 x 3 x 3, I_pad 16), 40 x 20 with I_pad 24, the GEGLU interleave (64 x 24), ranks 1, 4, 33
# (one full chunk + 1) and 130 (four full chunks + 2), a LoHa of ranks (33, 4), Kronecker factors 72 = 3 * 24 rows (a 64-row tile
# crosses o1) and 12 = 2 * 6 columns (I2 = 6: a factor boundary inside a lane's four columns), dense and low-rank, with and
# without padded K, and a mixed call with scale_p 1/2.
K = dict(kron=(3, 2))
CASES = [
    ("lora_r1", 40, 20, 1, 1, 24, False, 1.0, [("lora", dict(rank=1))]),
    ("lora_conv_r33", 72, 12, 3, 3, 16, False, 1.0, [("lora", dict(rank=33))]),
    ("lora_geglu_r130", 64, 24, 1, 1, 24, True, 1.0, [("lora", dict(rank=130))]),
    ("locon_mid_r4", 72, 12, 3, 3, 16, False, 1.0, [("locon_mid", dict(rank=4))]),
    ("loha_r4", 40, 20, 1, 1, 24, False, 1.0, [("loha", dict(rank=4))]),
    ("loha_conv_r33_r4", 72, 12, 3, 3, 16, False, 1.0, [("loha", dict(rank=33, rank2=4, scale_rule="scale"))]),
    ("loha_geglu_r1", 64, 24, 1, 1, 24, True, 1.0, [("loha", dict(rank=4, rank2=1, scale_rule="scale"))]),
    ("loha_t_r4", 72, 12, 3, 3, 16, False, 1.0, [("loha_t", dict(rank=4))]),
    ("lokr_dense", 72, 12, 1, 1, 12, False, 1.0, [("lokr_dense", K)]),
    ("lokr_dense_conv_pad", 72, 12, 3, 3, 16, False, 1.0, [("lokr_dense", K)]),
    ("lokr_lowrank_r4", 72, 12, 1, 1, 12, False, 1.0, [("lokr_lowrank", dict(rank=4, **K))]),
    ("lokr_lowrank_conv_pad_r33", 72, 12, 3, 3, 16, False, 1.0, [("lokr_lowrank", dict(rank=33, **K))]),
    ("lokr_w1_lowrank", 72, 12, 1, 1, 16, False, 1.0, [("lokr_w1_lowrank", dict(rank=4, **K))]),
    ("lokr_t_r4", 72, 12, 3, 3, 16, False, 1.0, [("lokr_t", dict(rank=4, **K))]),
    ("lokr_geglu", 64, 24, 1, 1, 24, True, 1.0, [("lokr_lowrank", dict(rank=4, kron=(4, 4)))]),
    ("full_conv", 72, 12, 3, 3, 16, False, 1.0, [("full", {})]),
    ("full_geglu", 64, 24, 1, 1, 24, True, 1.0, [("full", {})]),
    ("mixed_half", 72, 12, 3, 3, 16, False, 0.5, [("lora", dict(rank=33)), ("loha", dict(rank=4)), ("lokr_lowrank", dict(rank=4, **K)),
                                                  ("full", {})]),
]


def case_terms(case, family="lattice"):
    """(base, terms) of one CASES entry; every term with user scale 1."""
    name, O, I, KH, KW, I_pad, geglu, scale_p, forms = case
    seed = sum(map(ord, name))
    make = lattice_fields if family == "lattice" else gaussian_fields
    terms = []
    for j, (form, kw) in enumerate(forms):
        kw = dict(kw)
        if family != "lattice":
            kw.pop("scale_rule", None)
        terms.append((make(form, O, I, KH, KW, seed=seed + j, **kw), 1.0))
    base = (lattice_base if family == "lattice" else gaussian_base)(O, I, KH, KW, seed)
    return base, terms
