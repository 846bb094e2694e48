"""Reference, emulation, data and error bound for the row-major delta merge (gyre_amd/csrc/kernels_lyco.hip k_merge_delta,
gyre_op_merge_delta), the output-typed form of the repack that tests/lyco_ref.py covers:

    out[o][i] = round_out( base[o][i] + sum_j s_j * D_j[o][i] )          base, out [O][I] row-major, out of fp32 / bf16 / fp16

Terms are lyco_ref's ``(fields, user_scale)`` (a LyCORIS file's tensors of one module; s_j = user_scale * file_scale(fields)), the
float64 reference is lyco_ref.ref64 with KH = KW = 1 and no padding, the operands are lowered by lyco_ref.lower.

Operation order (fp32; header of kernels_lyco.hip WITHOUT its final multiplication - change both or neither), restated by ``emulate``:

    P(up, down; row, col):  p = 0;  for q ascending: p = fma(up[row, q], down[q, col], p)
    LORA d = P;   HADA d = P1 * P2 (P1 completely, then P2, one multiplication);   FULL d = diff
    KRON d = w1[o / O2][i / I2] * d2,  d2 = P(up, down; o % O2, i % I2) or the dense W2 there
    acc = base;  for j in argument order: acc = fma(s_j, d_j, acc)
    out = round_out(acc)                      fp32: acc as it stands;  bf16 / fp16: one round to nearest even

Error bound (``bound``): lyco_ref.bound with scale_p = 1 (M_j, e_j as defined there), the storage term replaced by the OUTPUT
type's unit roundoff u_out - 2^-8 for bf16, 2^-11 for fp16, 0 for fp32, whose store rounds nothing:

    |err| <= ( sum_j |s_j| (e_j + u32 M_j + (J - j + 1) u32 M_j) + J u32 |base| + u32 |ref| + u_out |ref| ) (1 + 2^-10)

plus the fp16 subnormal floor 2^-25 for an fp16 output.  (The u32 |ref| term is lyco_ref's rounding of the multiplication by
scale_p; it stays, as that bound is taken over unchanged apart from the storage term.)

``MISTAKES`` are the seeded errors the host test shows the yardsticks to catch: an output rounded to the OTHER 16-bit type first
(or, for fp32, through bf16), the delta summed apart from the base in 16 bits, the last partial 32-rank chunk dropped, and the
Kronecker row split with div and mod swapped.
"""
import numpy as np
import torch

import lyco_ref as LY
from lora_ref import U32, _fma32, on_lattice, unit_roundoff, worst_ratio  # noqa: F401

MISTAKES = ("wrong_out_rounding", "delta_in_16_bits", "drop_last_partial_rank", "kron_div_mod_swapped")
OUT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def ref64(base, terms) -> np.ndarray:
    """float64 value of the formula from the file tensors, [O][I]."""
    O, I = base.shape
    return LY.ref64(base, terms).reshape(O, I)


def _product(up, down, rowidx, colidx, drop_partial=False):
    """P over [len(rowidx), len(colidx)]: q ascending, one fma each (drop_partial: the last, partial 32-rank chunk is lost)."""
    u = up.astype(np.float32)[rowidx]
    d = down.astype(np.float32).reshape(down.shape[0], -1)[:, colidx]
    r = u.shape[1]
    nr = r - r % 32 if drop_partial else r
    p = np.zeros((len(rowidx), len(colidx)), dtype=np.float32)
    for q in range(nr):
        p = _fma32(u[:, q, None], d[None, q], p)
    return p


def round_out(acc: np.ndarray, out_dtype) -> torch.Tensor:
    """fp32 [O][I] -> tensor of out_dtype, torch's round to nearest even (fp32: unchanged)."""
    return torch.from_numpy(np.ascontiguousarray(acc, dtype=np.float32)).to(out_dtype)


def emulate(base, terms, out_dtype=torch.float32, mistake=None, core=LY.core_emulate) -> torch.Tensor:
    """numpy fp32 emulation of k_merge_delta in its stated order -> [O][I] tensor of out_dtype."""
    assert mistake is None or mistake in MISTAKES
    O, I = base.shape
    rows, cols = np.arange(O), np.arange(I)
    drop = mistake == "drop_last_partial_rank"
    acc = base.astype(np.float32).copy()
    other = torch.float16 if out_dtype == torch.bfloat16 else torch.bfloat16
    delta16 = np.zeros_like(acc)
    for fields, user in terms:
        kind, ops, w1 = LY.lower(fields, base.shape, core)
        if kind == "LORA":
            d = _product(*ops[0], rows, cols, drop)
        elif kind == "HADA":
            d = (_product(*ops[0], rows, cols, drop) * _product(*ops[1], rows, cols, drop)).astype(np.float32)
        elif kind == "KRON":
            O1, I1 = w1.shape
            O2, I2 = O // O1, I // I1
            r1, r2 = (rows % O1, rows // O1) if mistake == "kron_div_mod_swapped" else (rows // O2, rows % O2)
            up, down = ops[0]
            d2 = down.astype(np.float32).reshape(O2, I2)[r2][:, cols % I2] if up is None else _product(up, down, r2, cols % I2, drop)
            d = (w1.astype(np.float32)[r1][:, cols // I2] * d2).astype(np.float32)
        else:
            d = ops[0][1].astype(np.float32).reshape(O, I)
        s = np.float32(float(user) * LY.file_scale(fields))
        if mistake == "delta_in_16_bits":                                 # the delta kept apart from the base, in a 16-bit type
            delta16 = torch.from_numpy(_fma32(s, d, delta16)).to(other if out_dtype == torch.float32 else out_dtype).float().numpy()
        else:
            acc = _fma32(s, d, acc)
    if mistake == "delta_in_16_bits":
        acc = (acc + delta16).astype(np.float32)
    if mistake == "wrong_out_rounding":                                   # through the other 16-bit type first (fp32: through bf16)
        acc = torch.from_numpy(acc).to(other).float().numpy()
    return round_out(acc, out_dtype)


def bound(base, terms, out_dtype=torch.float32) -> np.ndarray:
    """Element-wise tolerance of the module docstring, [O][I] (float64)."""
    O, I = base.shape
    J = len(terms)
    e = J * np.abs(base.astype(np.float64))
    for j, (fields, user) in enumerate(terms, 1):
        M, err = LY._term_abs(fields, base.shape)
        e = e + abs(float(user) * LY.file_scale(fields)) * (err + (1 + (J - j + 1)) * M).reshape(O, I)
    ref = np.abs(ref64(base, terms))
    u_out = 0.0 if out_dtype == torch.float32 else unit_roundoff(out_dtype)
    tol = (U32 * e + U32 * ref + u_out * ref) * (1 + 2.0 ** -10)
    return tol + (2.0 ** -25 if out_dtype == torch.float16 else 0.0)


# (name, O, I, [(form, lattice_fields / gaussian_fields keywords, user scale)...]): the smallest matrices that cross each edge of the
# 64 x 64 tile and of the 32-rank chunk - a partial second row tile (72 x 12), exactly one row tile (64 x 24), a partial first tile
# (40 x 20), more than two row tiles and a second, partial column tile (130 x 68); ranks 1, 4, 33 (one chunk + 1) and 130 (four
# chunks + 2); Kronecker factors O2 = 24, I2 = 6 (a 64-row tile crosses o1, a lane's four columns cross i1) with the dense and the
# low-rank right factor, and O2 = 26, I2 = 34 over several tiles; LoHa pairs of different rank; 0, 1, 4 and 8 terms.
K = dict(kron=(3, 2))
CASES = [
    ("zero_terms", 40, 20, []),
    ("zero_terms_tiles", 130, 68, []),
    ("lora_r1", 40, 20, [("lora", dict(rank=1), 1.0)]),
    ("lora_r33", 72, 12, [("lora", dict(rank=33), 1.0)]),
    ("lora_r130", 64, 24, [("lora", dict(rank=130), 1.0)]),
    ("lora_r4_tiles", 130, 68, [("lora", dict(rank=4), 1.0)]),
    ("loha_r33_r4", 72, 12, [("loha", dict(rank=33, rank2=4, scale_rule="scale"), 1.0)]),
    ("loha_r4_r1_tiles", 130, 68, [("loha", dict(rank=4, rank2=1, scale_rule="scale"), 1.0)]),
    ("lokr_dense", 72, 12, [("lokr_dense", K, 1.0)]),
    ("lokr_lowrank_r33", 72, 12, [("lokr_lowrank", dict(rank=33, **K), 1.0)]),
    ("lokr_w1_lowrank", 72, 12, [("lokr_w1_lowrank", dict(rank=4, **K), 1.0)]),
    ("lokr_lowrank_tiles", 130, 68, [("lokr_lowrank", dict(rank=4, kron=(5, 2)), 1.0)]),
    ("full_tiles", 130, 68, [("full", {}, 1.0)]),
    ("four_terms", 72, 12, [("lora", dict(rank=33), 1.0), ("loha", dict(rank=4), 1.0), ("lokr_lowrank", dict(rank=4, **K), 1.0),
                            ("full", {}, 1.0)]),
    # magnitudes <= 1 + 3 * 1/2 + 2 * 1 + 2 * 1 + 1/2 = 7 in multiples of 1/8: six significant bits
    ("eight_terms", 40, 20, [("lora", dict(rank=1), 0.5), ("lora", dict(rank=4), 0.5), ("loha", dict(rank=4), 0.5),
                             ("lokr_dense", dict(kron=(2, 2)), 1.0), ("full", {}, 0.5), ("lora", dict(rank=33), 0.5),
                             ("loha", dict(rank=4, rank2=1, scale_rule="scale"), 0.5), ("lokr_lowrank", dict(rank=4, kron=(2, 2)), 1.0)]),
]
IDS = [c[0] for c in CASES]


def case_terms(case, family="lattice"):
    """(base [O][I], terms) of one CASES entry."""
    name, O, I, forms = case
    seed = sum(map(ord, name))
    make = LY.lattice_fields if family == "lattice" else LY.gaussian_fields
    terms = []
    for j, (form, kw, user) in enumerate(forms):
        kw = dict(kw)
        if family != "lattice":
            kw.pop("scale_rule", None)
        terms.append((make(form, O, I, seed=seed + j, **kw), user))
    base = (LY.lattice_base if family == "lattice" else LY.gaussian_base)(O, I, seed=seed)
    return base, terms


def quantize(a: np.ndarray, dtype) -> np.ndarray:
    """The values a tensor of ``dtype`` holds, as fp32 numpy (references start from what the kernel reads)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()
