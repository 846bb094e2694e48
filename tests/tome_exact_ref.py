"""float64 reference of the token-merging kernels (csrc/kernels_tome.hip), the lattice keys on which their SELECTION is exact in
every arithmetic, the element tolerance of the merge / unmerge arithmetic and a numpy fp32 emulation of the kernels' summation
order.  TEST INFRASTRUCTURE, shared by tests/test_tome_ref_host.py (CPU) and tests/test_gpu_tome_exact.py (-m gpu).

Selection (the documented tie rules): node_idx = the FIRST maximal b index of every a token's score row, order = a stable
ascending sort of -node_max (equal scores rank by ascending a index), dstlist[k] = node_idx[order[k]] for k < r.

Lattice keys.  Every token has m non-zero entries of +-1, m in {4, 16, 64} (m <= C).  Its squared norm m is a power of 4, so
1 / |k| is 1/2, 1/4 or 1/8 and the normalised entry - even from a 1-ulp rsqrtf - rounds to exactly that in bf16 and in fp16.  A
score is then (an integer of magnitude <= 64) / (4 .. 64): at most 7 significant bits, exact in the fp32 accumulator of the
similarity GEMM in any summation order and exact after its 16-bit rounding.  So oracle/tome_ref.py with and without its bf16
emulation, this float64 selection and the kernels must agree on every index, and ties are exact ties: a tokens are sign-flipped
copies of b tokens (few score levels -> large groups of equal node_max, cut by rank r), and some b tokens are exact duplicates of
earlier ones (tied row maxima), placed where the kernel's three tie sites are (duplicate_pairs()).

Element tolerance of merge_wavg (one output row = the mean of cnt tokens):

    |got - ref| <= u |ref| + (cnt + 2) 2^-24 mean|x|          u = 2^-8 (bf16) / 2^-11 (fp16), mean|x| = sum_i |x_i| / cnt

The kernel adds the cnt values in fp32 (the b token first, then the merged a tokens by ascending rank): cnt - 1 additions, each
with relative error 2^-24 on a partial sum that is at most sum |x_i| -> (cnt - 1) 2^-24 sum|x_i|; 1.0f / cnt and the product add
2 2^-24 |sum|; the division by cnt turns sum|x_i| into mean|x|: (cnt + 1) 2^-24 mean|x| to first order, cnt + 2 with the second-
order terms.  u |ref| is the single 16-bit rounding of the result; u is the exact unit roundoff of the format, so this term is
SHARP (a value just above a power of two reaches it): the host self-test holds the fp32 emulation BEFORE that rounding to half
of the second term, and the rounded emulation to the whole tolerance.  Rows with cnt = 1 (unmerged a tokens, b tokens nothing was
merged into, the trailing token of an odd N) are copies: bit-equal.

Unmerge (adjoint): dx[token] = w dy[row the token went into], w = 1 / cnt of that row: 1.0f / cnt and the product are two fp32
roundings, then one 16-bit rounding:  |got - ref| <= u |ref| + 2 2^-24 |dy|;  bit-equal where w is 1 or a power of two.

Both tolerances carry the format's own absolute floor, half its smallest subnormal (gpu_util.check_bound does the same): an fp16
result below 2^-14 is rounded to a multiple of 2^-24, whatever u |ref| is."""
from __future__ import annotations

import numpy as np
import torch

Tensor = torch.Tensor
U32 = 2.0 ** -24
LATTICE_M = (4, 16, 64)


# ---- selection -------------------------------------------------------------------------------------------------------------------
def select64(key: Tensor, r: int):
    """key [B, N, C] -> (order [B, N//2], node_idx [B, N//2], node_max [B, N//2] float64, r clipped to N//2), all in float64."""
    B, N, C = key.shape
    half = N // 2
    r = max(0, min(int(r), half))
    k = key.double()
    metric = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-300)
    a, b = metric[:, 0:2 * half:2], metric[:, 1:2 * half:2]
    scores = a @ b.transpose(-1, -2)
    node_max = scores.max(dim=-1).values
    cols = torch.arange(half).expand_as(scores)
    node_idx = torch.where(scores == node_max[..., None], cols, torch.full_like(cols, half)).min(dim=-1).values   # FIRST maximum
    order = torch.sort(-node_max, dim=-1, stable=True).indices                                                   # ties: ascending index
    return order, node_idx, node_max, r


def dstlist_of(order: Tensor, node_idx: Tensor, r: int) -> Tensor:
    return torch.gather(node_idx, 1, order[:, :r])


# ---- the merge as a linear map ---------------------------------------------------------------------------------------------------
def merge_rows(order: Tensor, dstlist: Tensor, r: int, N: int):
    """Per sample the rows of the merge map: (row [B, N] = output row every original token goes into, cnt [B, N - r] = token
    count of every output row).  Output rows: the half - r unmerged a tokens in rank order, the half b tokens, the trailing token
    of an odd N."""
    B, half = order.shape
    nu = half - r
    row = torch.zeros(B, N, dtype=torch.long)
    for b in range(B):
        row[b, 2 * order[b, r:]] = torch.arange(nu)
        row[b, 2 * order[b, :r]] = nu + dstlist[b, :r]
        row[b, 1:2 * half:2] = nu + torch.arange(half)
        if N > 2 * half:
            row[b, N - 1] = N - r - 1
    cnt = torch.zeros(B, N - r, dtype=torch.long)
    cnt.scatter_add_(1, row, torch.ones_like(row))
    return row, cnt


def merge_matrix(order: Tensor, dstlist: Tensor, r: int, N: int) -> Tensor:
    """M [B, N - r, N] float64 with merge_wavg(x) = M x (small shapes only: dense)."""
    row, cnt = merge_rows(order, dstlist, r, N)
    B = order.shape[0]
    M = torch.zeros(B, N - r, N, dtype=torch.float64)
    for b in range(B):
        M[b, row[b], torch.arange(N)] = 1.0 / cnt[b, row[b]].double()
    return M


def merge_wavg64(x: Tensor, order: Tensor, node_idx: Tensor, r: int):
    """x [B, N, C] -> (merged [B, N - r, C] float64, cnt [B, N - r], absmean [B, N - r, C] = sum_i |x_i| / cnt)."""
    B, N, C = x.shape
    row, cnt = merge_rows(order, dstlist_of(order, node_idx, r), r, N)
    xd = x.double()
    out = torch.zeros(B, N - r, C, dtype=torch.float64)
    ab = torch.zeros(B, N - r, C, dtype=torch.float64)
    idx = row[:, :, None].expand(-1, -1, C)
    out.scatter_add_(1, idx, xd)
    ab.scatter_add_(1, idx, xd.abs())
    return out / cnt[..., None].double(), cnt, ab / cnt[..., None].double()


def unmerge64(dy: Tensor, order: Tensor, dstlist: Tensor, r: int, N: int):
    """The transpose of merge_matrix applied to dy [B, N - r, C] -> (dx [B, N, C] float64, w [B, N] weight of every token,
    |dy| of the source row [B, N, C])."""
    M = merge_matrix(order, dstlist, r, N)
    dx = M.transpose(1, 2) @ dy.double()
    row, cnt = merge_rows(order, dstlist, r, N)
    w = 1.0 / torch.gather(cnt, 1, row).double()
    src = torch.gather(dy.double().abs(), 1, row[:, :, None].expand(-1, -1, dy.shape[2]))
    return dx, w, src


def _floor(u: float) -> float:
    """Half the smallest subnormal of the 16-bit format: below its smallest normal the rounding error is absolute, not u |ref|
    (fp16: |value| < 2^-14, which a Gaussian value times 1 / cnt reaches; bf16: out of reach)."""
    return 2.0 ** -25 if u == 2.0 ** -11 else 2.0 ** -134


def merge_tolerance(ref: Tensor, cnt: Tensor, absmean: Tensor, u: float) -> Tensor:
    return u * ref.abs() + (cnt[..., None].double() + 2) * U32 * absmean + _floor(u)


def unmerge_tolerance(ref: Tensor, dy_src_abs: Tensor, u: float) -> Tensor:
    return u * ref.abs() + 2 * U32 * dy_src_abs + _floor(u)


# ---- fp32 emulation of the kernels' order (numpy) -----------------------------------------------------------------------------------
def merge_emulate_f32(x: Tensor, order: Tensor, dstlist: Tensor, r: int) -> np.ndarray:
    """k_tome_merge_rows before its 16-bit rounding: acc = b token; acc += merged a tokens by ascending rank; acc *= 1.0f / cnt."""
    B, N, C = x.shape
    half = N // 2
    nu = half - r
    xs = x.float().numpy()
    out = np.zeros((B, N - r, C), np.float32)
    for b in range(B):
        od, dl = order[b].numpy(), dstlist[b].numpy()
        out[b, :nu] = xs[b, 2 * od[r:]]
        acc = xs[b, 1:2 * half:2].copy()
        cnt = np.ones(half, np.int64)
        for k in range(r):
            acc[dl[k]] = acc[dl[k]] + xs[b, 2 * od[k]]
            cnt[dl[k]] += 1
        inv = (np.float32(1.0) / cnt.astype(np.float32)).astype(np.float32)
        out[b, nu:nu + half] = acc * inv[:, None]
        if N > 2 * half:
            out[b, N - r - 1] = xs[b, N - 1]
    return out


def unmerge_emulate_f32(dy: Tensor, order: Tensor, dstlist: Tensor, r: int, N: int) -> np.ndarray:
    row, cnt = merge_rows(order, dstlist, r, N)
    w = (np.float32(1.0) / torch.gather(cnt, 1, row).numpy().astype(np.float32)).astype(np.float32)
    src = torch.gather(dy.float(), 1, row[:, :, None].expand(-1, -1, dy.shape[2])).numpy()
    return src * w[..., None]


# ---- lattice keys -----------------------------------------------------------------------------------------------------------------
def duplicate_pairs(half: int):
    """(first, later) b indices that hold the same token, one pair per tie site of k_tome_rowmax that the row length reaches:
    within one 8-column vector (the in-lane scan), in different lanes (the butterfly), 512 columns apart (the lane's second trip),
    the later copy in the scalar tail of four columns (half % 8 == 4)."""
    pairs = []
    if half >= 8:
        pairs.append((1, 5))
    if half >= 32:
        pairs.append((2, 26))
    if half >= 520:
        pairs.append((7, 519))
    if half % 8 == 4:
        pairs.append((1, 3) if half == 4 else (10, half - 2))
    return pairs


def lattice_keys(B: int, N: int, C: int, seed: int, star: bool = False, r: int = 0) -> Tensor:
    """[B, N, C] float32 keys on the lattice (module docstring).  r > 0: a sample is drawn again (same stream) until a group of
    equal node_max straddles rank r, so that the cut through equal scores is exercised in every sample.  star: every a token is a copy of ONE b token - the later copy of
    the first duplicate pair, so that every row maximum is tied and all a tokens fall to the earlier copy."""
    rng = np.random.RandomState(seed)
    half = N // 2
    ms = [m for m in LATTICE_M if m <= C]

    def token(m):
        t = np.zeros(C)
        t[rng.choice(C, m, replace=False)] = rng.choice([-1.0, 1.0], m)
        return t

    k = np.zeros((B, N, C))
    pairs = duplicate_pairs(half)
    b = 0
    while b < B:
        bt = np.stack([token(ms[-1] if star else ms[rng.randint(len(ms))]) for _ in range(half)])
        for j1, j2 in pairs:
            bt[j2] = bt[j1]
        src = rng.randint(half, size=half)
        slots = rng.permutation(half)
        forced = [j for p in pairs for j in (p[1], p[0], p[1])] + [half - 1, half - 3]      # tied maxima; maxima in the tail columns
        for s, j in zip(slots, forced):
            src[s] = j
        if star:
            src[:] = pairs[0][1]
        at = bt[src].copy()
        for i in range(half):
            nz = np.flatnonzero(at[i])
            flips = rng.randint(0, len(nz) // (8 if star else 4) + 1)
            at[i, rng.choice(nz, flips, replace=False)] *= -1.0
        k[b, 0:2 * half:2], k[b, 1:2 * half:2] = at, bt
        if N > 2 * half:
            k[b, N - 1] = token(ms[0])
        if 0 < r < half:
            ranked = np.sort(((at / np.linalg.norm(at, axis=1, keepdims=True)) @ (bt / np.linalg.norm(bt, axis=1, keepdims=True)).T).max(1))[::-1]
            if ranked[r - 1] != ranked[r]:
                continue
        b += 1
    return torch.from_numpy(k).float()
