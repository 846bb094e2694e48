"""float64 reference, error model and input families of the forward attention checks (tests/test_gpu_attn_fwd.py on the GPU,
tests/test_attn_fwd_ref_host.py on the host).  Nothing here touches a GPU.

Reference.  fwd_ref() evaluates softmax(logits) V in float64 on the exact 16-bit values the kernel is handed: for k_prescaled the
already scaled and rounded K with logits q.k ln 2, otherwise q.k / sqrt(D).  ref = P V, bound = P |V|: the absolute-value form of
what the kernel adds up, so a key that is dropped, doubled or shifted in one row is measured against the size of that row's own
terms, not against the energy of the whole tensor.

Error model.  Every element is held to  |got - ref| <= K_FWD u bound + u |ref| + tiny  (gpu_util.check_bound), u the unit
roundoff of the storage type (2^-8 bf16, 2^-11 fp16).  What a correct kernel rounds to 16 bits (csrc/kernels_attn.hip):

  1. P is packed to the storage type once, right before the P V product (pack_bf16x2 in every family, round to nearest even):
     p_j (1 + d_j), |d_j| <= u.  The numerator sum_j p_j V_j moves by at most u sum_j p_j |V_j|: after the division u * bound.
  2. The row sum.  k_attn, the plain k_attn2 and the folded forms with D % 16 == 0 add up the UNROUNDED fp32 p (`ls += pv` before
     the pack): no 16-bit rounding.  The folded forms with a padded head dim (ONES: D = 40 in k_attn2 FOLD and k_attn3) take the
     row sum inside the matrix core from a V^T row of ones, i.e. from the ROUNDED p: the denominator moves by at most a factor
     (1 +- u), the quotient by u |out| <= u * bound.  So the families differ here; the larger count is kept for all.
  3. The output is rounded once on store: the u |ref| term.

  Everything else (scores, maximum, exp2, rescale by alpha, P V accumulation, the reciprocal) is fp32: together a few 2^-23, under
  one percent of u even for fp16, and is not counted.  K_FWD = 1 (P) + 1 (row sum from rounded p) = 2.

Absolute floor `tiny` (fwd_tiny).  bf16 shares fp32's exponent range: none.  fp16 packs P to a type whose subnormal spacing is
2^-24, so a p below 2^-14 is rounded with an ABSOLUTE error of at most 2^-25 which no relative bound describes.  p is taken relative
to the row's reference: the running maximum (k_attn, plain k_attn2: p <= 1, and the key that holds the maximum has p = 1) or the
reference maximum of the folded forms (first tile's maximum, re-centred when a score exceeds it by TAU: p <= 2^TAU, and the key
that set the reference has p = 2^0 = 1 - the comment at k_attn2, FOLD).  A later rescale multiplies earlier partial sums by
alpha <= 1 and the tile that moved the reference brings a new p = 1, so in the units of the final reference the numerator's absolute
error is at most 2^-25 sum_j |V_j| and the row sum is at least 1: after the division at most 2^-25 sum_j |V_j| per channel.

Logit error.  The score is an fp32 accumulation; one fp32 ulp of a score s (log2 units) is a relative error of about
|s| 2^-24 ln 2 in p.  For the largest scores any case here builds (300 log2 units above the first tile) that is 1.2e-5: 2.5 percent
of fp16's u, 0.3 percent of bf16's, and the key that carries it then holds the whole row, where the error cancels in the quotient.
No case needs a term for it - the fp32 emulation of tests/test_attn_fwd_ref_host.py meets the bound without one on every
family - so none is added: the huge-score cases are held to the same tolerance as all others.
"""
import math

import torch

import gpu_util

K_FWD = 2.0
LOG2E = 1.4426950408889634
# GYRE_ATTN_TAU of csrc/common.h: the folded kernels re-centre a row (and the optimistic pass of k_attn3 is rejected) when a score
# exceeds the row's reference maximum by more than TAU log2 units; 14 for fp16 storage, whose P operand ends at 65504
TAU = {torch.bfloat16: 60.0, torch.float16: 14.0}
PROBE_KEYS = (0, 7, 8, 63, 64, 65)       # + first key of the last tile, Nk - 2, Nk - 1 (probe_positions)


def unit_roundoff(dt):
    return 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11


def q16(t, dt):
    """Round to the storage dtype; float32 holding exactly the 16-bit values."""
    return t.to(dt).float()


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def heads_of(t, heads):
    """[B, N, heads * D] -> float64 [B, heads, N, D]"""
    B, N, C = t.shape
    return t.double().reshape(B, N, heads, C // heads).transpose(1, 2)


def merge(t):
    B, H, N, D = t.shape
    return t.transpose(1, 2).reshape(B, N, H * D)


def log2_scale(D, presc):
    """log2 units of the score per unit of q.k"""
    return 1.0 if presc else LOG2E / math.sqrt(D)


def fwd_ref(q, k, v, heads, presc):
    """(ref, bound) [B, Nq, C] float64.  One sample at a time: the float64 [heads, Nq, Nk] scores of a whole batch need not exist
    at once."""
    D = q.shape[-1] // heads
    beta = math.log(2.0) if presc else 1.0 / math.sqrt(D)
    refs, bnds = [], []
    for b in range(q.shape[0]):
        Q, K, V = (heads_of(t[b:b + 1], heads) for t in (q, k, v))
        P = (Q @ K.transpose(-1, -2) * beta).softmax(-1)
        refs.append(merge(P @ V))
        bnds.append(merge(P @ V.abs()))
    return torch.cat(refs), torch.cat(bnds)


def fwd_tiny(v, dt):
    """fp16: 2^-25 sum_j |V_j| per (sample, channel), broadcast over the query rows (module docstring); bf16: none."""
    if dt == torch.bfloat16:
        return 0.0
    return 2.0 ** -25 * v.double().abs().sum(1, keepdim=True)


def check(name, got, ref, bound, dt, tiny=0.0, k=K_FWD, enforce=True):
    """gpu_util.check_bound for an explicit storage type (the host self-test emulates both flavours in one process)."""
    return gpu_util.check_bound(name, got, ref, bound, k=k, tiny=tiny, dims=("sample", "query", "channel"), hdt=dt, enforce=enforce)


# ---------------------------------------------------------------------------------------------------------------------------
# input families: every builder returns (q, k, v) as float32 [B, N, heads * D] holding exactly the 16-bit values of `dt`;
# k is what the kernel reads (already prescaled and rounded when presc)
# ---------------------------------------------------------------------------------------------------------------------------
def _kscale(D, presc):
    return LOG2E / math.sqrt(D) if presc else 1.0


def family_randn(B, heads, Nq, Nk, D, presc, dt, seed=0):
    C = heads * D
    return (q16(randn(B, Nq, C, seed=seed + 1), dt), q16(randn(B, Nk, C, seed=seed + 2) * _kscale(D, presc), dt),
            q16(randn(B, Nk, C, seed=seed + 3), dt))


def probe_positions(Nk):
    last_tile = (Nk - 1) // 64 * 64
    return sorted({j for j in PROBE_KEYS + (last_tile, Nk - 2, Nk - 1) if 0 <= j < Nk})


def probe_rows(Nq):
    """One query row in every 16-row fragment (the MFMA row block every kernel family works in), at a position that walks through
    the fragment."""
    return [min(16 * f + (5 * f + 3) % 16, Nq - 1) for f in range((Nq + 15) // 16)]


def family_probes(B, heads, Nq, Nk, D, presc, dt, seed=0, keys=None):
    """Key probes: in every 16-row fragment one query row gives >= 0.99 of its softmax mass to one key of `keys` (default
    probe_positions(Nk)); which key walks with the fragment and the head.  All rows of a (sample, head) that probe the same key
    share that key's direction (k_j = a q_row), directions of different keys are orthogonal where the head dim has room.  |V_j|
    of the probed keys is 4x the others', so a dropped, doubled or shifted key moves that row by about its own size.
    Returns (q, k, v, rows, assigned): rows the probing query rows, assigned [heads][len(rows)] the key each one probes."""
    C = heads * D
    keys = probe_positions(Nk) if keys is None else [j for j in keys if 0 <= j < Nk]
    rows = probe_rows(Nq)
    nk = len(keys)
    g = torch.Generator().manual_seed(seed + 11)
    q = randn(B, Nq, C, seed=seed + 1).reshape(B, Nq, heads, D)
    k = (randn(B, Nk, C, seed=seed + 2) * _kscale(D, presc)).reshape(B, Nk, heads, D)
    v = randn(B, Nk, C, seed=seed + 3).reshape(B, Nk, heads, D)
    dirs = torch.randn(B, heads, max(nk, D), D, generator=g)
    if nk <= D:
        dirs = torch.linalg.qr(dirs.transpose(-1, -2).double())[0].transpose(-1, -2).float()     # orthonormal rows
    dirs = dirs[:, :, :nk] / dirs[:, :, :nk].norm(dim=-1, keepdim=True) * math.sqrt(D)           # |d| = sqrt(D), like a randn row
    assigned = [[(f + h) % nk for f in range(len(rows))] for h in range(heads)]
    for h in range(heads):
        for f, r in enumerate(rows):
            q[:, r, h] = dirs[:, h, assigned[h][f]]
    v[:, keys] *= 4.0
    q, v = q16(q.reshape(B, Nq, C), dt), q16(v.reshape(B, Nk, C), dt)
    beta = (math.log(2.0) if presc else 1.0 / math.sqrt(D))
    gap = math.log(99.0 * max(Nk, 2)) + 4.0                  # logit of the probed key over a typical other key (sigma ~ 1)
    for _ in range(6):
        kk = k.clone()
        for i, j in enumerate(keys):
            kk[:, j] = dirs[:, :, i] * (gap / (beta * D))       # logit of the probing rows on key j: beta |d|^2 a = gap
        kr = q16(kk.reshape(B, Nk, C), dt)
        P = (heads_of(q[:, rows], heads) @ heads_of(kr, heads).transpose(-1, -2) * beta).softmax(-1)     # the probing rows only
        mass = min(float(P[:, h, f, keys[assigned[h][f]]].min()) for h in range(heads) for f in range(len(rows)))
        if mass >= 0.99:
            break
        gap *= 1.5                                           # directions that could not be made orthogonal (D < number of probes)
    assert mass >= 0.99, f"probe mass {mass}"
    return q, kr, v, rows, [[keys[i] for i in a] for a in assigned]


def family_ramp(B, heads, Nq, Nk, D, presc, dt, up=True, seed=0, qscale=3.0):
    """Key norms ramp along the sequence: up - the row maximum moves tile after tile; down - the first tile holds it and later p
    are tiny."""
    C = heads * D
    ramp = torch.linspace(0.2, 2.0, Nk) if up else torch.linspace(2.0, 0.02, Nk)
    k = randn(B, Nk, C, seed=seed + 2) * ramp.view(1, Nk, 1) * _kscale(D, presc)
    return q16(randn(B, Nq, C, seed=seed + 1) * qscale, dt), q16(k, dt), q16(randn(B, Nk, C, seed=seed + 3), dt)


def first_tile_excess(q, k, heads, presc):
    """log2 of sum_j 2^(s_j - m0) per row, m0 the maximum over the first 64 keys: what the optimistic pass of k_attn3 compares
    with TAU (its row sum), float64 [B, heads, Nq]."""
    D = q.shape[-1] // heads
    S = heads_of(q, heads) @ heads_of(k, heads).transpose(-1, -2) * log2_scale(D, presc)
    m0 = S[..., :64].max(-1, keepdim=True).values
    return torch.logsumexp((S - m0) * math.log(2.0), -1) / math.log(2.0)


def family_late_key(B, heads, Nq, Nk, D, presc, dt, excess, seed=0, row=5, key=None):
    """randn, and one late key aligned with query `row` of every (sample, head) so that its score lies `excess` log2 units above
    the maximum of that row's first key tile.  That row is twice as long as a randn row, so no other row of the head lines up
    with the planted key by more than it does.  Returns (q, k, v, row)."""
    C = heads * D
    key = Nk - 30 if key is None else key
    assert key >= 64 and row < Nq
    q, k, v = family_randn(B, heads, Nq, Nk, D, presc, dt, seed=seed)
    q[:, row] *= 2.0
    c2 = log2_scale(D, presc)
    Q, K = heads_of(q, heads), heads_of(k, heads)
    qr = Q[:, :, row]                                                            # [B, heads, D]
    m0 = (qr.unsqueeze(-2) @ K[:, :, :64].transpose(-1, -2)).squeeze(-2).max(-1).values * c2
    t = (m0 + excess) / (c2 * (qr * qr).sum(-1))
    k = k.reshape(B, Nk, heads, D).clone()
    k[:, key] = (qr * t.unsqueeze(-1)).float()
    return q, q16(k.reshape(B, Nk, C), dt), v, row


def family_balanced(B, heads, Nq, Nk, D, presc, dt, seed=0):
    """Every row balanced: all keys but one are zero (score 0) and share one V row, the one (in the last tile) scores
    log2(Nk - 1), so the output is half one V row and half the other and moves with any error in the scale or in the row sum.  All
    query rows of a (sample, head) are one vector."""
    assert Nk >= 2
    C = heads * D
    d = q16(randn(B, 1, C, seed=seed + 1), dt)
    q = d.expand(B, Nq, C).contiguous()
    c2 = log2_scale(D, presc)
    dd = d.reshape(B, heads, D).double()
    t = math.log2(Nk - 1) / (c2 * (dd * dd).sum(-1, keepdim=True))
    k = torch.zeros(B, Nk, heads, D)
    k[:, Nk - 2] = (dd * t).float()
    va, vb = randn(B, 1, C, seed=seed + 3), randn(B, 1, C, seed=seed + 4)
    v = va.expand(B, Nk, C).clone()
    v[:, Nk - 2] = vb[:, 0]
    return q, q16(k.reshape(B, Nk, C), dt), q16(v, dt)


def family_uniform(B, heads, Nq, Nk, D, presc, dt, seed=0):
    """All keys of a (sample, head) equal: every output row is the plain mean of V."""
    C = heads * D
    k = (randn(B, 1, C, seed=seed + 2) * _kscale(D, presc)).expand(B, Nk, C).contiguous()
    return q16(randn(B, Nq, C, seed=seed + 1), dt), q16(k, dt), q16(randn(B, Nk, C, seed=seed + 3), dt)


def family_negative(B, heads, Nq, Nk, D, presc, dt, seed=0, depth=10.0):
    """Every score `depth` log2 units BELOW zero (all query rows of a (sample, head) are one vector d, every key is -t d plus a
    little noise): a key that is not there - score 0 from a zero page or a pad column, V = 0 - would outweigh all real keys
    together.  For key counts that are not a multiple of 8 or 64."""
    C = heads * D
    d = q16(randn(B, 1, C, seed=seed + 1), dt)
    q = d.expand(B, Nq, C).contiguous()
    c2 = log2_scale(D, presc)
    dd = d.reshape(B, 1, heads, D).double()
    t = depth / (c2 * (dd * dd).sum(-1, keepdim=True))
    k = (-dd * t).float().expand(B, Nk, heads, D) + 0.05 * _kscale(D, presc) * randn(B, Nk, heads, D, seed=seed + 2)
    return q, q16(k.reshape(B, Nk, C), dt), q16(randn(B, Nk, C, seed=seed + 3), dt)


# ---------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors
# ---------------------------------------------------------------------------------------------------------------------------
def expects_qloop(B, H, Nq, Nk, D):
    """The launch condition of the several-query-blocks-per-workgroup form, mirrored from launch_attn2_t
    (csrc/kernels_attn.hip): head dims 40 / 64 / 80 / 160, 128 query rows per block, qiter = min(nblk B H / 512, 8, nblk) >= 2, and
    every key tile in its own ring slot (PD + 2 slots: 4 up to D = 80, 3 for D = 160).  Returns qiter, 0 when the one-block form runs."""
    if D not in (40, 64, 80, 160):
        return 0
    nblk = (Nq + 127) // 128
    qiter = min(nblk * B * H // 512, 8, nblk)
    slots = (2 if D <= 80 else 1) + 2
    return qiter if (Nk + 63) // 64 <= slots and qiter >= 2 else 0
