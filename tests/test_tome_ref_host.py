"""Host self-test of the token-merging reference (tests/tome_exact_ref.py): the lattice keys are exact (three references agree on
every index), they carry the ties the documented rules decide, the element tolerance is achievable by an fp32 emulation of the
kernels' order, and every seeded mistake is caught by the new criteria.

Which seeded mistakes the OLD criteria let through (test_gpu_kernels.py::test_tome_merge_matches_oracle: >= 97 % agreement of
node_idx on Gaussian keys, rel-L2 <= 4e-3 of the merged rows on even N only; the adjoint only through whole-UNet VJP tests at
rel-L2 5e-2), as this file prints them ([old] lines, Gaussian data with the bf16 score rounding):

    last maximal index            PASSES: node_idx agreement 0.984 (2, 256, 320, 64), 0.985 (2, 137, 320, 40)
    descending-index rank ties    PASSES: node_idx is untouched (agreement 1.0); the ranking was only a 95 % set overlap
    tail columns ignored          passes where N/2 % 8 == 0 (1.0); caught where there is a tail (0.919 at N/2 = 68)
    cnt off by one, in one row    PASSES at the large shapes: rel-L2 2.6e-3 at N = 1096, 1.7e-5 in the star case (1e-2 .. 2e-1 at N <= 137)
    division by r                 caught (rel-L2 0.2 .. 0.6); PASSES in the star case (1.6e-5; r = 256 against cnt = 257)
    trailing token dropped        PASSES: no old case had an odd N (there it is rel-L2 0.11)
    unmerge without the division  no direct criterion: the entry point was never run (rel-L2 0.3 .. 1.1 if it had been)
    unmerge dy[rank]              no direct criterion: the entry point was never run (rel-L2 0.8 .. 0.95)

The fp32 emulation of the merge uses 0.21 .. 0.34 of the (cnt + 2) 2^-24 mean|x| term (0.001 at cnt = 257), of the unmerge 0.16 ..
0.22 of 2 2^-24 |dy|; rounded to 16 bits both reach 0.99 of the whole tolerance, as the sharp u |ref| term must allow."""
import pytest
import torch

import tome_exact_ref as X
from oracle import tome_ref as TR
from tome_cases import GAUSS, LATTICE, LATTICE_SMALL

U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _id(c):
    return "x".join(str(int(v)) for v in c)


_KEYS = {}


def _keys(case):
    if case not in _KEYS:
        B, N, C, r, star = case
        _KEYS[case] = X.lattice_keys(B, N, C, seed=1000 + N, star=star, r=r)
    return _KEYS[case]


# ---- the lattice is exact and tie-bearing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LATTICE, ids=_id)
def test_lattice_selection_is_exact_in_every_arithmetic(case):
    B, N, C, r, star = case
    k = _keys(case)
    nz = (k != 0).sum(-1)
    assert set(nz.unique().tolist()) <= set(X.LATTICE_M) and set(k.unique().tolist()) <= {-1.0, 0.0, 1.0}
    o64, n64, _, r64 = X.select64(k, r)
    for emulate in (True, False):
        for dt in (torch.float32, torch.bfloat16, torch.float16):            # the keys as either flavour stores them
            o, n, reff = TR.bipartite_soft_matching(k.to(dt), r, emulate_bf16=emulate)
            assert reff == r64 and torch.equal(o, o64) and torch.equal(n, n64), (emulate, dt)


@pytest.mark.parametrize("case", LATTICE, ids=_id)
def test_lattice_cases_exercise_the_tie_rules(case):
    B, N, C, r, star = case
    half = N // 2
    k = _keys(case).double()
    metric = k / k.norm(dim=-1, keepdim=True)
    scores = metric[:, 0:2 * half:2] @ metric[:, 1:2 * half:2].transpose(1, 2)
    order, node_idx, node_max, reff = X.select64(_keys(case), r)
    tied = (scores == node_max[..., None]).sum(-1) > 1
    levels = [len(node_max[b].unique()) for b in range(B)]
    print(f"[lattice] {_id(case)}: rows with a tied maximum {float(tied.double().mean()):.2f}, node_max levels per sample {levels}")
    for b in range(B):
        assert int(tied[b].sum()) >= 1
        ranked = node_max[b, order[b]]
        if reff < half:            # a group of equal node_max straddles the cut at rank r
            assert ranked[reff - 1] == ranked[reff]
        else:                      # r = N/2: nothing is cut; the ranking of equal scores still decides the accumulation order
            assert len(ranked.unique()) < half
    for i, (j1, j2) in enumerate(X.duplicate_pairs(half)):                   # every placed duplicate is some row's tied maximum
        assert torch.equal(k[:, 2 * j1 + 1], k[:, 2 * j2 + 1])
        if star and i:                                                       # (the star's a tokens all copy the first pair)
            continue
        assert bool(((scores[:, :, j1] == node_max) & (scores[:, :, j2] == node_max)).any())
    if star:
        _, cnt = X.merge_rows(order, X.dstlist_of(order, node_idx, reff), reff, N)
        assert int(cnt.max()) == half + 1 == 257


def test_r_above_half_clamps():
    k = _keys(LATTICE[1])
    assert X.select64(k, 10 ** 6)[3] == k.shape[1] // 2 and X.select64(k, -3)[3] == 0


# ---- the merge map and its transpose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LATTICE_SMALL, ids=_id)
def test_merge_matrix_is_merge_wavg_and_agrees_with_the_oracle(case):
    B, N, C, r, star = case
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, N, C, generator=g)
    order, node_idx, _, reff = X.select64(_keys(case), r)
    ref, cnt, absmean = X.merge_wavg64(x, order, node_idx, reff)
    M = X.merge_matrix(order, X.dstlist_of(order, node_idx, reff), reff, N)
    assert float((M @ x.double() - ref).abs().max()) < 1e-13
    assert float((TR.merge_wavg(x, order, node_idx, reff).double() - ref).abs().max()) < 1e-5
    assert torch.equal(cnt.sum(-1), torch.full((B,), N)) and float((M.sum(-1) - 1).abs().max()) < 1e-15
    dy = torch.randn(B, N - reff, C, generator=g)
    dx, w, _ = X.unmerge64(dy, order, X.dstlist_of(order, node_idx, reff), reff, N)
    # <M x, dy> = <x, M^T dy>
    assert abs(float((ref * dy.double()).sum() - (x.double() * dx).sum())) < 1e-9 * float(x.abs().sum())


# ---- the tolerance is achievable ----------------------------------------------------------------------------------------------------
def _gauss(case):
    B, N, C, r = case
    g = torch.Generator().manual_seed(200 + N)
    return torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g)


@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", GAUSS + [c[:4] for c in LATTICE_SMALL if c[4]], ids=_id)
def test_fp32_emulation_of_the_kernel_order_stays_under_half_the_tolerance(case, hdt):
    B, N, C, r = case
    star = case in [c[:4] for c in LATTICE if c[4]]
    k, v = _gauss(case)
    k, v = k.to(hdt).float(), v.to(hdt).float()
    order, node_idx, _, reff = X.select64(_keys(case + (True,)) if star else k, r)
    dl = X.dstlist_of(order, node_idx, reff)
    ref, cnt, absmean = X.merge_wavg64(v, order, node_idx, reff)
    emu = torch.from_numpy(X.merge_emulate_f32(v, order, dl, reff))
    fp32_term = (cnt[..., None].double() + 2) * X.U32 * absmean
    worst32 = float(((emu.double() - ref).abs() / fp32_term).max())
    tol = X.merge_tolerance(ref, cnt, absmean, U16[hdt])
    worst = float(((emu.to(hdt).double() - ref).abs() / tol).max())
    print(f"[emul] merge {_id(case)} {hdt}: fp32 part {worst32:.3f} of (cnt + 2) 2^-24 mean|x|, rounded {worst:.3f} of the tolerance, max cnt {int(cnt.max())}")
    assert worst32 <= 0.5 and worst <= 1.0
    copies = (cnt == 1)
    assert torch.equal(emu.to(hdt)[copies], ref.to(hdt)[copies])
    dy = torch.randn(B, N - reff, C, generator=torch.Generator().manual_seed(N)).to(hdt).float()
    if N <= 1100:
        dx, w, src = X.unmerge64(dy, order, dl, reff, N)
        emu = torch.from_numpy(X.unmerge_emulate_f32(dy, order, dl, reff, N))
        worst32 = float(((emu.double() - dx).abs() / (2 * X.U32 * src).clamp_min(1e-300)).max())
        worst = float(((emu.to(hdt).double() - dx).abs() / X.unmerge_tolerance(dx, src, U16[hdt]).clamp_min(1e-300)).max())
        print(f"[emul] unmerge {_id(case)} {hdt}: fp32 part {worst32:.3f} of 2 2^-24 |dy|, rounded {worst:.3f} of the tolerance")
        assert worst32 <= 0.5 and worst <= 1.0
        pow2 = (torch.log2(w) == torch.log2(w).round())
        assert torch.equal(emu.to(hdt)[pow2], dx.to(hdt)[pow2])


# ---- seeded mistakes ------------------------------------------------------------------------------------------------------------------
def _scores(key, emulate_bf16=False):
    half = key.shape[1] // 2
    k = key.double()
    metric = k / k.norm(dim=-1, keepdim=True)
    if emulate_bf16:
        metric = metric.to(torch.bfloat16).double()
    s = metric[:, 0:2 * half:2] @ metric[:, 1:2 * half:2].transpose(1, 2)
    return s.to(torch.bfloat16).double() if emulate_bf16 else s


def _select(scores, mistake=None):
    """The reference selection from a score matrix, with one seeded mistake."""
    half = scores.shape[-1]
    s = scores.clone()
    if mistake == "tail columns ignored" and half % 8:
        s[..., half - half % 8:] = -3.0e38
    node_max = s.max(-1).values
    cols = torch.arange(half).expand_as(s)
    if mistake == "last maximal index":
        node_idx = torch.where(s == node_max[..., None], cols, torch.full_like(cols, -1)).max(-1).values
    else:
        node_idx = torch.where(s == node_max[..., None], cols, torch.full_like(cols, half)).min(-1).values
    if mistake == "descending-index rank ties":
        order = (half - 1) - torch.sort(-node_max.flip(-1), dim=-1, stable=True).indices
    else:
        order = torch.sort(-node_max, dim=-1, stable=True).indices
    return order, node_idx


def _merge(x, order, node_idx, r, mistake=None):
    ref, cnt, _ = X.merge_wavg64(x, order, node_idx, r)
    c = cnt[..., None].double()
    if mistake == "cnt off by one":                                          # in ONE row per sample, the most heavily merged one
        top = (c == c.amax(dim=1, keepdim=True)) & (c > 1)
        ref = torch.where(top, ref * c / (c + 1), ref)
    if mistake == "division by r":
        ref = torch.where(c > 1, ref * c / r, ref)
    if mistake == "trailing token dropped" and x.shape[1] % 2:
        ref = ref.clone()
        ref[:, -1] = 0.0
    return ref


def _unmerge(dy, order, dl, r, N, mistake=None):
    dx, w, _ = X.unmerge64(dy, order, dl, r, N)
    if mistake == "unmerge without the division":
        dx = dx / w[..., None]
    if mistake == "unmerge dy[rank]":
        dx = dx.clone()
        half = N // 2
        for b in range(dy.shape[0]):
            ranks = torch.arange(r, half)
            dx[b, 2 * order[b, r:]] = dy[b].double()[ranks.clamp_max(dy.shape[1] - 1)]
    return dx


SELECTION_MISTAKES = ["last maximal index", "descending-index rank ties", "tail columns ignored"]
MERGE_MISTAKES = ["cnt off by one", "division by r", "trailing token dropped"]
UNMERGE_MISTAKES = ["unmerge without the division", "unmerge dy[rank]"]
OLD_CASES = [(2, 256, 320, 64), (2, 137, 320, 40)]


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("mistake", SELECTION_MISTAKES)
def test_seeded_selection_mistakes_change_the_selection(mistake):
    caught = []
    for case in LATTICE:
        B, N, C, r, star = case
        s = _scores(_keys(case))
        o, n = _select(s)
        o64, n64, _, reff = X.select64(_keys(case), r)
        assert torch.equal(o, o64) and torch.equal(n, n64)                   # the unmutated copy IS the reference
        om, nm = _select(s, mistake)
        if not (torch.equal(om, o) and torch.equal(nm, n) and torch.equal(X.dstlist_of(om, nm, reff), X.dstlist_of(o, n, reff))):
            caught.append(_id(case))
    for case in OLD_CASES:                                                   # what the old 97 % criterion saw
        k = _gauss(case)[0].to(torch.bfloat16).float()
        s = _scores(k, emulate_bf16=True)
        (o, n), (om, nm) = _select(s), _select(s, mistake)
        print(f"[old] {mistake} on Gaussian {_id(case)}: node_idx agreement {float((n == nm).double().mean()):.4f} (old criterion >= 0.97)")
    print(f"[seeded] {mistake}: caught on {caught}")
    assert caught


@pytest.mark.parametrize("mistake", MERGE_MISTAKES + UNMERGE_MISTAKES)
def test_seeded_arithmetic_mistakes_exceed_the_element_tolerance(mistake):
    caught = []
    for case in GAUSS + [c for c in LATTICE if c[4]]:
        B, N, C, r = case[:4]
        k, v = _gauss(case[:4])
        v = v.to(torch.bfloat16).float()
        order, node_idx, _, reff = X.select64(_keys(case) if len(case) == 5 else k, r)
        dl = X.dstlist_of(order, node_idx, reff)
        if mistake in MERGE_MISTAKES:
            ref, cnt, absmean = X.merge_wavg64(v, order, node_idx, reff)
            bad = _merge(v, order, node_idx, reff, mistake).to(torch.bfloat16).double()
            ratio = float(((bad - ref).abs() / X.merge_tolerance(ref, cnt, absmean, 2.0 ** -8)).max())
            print(f"[old] {mistake} on Gaussian {_id(case)}: rel-L2 {_rel_l2(bad, ref):.2e} (old criterion <= 4e-3)")
        else:
            dy = torch.randn(B, N - reff, C, generator=torch.Generator().manual_seed(N)).to(torch.bfloat16).float()
            dx, w, src = X.unmerge64(dy, order, dl, reff, N)
            bad = _unmerge(dy, order, dl, reff, N, mistake).to(torch.bfloat16).double()
            ratio = float(((bad - dx).abs() / X.unmerge_tolerance(dx, src, 2.0 ** -8).clamp_min(1e-300)).max())
            print(f"[old] {mistake} on Gaussian {_id(case)}: rel-L2 {_rel_l2(bad, dx):.2e} (no direct old criterion; whole-UNet VJP 5e-2)")
        if ratio > 1.0:
            caught.append(_id(case))
    print(f"[seeded] {mistake}: exceeds the tolerance on {caught}")
    assert caught
