"""Self-test of the forward attention reference and error model (tests/attn_fwd_ref.py) - host only, no GPU.

The bound that judges the kernels in tests/test_gpu_attn_fwd.py must be ACHIEVABLE - a plain torch fp32 emulation of the kernels'
arithmetic (64-key tiles, running or first-tile reference maximum with re-centring above TAU, exp2, P rounded to the storage type,
fp32 P V accumulation, one output rounding) stays inside it on every input family, with the derived K_FWD - and SHARP: seeded
mutations of that emulation (a key dropped or doubled, a tile skipped, pad keys included, a wrong scale, the wrong head's V, a
skipped rescale, a row sum that misses a tile) each fail it on the family designed for them, also when confined to one 16-row
fragment.  For every mutation the whole-tensor criterion of tests/test_gpu_kernels.py (rel-L2 against TOL_ATTN) is printed next
to the worst ratio of the element-wise bound; only the latter is asserted.  Both storage types by parameter."""
import math

import pytest
import torch

import attn_fwd_ref as R

TOL_ATTN = 1e-2                      # tests/test_gpu_kernels.py
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


def emulate(q, k, v, heads, presc, dt, fold, mut=None, rows=None):
    """fp32 emulation of one forward attention launch on [B, N, heads * D] operands.  fold = False: running maximum, row sum from
    the unrounded p (k_attn, plain k_attn2); fold = True (needs presc): reference maximum of the first tile, re-centred when a
    score exceeds it by TAU, row sum from the rounded p when D % 16 != 0 (k_attn2 FOLD, k_attn3).  mut names a seeded mistake,
    applied to the query rows `rows` (boolean [Nq], default all)."""
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // heads
    sp = lambda t: t.float().reshape(B, t.shape[1], heads, D).transpose(1, 2)
    Q, K, V = sp(q), sp(k), sp(v)
    rows = torch.ones(Nq, dtype=torch.bool) if rows is None else rows
    rmask = rows.view(1, 1, Nq, 1)
    if mut == "pad_keys":                       # (d) keys Nk .. ceil8(Nk): zero K (score 0), zero V
        pad = (Nk + 7) // 8 * 8 - Nk
        assert pad > 0
        K = torch.cat([K, torch.zeros(B, heads, pad, D)], 2)
        V = torch.cat([V, torch.zeros(B, heads, pad, D)], 2)
    if mut == "next_head_v":                    # (f)
        V = V.roll(-1, 1)
    n_keys = K.shape[2]
    Dscale = (D + 15) // 16 * 16 if mut == "scale_d16" else D                    # (e)
    sc = torch.tensor(1.0 if presc else 1.0 / math.sqrt(Dscale), dtype=torch.float32) * (1.0 if presc else R.LOG2E)
    tau = R.TAU[dt]
    ones = fold and D % 16 != 0
    m = torch.zeros(B, heads, Nq, 1) if fold else torch.full((B, heads, Nq, 1), -1e30)
    l = torch.zeros(B, heads, Nq, 1)
    o = torch.zeros(B, heads, Nq, D)
    nt = (n_keys + 63) // 64
    for t in range(nt):
        j0, j1 = t * 64, min(t * 64 + 64, n_keys)
        if mut == "skip_partial_tile" and j1 - j0 < 64:                          # (c)
            continue
        s = Q @ K[:, :, j0:j1].transpose(-1, -2)
        if fold:
            s = s - m
            mx = s.max(-1, keepdim=True).values
            delta = mx if t == 0 else torch.where(mx > tau, mx, torch.zeros_like(mx))
            alpha = torch.exp2(-delta)
            m = m + delta
            p = torch.exp2(s - delta)
        else:
            mx = s.max(-1, keepdim=True).values
            m_new = torch.maximum(m, mx)
            alpha = torch.exp2((m - m_new) * sc)
            p = torch.exp2(s * sc - m_new * sc)
            m = m_new
        if j1 == n_keys and mut in ("drop_last", "double_last"):                 # (a), (b)
            f = 0.0 if mut == "drop_last" else 2.0
            p = torch.cat([p[..., :-1], torch.where(rmask, p[..., -1:] * f, p[..., -1:])], -1)
        p16 = p.to(dt).float()
        ls = (p16 if ones else p).sum(-1, keepdim=True)
        if mut == "sum_misses_first_tile" and t == 0:                            # (h)
            ls = torch.where(rmask, torch.zeros_like(ls), ls)
        l = l * alpha + ls
        a_o = torch.where(rmask, torch.ones_like(alpha), alpha) if (mut == "skip_rescale" and t == 1) else alpha   # (g)
        o = o * a_o + p16 @ V[:, :, j0:j1]
    out = (o * (1.0 / l)).to(dt).float()
    return out.transpose(1, 2).reshape(B, Nq, C)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


B, H, NQ, NK = 2, 2, 150, 205


def _families(D, presc, dt):
    """name -> (q, k, v)"""
    tau = R.TAU[dt]
    fams = {
        "randn": R.family_randn(B, H, NQ, NK, D, presc, dt),
        "probes": R.family_probes(B, H, NQ, NK, D, presc, dt)[:3],
        "ramp up": R.family_ramp(B, H, NQ, NK, D, presc, dt, up=True),
        "ramp down": R.family_ramp(B, H, NQ, NK, D, presc, dt, up=False),
        "balanced": R.family_balanced(B, H, NQ, NK, D, presc, dt),
        "uniform": R.family_uniform(B, H, NQ, NK, D, presc, dt),
        "negative": R.family_negative(B, H, NQ, NK, D, presc, dt),
        "one key": R.family_randn(B, H, NQ, 1, D, presc, dt),
    }
    for e in (tau - 2, tau + 2, 90.0, 300.0):
        fams[f"late key +{e:g}"] = R.family_late_key(B, H, NQ, NK, D, presc, dt, e)[:3]
    return fams


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [32, 40])
def test_fp32_emulation_is_inside_the_bound_on_every_family(D, dt):
    """D = 40: padded head dim, the folded emulation takes its row sum from the rounded p; D = 32: from the unrounded p."""
    worst = {}
    for presc, fold in ((0, False), (1, False), (1, True)):
        for name, (q, k, v) in _families(D, presc, dt).items():
            got = emulate(q, k, v, H, presc, dt, fold)
            ref, bound = R.fwd_ref(q, k, v, H, presc)
            tiny = R.fwd_tiny(v, dt)
            w = R.check(f"emulation {IDS[DTYPES.index(dt)]} D{D} presc{presc} fold{int(fold)} {name}", got, ref, bound, dt, tiny=tiny)
            worst[name] = max(worst.get(name, 0.0), w)
            if name == "one key":
                assert torch.equal(got, v.expand_as(got)), "one key: the output is V's single row bit for bit"
    print(f"[emulation] D{D} {IDS[DTYPES.index(dt)]} worst ratio per family (K_FWD = {R.K_FWD}): "
          + ", ".join(f"{n} {w:.2f}" for n, w in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_late_key_lands_on_the_intended_side_of_tau(dt):
    tau = R.TAU[dt]
    for e, above in ((tau - 2, False), (tau + 2, True), (90.0, True), (300.0, True)):
        q, k, v, row = R.family_late_key(B, H, NQ, NK, 40, 1, dt, e)
        x = R.first_tile_excess(q, k, H, 1)
        assert (float(x.max()) > tau + 0.5) == above and abs(float(x[:, :, row].min()) - e) < 0.05 * e + 0.5, (e, float(x.max()))


def _fragment(Nq):
    """the second 16-row fragment of the last 128-row query block"""
    r = torch.zeros(Nq, dtype=torch.bool)
    q0 = (Nq - 1) // 128 * 128 + 16
    r[q0:q0 + 16] = True
    return r


# mutation -> (family that is designed to show it, presc, fold, rows)
MUTATIONS = [
    ("(a) last key dropped", "drop_last", "probes", 1, True, None),
    ("(b) last key counted twice", "double_last", "probes", 1, True, None),
    ("(c) partial tile skipped", "skip_partial_tile", "probes", 1, True, None),
    ("(d) pad keys included, V = 0", "pad_keys", "negative", 1, True, None),
    ("(e) scale from D rounded up to 16", "scale_d16", "balanced", 0, False, None),
    ("(f) head h reads head h+1's V", "next_head_v", "randn", 0, False, None),
    ("(g) rescale skipped for one tile", "skip_rescale", "ramp up", 0, False, None),
    ("(h) row sum misses the first tile", "sum_misses_first_tile", "randn", 0, False, None),
    ("(a) in one 16-row fragment", "drop_last", "probes", 1, True, "fragment"),
    ("(b) in one 16-row fragment", "double_last", "probes", 1, True, "fragment"),
    # the same two at a shape and on the inputs of today's tests (1024 x 1000, randn): what rel-L2 sees of them - a record, not
    # asserted (on randn inputs one key of 1000 is worth less than the roundings of a correct kernel in most rows)
    ("(a) one fragment, 1024 x 1000", "drop_last", "probes", 1, True, "fragment", (1024, 1000)),
    ("(b) one fragment, 1024 x 1000", "double_last", "probes", 1, True, "fragment", (1024, 1000)),
    ("(a) everywhere, randn inputs, 1024 x 1000", "drop_last", "randn", 1, True, None, (1024, 1000)),
    ("(a) one fragment, randn inputs, 1024 x 1000", "drop_last", "randn", 1, True, "fragment", (1024, 1000)),
    ("(b) one fragment, randn inputs, 1024 x 1000", "double_last", "randn", 1, True, "fragment", (1024, 1000)),
]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_seeded_mutations_fail_the_bound(dt):
    D = 40
    lines, missed = [], []
    for label, mut, fam, presc, fold, rows, *shape in MUTATIONS:
        Nq, Nk = shape[0] if shape else (300, 205)      # three query blocks, the last a tail; four key tiles, the last partial; pad 205 .. 208
        build = {"randn": R.family_randn, "probes": lambda *a: R.family_probes(*a)[:3], "balanced": R.family_balanced,
                 "negative": R.family_negative, "ramp up": R.family_ramp}[fam]
        q, k, v = build(B, H, Nq, Nk, D, presc, dt)
        rmask = _fragment(Nq) if rows else None
        ref, bound = R.fwd_ref(q, k, v, H, presc)
        tiny = R.fwd_tiny(v, dt)
        tag = f"{IDS[DTYPES.index(dt)]} {label}"
        clean = R.check(f"{tag}, unmutated", emulate(q, k, v, H, presc, dt, fold), ref, bound, dt, tiny=tiny)
        got = emulate(q, k, v, H, presc, dt, fold, mut=mut, rows=rmask)
        old, new = rel_l2(got, ref), R.check(f"{tag}, mutated", got, ref, bound, dt, tiny=tiny, enforce=False)
        lines.append(f"| {label} | {fam} {Nq} x {Nk} | {old:.1e} {'FAIL' if old > TOL_ATTN else 'pass'} | {new:.3g} {'FAIL' if new > 1 else 'pass'} | {clean:.2f} |")
        # the randn rows are the record of what the whole-tensor criterion sees; the designed family must catch the mutation
        if not new > 1.0 and "randn inputs" not in label:
            missed.append(label)
    print(f"\n[mutations] {IDS[DTYPES.index(dt)]}, D = {D}: rel-L2 against TOL_ATTN = {TOL_ATTN} (today) | worst element-wise ratio (asserted)")
    print("| mutation | inputs | rel-L2 | bound ratio | unmutated ratio |\n|---|---|---|---|---|")
    print("\n".join(lines))
    assert not missed, f"mutations inside the bound: {missed}"


def test_expects_qloop_mirrors_the_launcher():
    assert R.expects_qloop(16, 8, 4096, 77, 40) == 8 and R.expects_qloop(2, 8, 1024, 77, 40) == 0
    assert R.expects_qloop(13, 16, 600, 77, 40) == 2 and R.expects_qloop(32, 32, 200, 80, 64) == 2
    assert R.expects_qloop(13, 16, 640, 256, 80) == 2 and R.expects_qloop(13, 16, 640, 257, 80) == 0
    assert R.expects_qloop(13, 16, 640, 192, 160) == 2 and R.expects_qloop(13, 16, 640, 193, 160) == 0
    assert R.expects_qloop(16, 8, 4096, 77, 32) == 0
