"""Host self-test of tests/graph_ref.py (CPU only, no GPU import): what the node-local criteria of tests/test_gpu_graph_nodes.py can
and cannot see, shown on the storage emulation with seeded wiring mistakes.

  * graph_ref.forward is oracle/models_ref.py bit for bit (values and gradients), so a seeded mistake is the only difference;
  * the stored FLOORS table is the re-measured emulation distance (10 %); the printed `FLOORS[...] = ...` lines are the procedure
    to update it;
  * the `fused` emulation - a graph that rounds LESS often - passes the verdict in both storage types;
  * every (mistake, site) pair of the catalogue fails the fp16 verdict, except the pairs named in graph_ref.BLIND (none of them of
    the 18 kinds of the sensitivity table); per kind one `[seeded]` line: smallest ratio, its site, whether bf16 catches that site too,
    and the same pair's ratio when only eps and d_x are judged by the same rule;
  * `[old]` lines: the same mistakes on tiny_unet() under the criteria the suite had before - eps <= 3e-2, d_x <= 5e-2, level taps
    <= 5e-3 (the fp16 run's) or <= 2e-2 (the bf16 run's) - judged on the fp16 emulation, so the bf16 count leaves out bf16's own
    noise.  Sites that PASS there, fp16 gates / bf16 gates, of all sites (measured with this file):
        time_emb_proj dropped 5 / 5 of 22       conv1 bias 5 / 22 of 22          conv2 bias 0 / 3 of 22          shortcut bias 0 / 4 of 14
        attn1 to_out bias 0 / 13 of 16          attn2 to_out bias 0 / 12 of 16   ff.net.2 bias 0 / 14 of 16      ff.net.0.proj bias 0 / 16 of 16
        proj_in bias 0 / 11 of 16               proj_out bias 0 / 2 of 16        LN1 beta 0 / 13 of 16           LN2 beta 13 / 16 of 16
        LN3 beta 0 / 13 of 16                   norm2 beta 0 / 18 of 22          sampler bias 0 / 0 of 6         ToMe unmerge bypassed 16 / 16 of 16
        gradient blocked through attn1 12 of 16, attn2 16 of 16, FF 5 of 16 (either gate set: only d_x <= 5e-2 looks at them)
        context of the other sample 0 of 16, timestep of the other sample 5 of 22, skip concat halves swapped 0 of 12, dskip dropped
        1 of 12, outer residual's gradient dropped 1 of 16, identity-shortcut gradient 0 of 8, downsampler's addend 0 of 3,
        GroupNorm eps 16 of 16.
    The five sites of time_emb_proj / conv1 bias / the other sample's timestep that pass even the fp16 gates are the C == G ones:
    the test asserts those, the rest is printed.
  * the C == G fact itself: on tiny_unet() dropping down_blocks.0.resnets.0.time_emb_proj does not move eps - the subtraction of the
    group mean removes the constant, so what is left is the rounding of that subtraction: below 64 units in the last place of
    whichever arithmetic runs it, fp32 (6e-7 measured) and float64 (1e-15) alike; on GRAPH_CFG it moves eps by 5.6e-2."""
import pytest
import torch

import graph_ref as G
from oracle import models_ref as M

_REF = {}


def _case(name, size=(16, 16), tome_r=0):
    key = (name, tuple(size), tome_r)
    if key not in _REF:
        cfg = G.CONFIGS[name]
        sd = G.state_dict(cfg)
        x, t, ctx, cot, added = G.inputs(cfg, *size)
        _REF[key] = (cfg, sd, (x, t, ctx, cot, added), G.oracle(sd, cfg, x, t, ctx, cot, tome_r=tome_r, added_cond=added))
    return _REF[key]


def _emulate(name, dtype, size=(16, 16), tome_r=0, **kw):
    cfg, sd, (x, t, ctx, cot, added), _ = _case(name, size, tome_r)
    return G.emulate(sd, cfg, x, t, ctx, cot, dtype, tome_r=tome_r, added_cond=added, **kw)


@pytest.mark.parametrize("name,tome_r", [("graph", 0), ("graph_lin", 0), ("graph", G.TOME_R), ("tiny_sdxl", 0)])
def test_restatement_is_the_oracle_bit_for_bit(name, tome_r):
    ref = _case(name, (9, 15) if name == "graph_lin" else (16, 16), tome_r)[3]
    got = _emulate(name, None, (9, 15) if name == "graph_lin" else (16, 16), tome_r)
    assert list(got["out"]) == list(ref["out"]) == G.node_names(G.CONFIGS[name])
    assert torch.equal(got["eps"], ref["eps"]) and torch.equal(got["d_x"], ref["d_x"])
    for k in ref["out"]:
        assert torch.equal(got["out"][k], ref["out"][k]) and torch.equal(got["grad"][k], ref["grad"][k]), k


def _keys():
    return sorted(G.FLOORS)


@pytest.mark.parametrize("key", _keys(), ids=lambda k: f"{k[0]}-{k[1][0]}x{k[1][1]}-{k[2]}")
def test_floor_table_is_current(key):
    label, size, dn = key
    name, _, tome = label.partition("+tome")
    dtype = {v: k for k, v in G.DT_NAME.items()}[dn]
    tome_r = int(tome) if tome else 0
    ref = _case(name, size, tome_r)[3]
    fresh = G.distances(_emulate(name, dtype, size, tome_r), ref)
    c = G.compact(fresh, G.CONFIGS[name])
    fmt = lambda v: "[" + ", ".join(f"{e:.3e}" for e in v) + "]"
    print(f"FLOORS[{key!r}] = {{'eps': {c['eps']:.3e}, 'd_x': {c['d_x']:.3e},\n    'out': {fmt(c['out'])},\n    'grad': {fmt(c['grad'])}}}")
    stored = G.floors_for(name, size, dtype, tome_r)
    pairs = [("eps", stored["eps"], fresh["eps"]), ("d_x", stored["d_x"], fresh["d_x"])]
    pairs += [(f"{g} {k}", stored[g][k], fresh[g][k]) for g in ("out", "grad") for k in fresh[g]]
    off = [(n, s, f) for n, s, f in pairs if not abs(s - f) <= 0.1 * f]
    assert not off, f"stored floors differ from the re-measurement by more than 10 %: {off[:5]}"


@pytest.mark.parametrize("dtype", G.DTYPES, ids=lambda d: G.DT_NAME[d])
@pytest.mark.parametrize("name,size", [("graph", (16, 16)), ("graph", (9, 15)), ("graph_lin", (16, 16))])
def test_a_graph_that_rounds_less_often_is_not_flagged(name, size, dtype):
    ref = _case(name, size)[3]
    ok, _, worst = G.verdict(_emulate(name, dtype, size, fused=True), ref, G.floors_for(name, size, dtype), dtype)
    print(f"[fused] {name} {size} {G.DT_NAME[dtype]}: " + "  ".join(f"{g} {r:.2f} ({k})" for g, (r, k) in worst.items()))
    assert ok


def _pairs(name, kind):
    cfg, sd = G.CONFIGS[name], _case(name)[1]
    return [(k, s) for k, s in G.catalogue(cfg, sd) if k == kind]


@pytest.mark.parametrize("kind", list(G.MISTAKES))
def test_seeded_mistake_fails_the_fp16_verdict_at_every_site(kind):
    tome_r = G.TOME_R if kind in G.TOME_KINDS else 0
    ref = _case("graph", (16, 16), tome_r)[3]
    rows = []
    for pair in _pairs("graph", kind):
        got = _emulate("graph", torch.float16, tome_r=tome_r, mistake=pair)
        ok, ratios, worst = G.verdict(got, ref, G.floors_for("graph", (16, 16), torch.float16, tome_r), torch.float16)
        rows.append((G.worst_ratio(worst), pair[1], max(ratios["eps"], ratios["d_x"]), ok))
    assert rows, "no site of this kind in GRAPH_CFG"
    r, site, e2e, _ = min(rows)
    got = _emulate("graph", torch.bfloat16, tome_r=tome_r, mistake=(kind, site))
    bok, _, bworst = G.verdict(got, ref, G.floors_for("graph", (16, 16), torch.bfloat16, tome_r), torch.bfloat16)
    print(f"[seeded] {kind}: {len(rows)} sites, smallest fp16 ratio {r:.2f} at {site} (bf16 there: {G.worst_ratio(bworst):.2f}, "
          f"{'caught' if not bok else 'NOT caught'}); eps / d_x alone: smallest {min(x[2] for x in rows):.2f}, "
          f"missed at {sum(x[2] <= 1 for x in rows)} sites")
    missed = [(kind, s) for _, s, _, ok in rows if ok]
    unlisted = [p for p in missed if p not in G.BLIND]
    assert not unlisted, f"undetected in fp16 and not in graph_ref.BLIND: {unlisted}"
    stale = [p for p in G.BLIND if p[0] == kind and p not in missed]
    assert not stale, f"listed in graph_ref.BLIND but detected: {stale}"


def test_blind_list_names_catalogue_pairs_with_reasons_and_none_of_the_table_kinds():
    cat = set(G.catalogue(G.GRAPH_CFG, _case("graph")[1]))
    for pair, reason in G.BLIND.items():
        assert pair in cat and pair[0] not in G.TABLE_KINDS and isinstance(reason, str) and reason.strip()
    assert len(G.TABLE_KINDS) == 18


OLD_EPS, OLD_DX, OLD_TAP, OLD_TAP_BF16 = 3e-2, 5e-2, 5e-3, 2e-2
# kinds whose every tiny_unet() site passes the old criteria whatever the rounding noise does: see the module docstring
C_EQ_G_SITES = ("down_blocks.0.resnets.0", "down_blocks.0.resnets.1", "up_blocks.3.resnets.0", "up_blocks.3.resnets.1", "up_blocks.3.resnets.2")


@pytest.mark.parametrize("kind", list(G.MISTAKES))
def test_old_criteria_on_the_tiny_unet(kind):
    tome_r = G.TOME_R if kind in G.TOME_KINDS else 0
    cfg, sd, _, ref = _case("tiny", (16, 16), tome_r)
    ref_taps = G.level_taps(cfg, ref["out"])
    passing, passing_bf16, rows = [], [], []
    for pair in _pairs("tiny", kind):
        got = _emulate("tiny", torch.float16, tome_r=tome_r, mistake=pair)
        taps = G.level_taps(cfg, got["out"])
        e, dx = G.rel_l2(got["eps"], ref["eps"]), G.rel_l2(got["d_x"], ref["d_x"])
        tp = max(G.rel_l2(taps[k], ref_taps[k]) for k in ref_taps)
        rows.append((pair[1], e, dx, tp))
        if e <= OLD_EPS and dx <= OLD_DX and tp <= OLD_TAP:
            passing.append(pair[1])
        if e <= OLD_EPS and dx <= OLD_DX and tp <= OLD_TAP_BF16:
            passing_bf16.append(pair[1])
    if not rows:
        print(f"[old] {kind}: no site in tiny_unet()")
        return
    print(f"[old] {kind}: {len(passing)} of {len(rows)} sites pass eps <= {OLD_EPS} / taps <= {OLD_TAP} / d_x <= {OLD_DX}, "
          f"{len(passing_bf16)} with taps <= {OLD_TAP_BF16}; "
          f"eps {min(r[1] for r in rows):.4f} .. {max(r[1] for r in rows):.4f}, d_x {min(r[2] for r in rows):.4f} .. {max(r[2] for r in rows):.4f}, "
          f"worst level tap {min(r[3] for r in rows):.4f} .. {max(r[3] for r in rows):.4f}")
    if kind in ("time_emb_proj dropped", "conv1 bias dropped", "timestep of the other sample"):
        # one channel per group: the GroupNorm behind conv1 removes every per-channel constant - the old criteria are blind there
        assert set(C_EQ_G_SITES) <= set(passing)


def test_one_channel_per_group_hides_the_time_embedding():
    p = "down_blocks.0.resnets.0.time_emb_proj"
    for name, moves in (("tiny", False), ("graph", True)):
        cfg, sd, (x, t, ctx, cot, added), ref = _case(name)
        assert (cfg.block_out_channels[0] == cfg.norm_num_groups) == (not moves)
        cut = dict(sd)
        for k in (p + ".weight", p + ".bias"):
            cut[k] = torch.zeros_like(sd[k])
        d = G.rel_l2(M.unet_forward(cut, cfg, x, t, ctx), ref["eps"])
        dbl = lambda s_: {k: v.double() for k, v in s_.items()}
        d64 = G.rel_l2(M.unet_forward(dbl(cut), cfg, x.double(), t, ctx.double()), M.unet_forward(dbl(sd), cfg, x.double(), t, ctx.double()))
        print(f"[c==g] {name}: dropping {p} moves eps by {d:.3e} in fp32, {d64:.3e} in float64")
        if moves:
            assert d > 1e-3 and d64 > 1e-3
        else:
            assert d <= 64 * 2.0 ** -24 and d64 <= 64 * 2.0 ** -53
