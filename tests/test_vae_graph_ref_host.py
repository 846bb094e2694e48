"""Host self-test of tests/vae_graph_ref.py (CPU only, no GPU import): what the node-local criteria of
tests/test_gpu_vae_graph_nodes.py can and cannot see, shown on the storage emulation with seeded wiring mistakes.

  * vae_graph_ref.encode / decode are oracle/models_ref.py bit for bit (values and gradients), so a seeded mistake is the only difference;
  * the stored FLOORS table is the re-measured emulation distance (10 %); the printed `FLOORS[...] = ...` lines are the procedure
    to update it;
  * the `fused` emulation - a graph that rounds LESS often - passes the verdict in both storage types;
  * every (mistake, site) pair of the catalogue fails the fp16 verdict on vae_graph at 8x12, except the pairs named in
    vae_graph_ref.BLIND (the two eps pairs; no bias, beta, residual, pad, upsampling or shortcut kind may be there); per kind one
    `[seeded]` line: smallest ratio, its site, whether bf16 catches that site too, and the same pair's ratio when only the outer
    tensors (moments, or image and d_z) are judged by the same rule;
  * the key bias is invisible by construction (the softmax removes a per-row constant): the oracle's output moves by rounding only;
  * `[old]` lines: the same kinds on tiny_vae() at 8x12 latents under the gates the suite had before - image and moments <= 3e-2,
    d_z <= 5e-2 - judged on the fp16 emulation, so the count leaves out bf16's own noise.  Sites that PASS there, of all sites
    (measured with this file):
        conv1 bias 24 of 24                  conv2 bias 15 of 24                  norm2 beta 23 of 24              shortcut bias 1 of 2
        sampler conv bias 4 of 6             attention group_norm beta 2 of 2     query bias 2 of 2                value bias 2 of 2
        proj_attn bias 2 of 2                conv_in bias 1 of 2                  every norm's eps 2 of 2
        none of: quant_conv / post_quant_conv / conv_out bias (0 of 1, 1, 2), conv_norm_out beta (2), attention residual dropped (2),
        wrong softmax scale (2), SiLU dropped (2), pad on the wrong side (3), upsampling shifted in x / in y (3 each), halves swapped
        (1), the other sample's tensor (2), circular explicit pad (3), and the gradient-only kinds: identity-shortcut (13), shortcut
        conv (1), attention branch (1), attention residual (1), upsampler contribution (3) - d_z <= 5e-2 does see those.
    So the old gates miss dropped biases and betas inside the graph (76 of 90 such sites), not the structural mistakes.
    Only the C == G sites are asserted (conv1 bias at the five resnets of tiny_vae() whose conv1 writes 32 channels in 32 groups: the
    GroupNorm behind conv1 removes every per-channel constant); the rest is printed."""
import pytest
import torch

import vae_graph_ref as V
from oracle import models_ref as M

SIZE = V.SIZES[0]


def _tiling_of(kind):
    return "xy" if kind in V.TILING_KINDS else None


@pytest.mark.parametrize("name,size,tiling", [("vae_graph", (8, 12), None), ("vae_graph", (5, 7), None), ("vae_wide", (8, 12), None),
                                              ("vae_graph", (8, 12), "xy")])
@pytest.mark.parametrize("path", V.PATHS)
def test_restatement_is_the_oracle_bit_for_bit(name, size, tiling, path):
    ref = V.case(name, size, path, tiling)[3]
    got = V.emulate(name, size, path, None, tiling)
    assert list(got) == list(ref) and list(got["out"]) == list(ref["out"]) == V.node_names(V.CONFIGS[name], path)
    for k, v in ref.items():
        if isinstance(v, dict):
            for n in v:
                assert torch.equal(got[k][n], v[n]), (k, n)
        else:
            assert torch.equal(got[k], v), k
    assert ("grad" in ref) == (path == "decode" and tiling is None)


def _dtype(dn):
    return {v: k for k, v in V.DT_NAME.items()}[dn]


@pytest.mark.parametrize("key", V.floor_keys(), ids=lambda k: f"{k[0]}-{k[1][0]}x{k[1][1]}-{k[2]}-{k[3]}-{k[4]}")
def test_floor_table_is_current(key):
    name, size, path, til, dn = key
    tiling = None if til == "plain" else til
    ref = V.case(name, size, path, tiling)[3]
    fresh = V.distances(V.emulate(name, size, path, _dtype(dn), tiling), ref)
    fmt = lambda v: ("[" + ", ".join(f"{e:.3e}" for e in v) + "]") if isinstance(v, list) else f"{v:.3e}"
    print(f"FLOORS[{key!r}] = {{" + ",\n    ".join(f"'{k}': {fmt(v)}" for k, v in V.compact(fresh, V.CONFIGS[name], path).items()) + "}")
    assert key in V.FLOORS, "no stored floors for this key"
    stored = V.floors_for(name, size, path, _dtype(dn), tiling)
    assert list(stored) == list(fresh)
    pairs = []
    for k, v in fresh.items():
        pairs += [(f"{k} {n}", stored[k][n], x) for n, x in v.items()] if isinstance(v, dict) else [(k, stored[k], v)]
    off = [(n, s, f) for n, s, f in pairs if not abs(s - f) <= 0.1 * f]
    assert not off, f"stored floors differ from the re-measurement by more than 10 %: {off[:5]}"


def test_floor_table_holds_exactly_the_keys_of_the_gpu_test():
    assert sorted(V.FLOORS) == sorted(V.floor_keys())


@pytest.mark.parametrize("key", V.floor_keys(), ids=lambda k: f"{k[0]}-{k[1][0]}x{k[1][1]}-{k[2]}-{k[3]}-{k[4]}")
def test_a_graph_that_rounds_less_often_is_not_flagged(key):
    name, size, path, til, dn = key
    tiling = None if til == "plain" else til
    ref = V.case(name, size, path, tiling)[3]
    ok, _, worst = V.verdict(V.emulate(name, size, path, _dtype(dn), tiling, fused=True), ref, V.floors_for(name, size, path, _dtype(dn), tiling))
    print(f"[fused] {name} {size} {path} {til} {dn}: " + "  ".join(f"{g} {r:.2f} ({k})" for g, (r, k) in worst.items()))
    assert ok


def _pairs(name, kind):
    cfg, sd = V.CONFIGS[name], V.case(name, SIZE, "encode")[1]
    return [(k, s) for k, s in V.catalogue(cfg, sd) if k == kind]


@pytest.mark.parametrize("kind", list(V.MISTAKES))
def test_seeded_mistake_fails_the_fp16_verdict_at_every_site(kind):
    tiling = _tiling_of(kind)
    rows = []
    for pair in _pairs("vae_graph", kind):
        path = V.path_of(pair[1])
        if tiling and path == "decode":
            continue
        ref = V.case("vae_graph", SIZE, path, tiling)[3]
        got = V.emulate("vae_graph", SIZE, path, torch.float16, tiling, mistake=pair)
        ok, ratios, worst = V.verdict(got, ref, V.floors_for("vae_graph", SIZE, path, torch.float16, tiling))
        rows.append((V.worst_ratio(worst), pair[1], V.outer_ratio(ratios), ok))
    assert rows, "no site of this kind in the vae_graph config"
    r, site, _, _ = min(rows)
    path = V.path_of(site)
    got = V.emulate("vae_graph", SIZE, path, torch.bfloat16, tiling, mistake=(kind, site))
    bok, _, bworst = V.verdict(got, V.case("vae_graph", SIZE, path, tiling)[3], V.floors_for("vae_graph", SIZE, path, torch.bfloat16, tiling))
    print(f"[seeded] {kind}: {len(rows)} sites, smallest fp16 ratio {r:.2f} at {site} (bf16 there: {V.worst_ratio(bworst):.2f}, "
          f"{'caught' if not bok else 'NOT caught'}); outer tensors alone: {[x[2] for x in rows if x[1] == site][0]:.2f} there, smallest "
          f"{min(x[2] for x in rows):.2f}, missed at {sum(x[2] <= 1 for x in rows)} sites")
    missed = [(kind, s) for _, s, _, ok in rows if ok]
    unlisted = [p for p in missed if p not in V.BLIND]
    assert not unlisted, f"undetected in fp16 and not in vae_graph_ref.BLIND: {unlisted}"
    stale = [p for p in V.BLIND if p[0] == kind and p not in missed]
    assert not stale, f"listed in vae_graph_ref.BLIND but detected: {stale}"


def test_blind_list_names_catalogue_pairs_with_reasons_and_no_bias_residual_pad_or_upsample_kind():
    cat = set(V.catalogue(V.CONFIGS["vae_graph"], V.case("vae_graph", SIZE, "encode")[1]))
    for pair, reason in V.BLIND.items():
        assert pair in cat and pair[0] not in V.NEVER_BLIND and isinstance(reason, str) and reason.strip()
    assert len(V.NEVER_BLIND) == 23 and V.KEY_BIAS not in V.MISTAKES


@pytest.mark.parametrize("half", ["encoder", "decoder"])
def test_key_bias_is_invisible_by_construction(half):
    """q . (k_j + b) = q . k_j + q . b: one constant per query row, which the softmax removes.  What is left is the rounding of the
    row maximum's subtraction: far below the 1e-4 a visible bias moves the output by (the query bias moves it by more than 1e-3)."""
    cfg, sd, (z, img, cot), _ = V.case("vae_graph", SIZE, "encode")
    run = (lambda s_, x: M.vae_encode_moments(s_, cfg, x)) if half == "encoder" else (lambda s_, x: M.vae_decode(s_, cfg, x))
    x = img if half == "encoder" else z
    dbl = lambda s_: {k: v.double() for k, v in s_.items()}
    moved = {}
    for b in ("key", "query"):
        cut = dict(sd)
        k = f"{half}.mid_block.attentions.0.{b}.bias"
        assert float(sd[k].abs().max()) > 0
        cut[k] = torch.zeros_like(sd[k])
        with torch.no_grad():
            moved[b] = (V.rel_l2(run(cut, x), run(sd, x)), V.rel_l2(run(dbl(cut), x.double()), run(dbl(sd), x.double())))
        print(f"[keybias] {half}: dropping the {b} bias moves the output by {moved[b][0]:.3e} in fp32, {moved[b][1]:.3e} in float64")
    assert moved["key"][0] <= 1e-5 and moved["key"][1] <= 1e-13
    assert moved["query"][0] > 1e-4 and moved["query"][1] > 1e-4


OLD_OUT, OLD_DZ = 3e-2, 5e-2
# conv1 writes 32 channels in 32 groups there: norm2 removes a per-channel constant, whatever the rounding noise does
C_EQ_G_SITES = ("encoder.down_blocks.0.resnets.0", "encoder.down_blocks.0.resnets.1", "decoder.up_blocks.3.resnets.0",
                "decoder.up_blocks.3.resnets.1", "decoder.up_blocks.3.resnets.2")


@pytest.mark.parametrize("kind", list(V.MISTAKES))
def test_old_criteria_on_the_tiny_vae(kind):
    tiling = _tiling_of(kind)
    passing, rows = [], []
    for pair in _pairs("tiny", kind):
        path = V.path_of(pair[1])
        if tiling and path == "decode":
            continue
        ref = V.case("tiny", SIZE, path, tiling)[3]
        got = V.emulate("tiny", SIZE, path, torch.float16, tiling, mistake=pair)
        d = V.distances(got, ref)
        outer = d["moments"] if path == "encode" else d["image"]
        dz = d.get("d_z", 0.0)
        rows.append((pair[1], outer, dz))
        if outer <= OLD_OUT and dz <= OLD_DZ:
            passing.append(pair[1])
    print(f"[old] {kind}: {len(passing)} of {len(rows)} sites pass image / moments <= {OLD_OUT} and d_z <= {OLD_DZ}; "
          f"image / moments {min(r[1] for r in rows):.4f} .. {max(r[1] for r in rows):.4f}, d_z {min(r[2] for r in rows):.4f} .. {max(r[2] for r in rows):.4f}")
    if kind == "conv1 bias dropped":
        assert V.CONFIGS["tiny"].block_out_channels[0] == V.CONFIGS["tiny"].norm_num_groups
        assert set(C_EQ_G_SITES) <= set(passing)
