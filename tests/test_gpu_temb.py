"""The time-embedding chain (csrc/kernels_elem.hip: k_timestep_embedding, k_rowvec_linear, k_rowvec_small<1|2|4, 0|1|2>,
k_silu_inplace_f32) through its operator entry points, element by element against float64 within the error model derived in
tests/temb_ref.py (constants from the derivation, confirmed on the host by tests/test_temb_ref_host.py), plus the bit-identity of
the small (B <= 4) and the general kernels at operator level."""
import pytest
import torch

import temb_ref as R
from gyre_amd import _lib
from gpu_util import DEV, HDT, check_bound, st, vp

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
BS = (1, 2, 3, 4, 5, 16, 17, 33)
NS = (1, 3, 16, 17, 1284)
ROWS = max(BS)


def _embedding(t, dim, flip, shift):
    B = len(t)
    out = torch.full((B + 1, dim), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().gyre_op_timestep_embedding(st(), vp(t.to(DEV)), B, dim, flip, shift, vp(out)))
    out = out.cpu()
    assert bool((out[B] == SENTINEL).all())
    return out[:B]


def _linear(x, Wd, bias_d, N, silu, pad=5):
    """gyre_op_rowvec_linear on x [B, K] (CPU fp32): (out [B, N], x afterwards), ldo = N + pad on a sentinel-filled buffer whose gaps
    and extra row must stay untouched."""
    B, K = x.shape
    xd = x.to(DEV).contiguous()
    ldo = N + pad
    out = torch.full((B + 1, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().gyre_op_rowvec_linear(st(), vp(xd), B, K, vp(Wd), vp(bias_d), N, int(silu), vp(out), ldo))
    out = out.cpu()
    assert bool((out[:B, N:] == SENTINEL).all()) and bool((out[B] == SENTINEL).all()), "the gaps of out must stay untouched"
    return out[:B, :N], xd.cpu()


def _timestep_linear(t, dim, flip, shift, Wd, bias_d, N):
    B = len(t)
    ldo = N + 5
    out = torch.full((B + 1, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    scratch = torch.full((B, dim), SENTINEL, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().gyre_op_timestep_linear(st(), vp(t.to(DEV)), B, dim, flip, shift, vp(scratch), vp(Wd), vp(bias_d), N, vp(out), ldo))
    out = out.cpu()
    assert bool((out[:B, N:] == SENTINEL).all()) and bool((out[B] == SENTINEL).all())
    return out[:B, :N]


def _emb_check(name, got, t, dim, flip, shift):
    ref, a = R.embedding64(t, dim, flip, shift)
    ratio = ((got.double() - ref).abs() / R.embedding_tolerance(a)).nan_to_num(nan=float("inf"))
    flat = int(ratio.argmax())
    print(f"[bound] {name}: worst ratio {float(ratio.max()):.3g} at (row, column) ({flat // dim}, {flat % dim}): got {float(got.flatten()[flat]):.8g} "
          f"ref {float(ref.flatten()[flat]):.8g} a {float(a.flatten()[flat]):.6g}")
    assert float(ratio.max()) <= 1.0, name
    return float(ratio.max())


@pytest.mark.parametrize("dim", [8, 256, 320])
def test_timestep_embedding_element_wise(dim):
    """k_timestep_embedding for every B, and the same values out of the fused form (k_rowvec_small<., 2>, B <= 4) and the two-launch
    form (B > 4) of timestep_linear: with the identity as weight the Linear reproduces its input exactly."""
    eye = torch.eye(dim).to(HDT).to(DEV)
    worst = {"k_timestep_embedding": 0.0, "k_rowvec_small<.,2>": 0.0}
    for flip in (0, 1):
        for shift in (0.0, 1.0):
            for B in (1, 4, 5, 16):
                for off in range(5 if B < 5 else 1):                       # every timestep value in every row count
                    t = R.timesteps(B, off)
                    name = f"dim{dim} flip{flip} shift{shift:g} B{B} t{t.tolist()[:5]}"
                    got = _embedding(t, dim, flip, shift)
                    worst["k_timestep_embedding"] = max(worst["k_timestep_embedding"], _emb_check(f"timestep_embedding {name}", got, t, dim, flip, shift))
                    fused = _timestep_linear(t, dim, flip, shift, eye, None, dim)
                    w = _emb_check(f"timestep_linear(identity) {name}", fused, t, dim, flip, shift)
                    if B <= 4:
                        worst["k_rowvec_small<.,2>"] = max(worst["k_rowvec_small<.,2>"], w)
                    assert torch.equal(fused, got), "the fused form uses the embedding kernel's expressions: same bits"
    print(f"[bound] worst embedding ratios dim {dim}: {worst}")


@pytest.mark.parametrize("K", [8, 320, 512, 520, 1280, 2056])
def test_rowvec_linear_element_wise(K):
    """Every B (small kernels 1 | 2 | 4 rows, general kernel with one, two and three row groups), N (column groups that end at, before
    and past N), bias and SiLU on and off; one float64 reference per (K, N, SiLU), its first B rows serve every B."""
    worst = {}
    for N in NS:
        x, W, bias = R.linear_inputs(K, N, ROWS, seed=K + N)
        W = W.to(HDT)
        Wd, bd = W.to(DEV), bias.to(DEV)
        for silu in (False, True):
            refs = {has_bias: R.linear64(x, W.float(), bias if has_bias else None, silu) for has_bias in (False, True)}
            sref = R.silu64(x)
            for B in BS:
                for has_bias in (False, True):
                    got, x_after = _linear(x[:B], Wd, bd if has_bias else None, N, silu)
                    ref, bound = refs[has_bias]
                    kern = ("k_rowvec_small" if B <= 4 else "k_rowvec_linear") + ("+silu" if silu else "")
                    w = check_bound(f"rowvec_linear K{K} N{N} B{B} silu{int(silu)} bias{int(has_bias)}", got, ref[:B], bound[:B], k=1.0,
                                    hdt=torch.float32, dims=("row", "column"))
                    worst[kern] = max(worst.get(kern, 0.0), w)
                    # the documented side effect: B > 4 with SiLU leaves silu(x) in x, otherwise x is not written
                    if silu and B > 4:
                        tol = R.silu_s(x[:B]) * R.U32 * sref[:B].abs() + 2.0 ** -150
                        ws = float(((x_after.double() - sref[:B]).abs() / tol).max())
                        worst["k_silu_inplace_f32"] = max(worst.get("k_silu_inplace_f32", 0.0), ws)
                        assert ws <= 1.0, f"x after the call is not silu(x) within s(x) 2^-24: {ws:.3g}"
                    else:
                        assert torch.equal(x_after, x[:B]), "x must be left as it is"
    print(f"[bound] worst rowvec_linear ratios K {K}: {worst}")


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("K", [320, 2056])
def test_small_and_general_kernels_give_the_same_bits(K, silu):
    N = 17
    x, W, bias = R.linear_inputs(K, N, 5, seed=K)
    Wd, bd = W.to(HDT).to(DEV), bias.to(DEV)
    general, _ = _linear(x, Wd, bd, N, silu)                                  # B = 5: k_rowvec_linear (after k_silu_inplace_f32)
    for rows in (4, 2, 1):
        small, _ = _linear(x[:rows], Wd, bd, N, silu)                         # k_rowvec_small<4 | 2 | 1, 0 | 1>
        assert torch.equal(small, general[:rows]), f"B = {rows} differs from rows 0..{rows - 1} of the B = 5 run"
    three, _ = _linear(x[:3], Wd, bd, N, silu)                                # three rows run the four-row kernel
    assert torch.equal(three, general[:3])


@pytest.mark.parametrize("B", [1, 2, 4, 5])
def test_timestep_linear_is_embedding_then_linear(B):
    dim, N = 320, 1284
    _, W, bias = R.linear_inputs(dim, N, 1, seed=11)
    W = W.to(HDT)
    Wd, bd = W.to(DEV), bias.to(DEV)
    for flip, shift in ((1, 0.0), (0, 1.0)):
        t = R.timesteps(B, 2)
        emb = _embedding(t, dim, flip, shift)
        two, _ = _linear(emb, Wd, bd, N, False)
        one = _timestep_linear(t, dim, flip, shift, Wd, bd, N)
        assert torch.equal(one, two), f"B = {B}: timestep_linear differs from embedding followed by linear"
        # and against float64: the Linear's bound plus the embedding's tolerance carried through |W|
        e64, a = R.embedding64(t, dim, flip, shift)
        ref, bound = R.linear64(e64, W.float(), bias, False)
        bound = bound + (R.embedding_tolerance(a) / R.U32) @ W.double().abs().t()
        check_bound(f"timestep_linear B{B} flip{flip} shift{shift:g}", one, ref, bound, k=1.0, hdt=torch.float32, dims=("row", "column"))


def test_refusals():
    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=DEV)
    w = torch.zeros(4096, dtype=HDT, device=DEV)
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    before = L.gyre_last_launch_count()
    assert L.gyre_op_rowvec_linear(st(), vp(buf), 2, 12, vp(w), None, 4, 0, vp(buf), 4) == -1                    # K % 8
    assert L.gyre_op_timestep_embedding(st(), vp(t), 2, 7, 1, 0.0, vp(buf)) == -1                               # odd dim
    assert L.gyre_op_timestep_linear(st(), vp(t), 2, 7, 1, 0.0, vp(buf), vp(w), None, 4, vp(buf), 4) == -1       # odd dim
    assert L.gyre_op_timestep_linear(st(), vp(t), 2, 12, 1, 0.0, vp(buf), vp(w), None, 4, vp(buf), 4) == -1      # dim % 8 and K % 8
    assert L.gyre_op_timestep_linear(st(), vp(t), 5, 16, 1, 0.0, None, vp(w), None, 4, vp(buf), 4) == -1         # B > 4 needs the scratch
    assert L.gyre_op_rowvec_linear(st(), None, 2, 8, vp(w), None, 4, 0, vp(buf), 4) == -1
    assert L.gyre_last_launch_count() == before
