"""CPU reference for the kernels of the token-sequence T2I networks (kernels_seq.hip; imported by the tests, not collected).

attn_case(...)                          random data for ONE call of k_seq_attn
value64 / bound / emulate / verdict     float64 value, element-wise error bound and fp32 host emulation of such a call; MISTAKES["attn"]:
                                        seeded errors of the emulation, for the self-test of the bound
quick_gelu_ref                          (float64 value, bound) of the in-place QuickGELU; quick_gelu_emulate with the seeded "erf_gelu"
pool_ref / pool_emulate                 (float64 value, bound) of k_fuser_pool; seeded "padded_pixel_count"
gain_expr                               the fp32 expression k_fuser_gain equals bit for bit; seeded "alpha_without_one"

The attention call.  qkv [N L, ld_qkv] storage, sample-major rows (row n L + l; the reference's [L, N, E] of nn.MultiheadAttention is the
same data in another view order), q / k / v of head h at columns h D / W + h D / 2 W + h D with W = heads D: the packed in_proj output.
    l[a][b] = c (q_a . k_b),  c = fl32(D^-1/2);  p = softmax_b(l) over the L keys of the sample in fp32, rounded to storage
    o[a] = sum_b p[a][b] v_b, rounded once to storage, head h at columns [h D, h D + D)

Error bound: the derivation of tests/hat_ref.py with its 32 products per dot replaced by D, its nk by L, and without bias and mask.
u = 2^-8 (bf16) or 2^-11 (fp16), fl = half the smallest storage subnormal (2^-134, 2^-25), e = 2^-24.  q, k, v are storage values, so
every product is exact in fp32.  With A = sum_d |q_a,d| |k_b,d| and Lm = |c (q . k)|:
    logit        dl[a][b] <= c 2 D e A + 3 e Lm         (accumulation of D products, doubled because the adder tree inside the MFMA is
                                                          not documented; the product with c and two spare)
    exponent     r[a][b] = 2 Dm[a] + 2 e |x| + 4 e,  x = l - M,  Dm[a] = max_b dl[a][b]
    row sum      two-pass, running maximum over T = ceil(L / 32) + 2 factors:  R[a] = sum_b p (2 Dm + 2 e |x|) + 5 e T + L e
    probability  dp[a][b] = p (r + R + 4 e) (1 + u) + u p + fl + 2^-126
    output       t[a][d] = sum_b dp |v_b,d| + 2 L e sum_b p |v_b,d|;   bound = t + u (|E| + t) + fl

QuickGELU  y = x s, s = 1 / (1 + exp(-z)), z = c x with c = fl32(1.702) (torch multiplies an fp32 tensor by the fp32 constant).  The
product z: e |z| relative in the exponential; expf 2 e; the addition, the division and the product with x one e each:
    t = |x| s ((1 - s) (|z| + 2) e + 3 e) + 2^-126;   bound = t + u (|E| + t) + fl
(d s / s = (1 - s) d exp / exp.)  At the end of the fp16 range s is exactly 1 or the quotient is exactly -0: nothing leaves the range.

Pool  m = mean over h w; lane i adds elements i, i + 64, ... (ceil(hw / 64) additions), six tree levels, one division:
    dm <= (ceil(hw / 64) + 7) e mean|x|
out = silu(m) = m s(m) through exp2 and the hardware reciprocal (1 ulp each; |silu'| <= 1.1):
    t = 1.1 dm + |silu| ((1 - s) (2 |m| + 2) e + 4 e) + |m| 2^-126;   bound = t + u (|E| + t) + fl
"""
import math

import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
E = 2.0 ** -24
# (N, heads, L, D): one key; two samples and two heads on a few keys; D = 96 below one tile; 63 / 64 / 65 around the 64-query block
# and the 32-key tile; the style adapter on CLIP ViT-L/14 (257 + 8 tokens, 8 heads of 128: five query blocks, the LDS limit's case)
ATTN_CASES = [(1, 1, 1, 32), (2, 2, 4, 32), (1, 2, 12, 96), (2, 1, 63, 64), (1, 2, 64, 96), (1, 1, 65, 128), (1, 8, 265, 128)]
MAX_LEN = {32: 1120, 64: 576, 96: 384, 128: 288}          # K and V of one head in 160 KiB of LDS (kernels_seq.hip)
MISTAKES = {"attn": ("scale_dropped", "q_against_next_head", "k_v_swapped", "padded_keys_in_softmax", "n_l_swapped"),
            "quick_gelu": ("erf_gelu",), "pool": ("padded_pixel_count",), "gain": ("alpha_without_one",)}


def f32(v):
    """the float32 number nearest to v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# -------------------------------------------------------------------------------------------------------------- k_seq_attn
def attn_case(sdt, N, heads, L, D, seed=0, pad_cols=8, pad_rows=3):
    """qkv with q, k, v ~ N(0, 1) rounded to sdt, `pad_cols` NaN columns behind the 3 W live ones and `pad_rows` NaN rows behind the
    N L live ones; o NaN-filled with stride W + pad_cols and the same spare rows"""
    g = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * heads + 3 * L + D)
    W = heads * D
    qkv = torch.full((N * L + pad_rows, 3 * W + pad_cols), float("nan"))
    qkv[:N * L, :3 * W] = torch.randn((N * L, 3 * W), generator=g)
    o = torch.full((N * L + pad_rows, W + pad_cols), float("nan"))
    return dict(qkv=qkv.to(sdt), o=o.to(sdt), N=N, heads=heads, L=L, D=D)


def _operands(c, dt, l_major=False):
    """q, k, v [N, heads, L, D] of the call in dtype dt.  l_major: the rows read as l N + n (a seeded mistake)"""
    N, nh, L, D = c["N"], c["heads"], c["L"], c["D"]
    t = c["qkv"][:N * L, :3 * nh * D].to(dt)
    t = t.view(L, N, 3, nh, D).permute(2, 1, 3, 0, 4) if l_major else t.view(N, L, 3, nh, D).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _rows(c, ow, l_major=False):
    """[N, heads, L, D] -> [N L, W] in the row order of the call"""
    N, nh, L, D = c["N"], c["heads"], c["L"], c["D"]
    return (ow.permute(2, 0, 1, 3) if l_major else ow.permute(0, 2, 1, 3)).reshape(N * L, nh * D)


def value64(c):
    """(E, t): float64 value of the live elements [N L, W] and the error t of the bound before the output rounding"""
    d = torch.float64
    sdt = c["o"].dtype
    u, fl = U[sdt], FL[sdt]
    L, D = c["L"], c["D"]
    sc = f32(D ** -0.5)
    qq, kk, vv = _operands(c, d)
    T = math.ceil(L / 32) + 2
    dot = qq @ kk.transpose(-2, -1)
    A = qq.abs() @ kk.abs().transpose(-2, -1)
    l = sc * dot
    dl = sc * 2 * D * E * A + 3 * E * l.abs()
    Dm = dl.amax(-1, keepdim=True)
    x = l - l.amax(-1, keepdim=True)
    p = torch.softmax(l, dim=-1)
    r = 2 * Dm + 2 * E * x.abs() + 4 * E
    R = (p * (2 * Dm + 2 * E * x.abs())).sum(-1, keepdim=True) + 5 * E * T + L * E
    dp = p * (r + R + 4 * E) * (1 + u) + u * p + fl + 2.0 ** -126
    val = p @ vv
    t = dp @ vv.abs() + 2 * L * E * (p @ vv.abs())
    return _rows(c, val), _rows(c, t)


def bound(c):
    sdt = c["o"].dtype
    v, t = value64(c)
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def emulate(c, mistake=None):
    """the output buffer after the call, computed on the host in fp32 with the kernel's roundings (mistake: one of MISTAKES["attn"])"""
    assert mistake is None or mistake in MISTAKES["attn"]
    sdt, f = c["o"].dtype, torch.float32
    N, nh, L, D = c["N"], c["heads"], c["L"], c["D"]
    lm = mistake == "n_l_swapped"
    qq, kk, vv = _operands(c, f, l_major=lm)
    if mistake == "q_against_next_head":
        kk = torch.roll(kk, shifts=-1, dims=1)
    if mistake == "k_v_swapped":
        kk, vv = vv, kk
    sc = torch.tensor(1.0 if mistake == "scale_dropped" else f32(D ** -0.5), dtype=f)
    l = sc * (qq @ kk.transpose(-2, -1))
    if mistake == "padded_keys_in_softmax":                  # the zero rows of the 32-key tiles take part with logit 0
        pad = -L % 32
        l, vv = F.pad(l, (0, pad)), F.pad(vv, (0, 0, 0, pad))
    p = torch.softmax(l, dim=-1).to(sdt).float()
    ow = (p @ vv).to(sdt).float()
    buf = c["o"].clone()
    buf[:N * L, :nh * D] = _rows(c, ow, l_major=lm).to(sdt)
    return buf


def verdict(c, got):
    """(worst |got - E| / bound over the live elements, True when every other element still has the bits it had)"""
    v, bd = bound(c)
    rows, cols = c["N"] * c["L"], c["heads"] * c["D"]
    worst = float(((got[:rows, :cols].double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[:rows, :cols] = False
    return worst, torch.equal(bits(got)[keep], bits(c["o"])[keep])


# ------------------------------------------------------------------------------------------------------------ k_quick_gelu
C1702 = f32(1.702)


def quick_gelu_points(sdt):
    """0, +-small (the smallest subnormal and normal numbers of the storage type, 1e-3), +-moderate, +-large and the end of the range
    of fp16 (65504; bf16 takes the nearest value, 65536), padded to a multiple of 8 with ones"""
    tiny = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}[sdt]
    norm = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}[sdt]
    pos = [tiny, norm, 1e-3, 0.25, 1.0, 3.0, 10.0, 20.0, 60.0, 100.0, 1000.0, 30000.0, 65504.0]
    v = [0.0, -0.0] + pos + [-p for p in pos]
    v += [1.0] * (-len(v) % 8)
    return torch.tensor(v, dtype=torch.float64).to(sdt)


def quick_gelu_ref(x):
    """(float64 value, bound) of x sigmoid(1.702 x) on storage values x"""
    sdt = x.dtype
    xd = x.double()
    z = C1702 * xd
    s = torch.sigmoid(z)
    v = xd * s
    t = xd.abs() * s * ((1 - s) * (z.abs() + 2) * E + 3 * E) + 2.0 ** -126
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def quick_gelu_emulate(x, mistake=None):
    xf = x.float()
    return (F.gelu(xf) if mistake == "erf_gelu" else xf * torch.sigmoid(torch.tensor(C1702, dtype=torch.float32) * xf)).to(x.dtype)


# ------------------------------------------------------------------------------------------------- k_fuser_pool, k_fuser_gain
POOL_CASES = [(2, 32, 1, 1), (1, 32, 3, 5), (2, 320, 3, 5), (1, 32, 8, 8), (2, 320, 8, 8), (1, 320, 1, 1)]      # (N, C, h, w)


def pool_case(sdt, N, C, h, w, seed=0):
    """an NCHW map ~ N(0, 1) + a per-channel offset (keeps the means away from zero), rounded to sdt"""
    g = torch.Generator().manual_seed(100 * seed + 7 * N + C + 3 * h + w)
    return (torch.randn((N, C, h, w), generator=g) + torch.randn((1, C, 1, 1), generator=g)).to(sdt)


def pool_ref(x):
    """(silu(mean) [N, C] float64, bound) of the storage map x [N, C, h, w]"""
    sdt = x.dtype
    hw = x.shape[2] * x.shape[3]
    xd = x.double()
    m = xd.mean((2, 3))
    dm = (math.ceil(hw / 64) + 7) * E * xd.abs().mean((2, 3))
    s = torch.sigmoid(m)
    v = m * s
    t = 1.1 * dm + v.abs() * ((1 - s) * (2 * m.abs() + 2) * E + 4 * E) + m.abs() * 2.0 ** -126
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def pool_emulate(x, mistake=None):
    xf = x.float()
    if mistake == "padded_pixel_count":                      # the sum divided by the pixel count rounded up to the 64 lanes
        hw = x.shape[2] * x.shape[3]
        m = xf.sum((2, 3)) / (math.ceil(hw / 64) * 64)
    else:
        m = xf.mean((2, 3))
    return F.silu(m).to(x.dtype)


def gain_expr(x, alpha, out=None, mistake=None):
    """x (alpha + 1) in fp32, each operation rounded on its own, (+ out), narrowed once: what k_fuser_gain gives bit for bit.
    x, out [N, C, h, w] storage, alpha [N, C] fp32"""
    g = alpha if mistake == "alpha_without_one" else alpha + 1.0
    v = x.float() * g[:, :, None, None]
    if out is not None:
        v = out.float() + v
    return v.to(x.dtype)


# ---------------------------------------------------------------------------------------------------------------- the networks
# style_net / fuser_net restate StyleAdapter.forward and CoAdapterFuser.forward (adapter.py:173-199, 266-343) with explicit attention
# (no nn.MultiheadAttention), in `compute` precision.  With store = a 16-bit dtype, the matrix weights and every tensor the native
# graphs keep in memory are rounded to it at the points csrc/model_t2i_seq.hip names: the emulation whose distance from the float64
# restatement sets the model gates.  mistake: one of NET_MISTAKES.
# (erf GELU for QuickGELU moves a whole net by less than its bf16 roundings do: it is seeded where it shows, at the kernel - MISTAKES)
NET_MISTAKES = ("task_index_off_by_one", "positional_embedding_dropped", "first_rows_instead_of_last", "alpha_without_one")
EXTRA_CONDITION = {"sketch": 0, "keypose": 1, "seg": 2, "depth": 3, "canny": 4, "style": 5, "color": 6, "openpose": 7}
STYLE_CASES = [(1, 1), (3, 5), (1, 50), (3, 1)]                      # (N, S) stored in tests/golden/t2i_seq_vectors.npz
# name -> [(condition, "spatial" | "tokens", T, seed)] in the caller's dict order; N = 2
FUSER_CASES = {"one_spatial": [("sketch", "spatial", 0, 41)],
               "two_spatial_one_style": [("canny", "spatial", 0, 42), ("style", "tokens", 3, 43), ("depth", "spatial", 0, 44)],
               "two_token_inputs": [("style", "tokens", 3, 45), ("color", "tokens", 2, 46)]}
FUSER_N, FUSER_HW = 2, [(4, 6), (2, 3), (1, 1), (1, 1)]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def style_input(N, S, width, seed=0):
    """CLIP-like hidden states [N, S, width] ~ N(0, 1)"""
    return torch.randn((N, S, width), generator=torch.Generator().manual_seed(7000 + 100 * seed + 10 * N + S))


def fuser_inputs(spec, cfg, N=FUSER_N, hw=None):
    """[(condition, four states [N, C_i, h_i, w_i] | tokens [N, T, width])] of a FUSER_CASES entry, fp32"""
    out = []
    for name, kind, T, seed in spec:
        g = torch.Generator().manual_seed(seed)
        if kind == "tokens":
            out.append((name, torch.randn((N, T, cfg["width"]), generator=g)))
        else:
            out.append((name, [torch.randn((N, c, h, w), generator=g) + 0.5 * torch.randn((1, c, 1, 1), generator=g)
                               for c, (h, w) in zip(cfg["unet_channels"], hw or FUSER_HW)]))
    return out


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * w + b


def _trunk(x, sd, cfg, q, fl, wt, mistake=None):
    """ln_pre and the ResidualAttentionBlocks over x [N, L, W]"""
    W, nh = cfg["width"], cfg["num_head"]
    D = W // nh
    N, L, _ = x.shape
    x = q(_ln(x, fl(sd["ln_pre.weight"]), fl(sd["ln_pre.bias"])))
    for i in range(cfg["n_layes"]):
        p = f"transformer_layes.{i}"
        h = q(_ln(x, fl(sd[p + ".ln_1.weight"]), fl(sd[p + ".ln_1.bias"])))
        qkv = q(h @ wt(p + ".attn.in_proj_weight").T + fl(sd[p + ".attn.in_proj_bias"])).view(N, L, 3, nh, D).permute(2, 0, 3, 1, 4)
        att = q(torch.softmax(f32(D ** -0.5) * (qkv[0] @ qkv[1].transpose(-2, -1)), dim=-1))
        o = q(att @ qkv[2]).permute(0, 2, 1, 3).reshape(N, L, W)
        x = q(x + o @ wt(p + ".attn.out_proj.weight").T + fl(sd[p + ".attn.out_proj.bias"]))
        h = q(_ln(x, fl(sd[p + ".ln_2.weight"]), fl(sd[p + ".ln_2.bias"])))
        f = q(h @ wt(p + ".mlp.c_fc.weight").T + fl(sd[p + ".mlp.c_fc.bias"]))
        f = q(f * torch.sigmoid(C1702 * f))
        x = q(x + f @ wt(p + ".mlp.c_proj.weight").T + fl(sd[p + ".mlp.c_proj.bias"]))
    return x


def _helpers(sd, store, compute):
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: t.to(store).to(compute))
    return fl, q, (lambda k: q(fl(sd[k])))


def style_net(sd, cfg, x, store=None, compute=torch.float32, mistake=None):
    """StyleAdapter.forward: x [N, S, width] -> [N, num_token, context_dim]"""
    fl, q, wt = _helpers(sd, store, compute)
    T = cfg["num_token"]
    t = q(torch.cat([fl(x), fl(sd["style_embedding"]).expand(x.shape[0], -1, -1)], dim=1))
    t = _trunk(t, sd, cfg, q, fl, wt, mistake)
    t = t[:, :T] if mistake == "first_rows_instead_of_last" else t[:, -T:]
    t = q(_ln(t, fl(sd["ln_post.weight"]), fl(sd["ln_post.bias"])))
    return q(t @ wt("proj"))


def fuser_net(sd, cfg, feats, store=None, compute=torch.float32, mistake=None):
    """CoAdapterFuser.forward over feats [(condition, states | tokens)]: (four summed gained maps | None, gained tokens | None)"""
    fl, q, wt = _helpers(sd, store, compute)
    task, pos = fl(sd["task_embedding"]), fl(sd["positional_embedding"])
    rows = []
    for name, v in feats:
        idx = EXTRA_CONDITION[name] + (1 if mistake == "task_index_off_by_one" else 0)
        if not isinstance(v, list):
            rows.append(q(fl(v) + task[idx]))
            continue
        seq = []
        for i, m in enumerate(v):
            vec = q(F.silu(q(fl(m)).mean((2, 3))))
            seq.append(q(vec @ wt(f"spatial_feat_mapping.{i}.1.weight").T + fl(sd[f"spatial_feat_mapping.{i}.1.bias"])))
        s = torch.stack(seq, dim=1) + task[idx]
        rows.append(q(s if mistake == "positional_embedding_dropped" else s + pos))
    x = _trunk(torch.cat(rows, dim=1), sd, cfg, q, fl, wt, mistake)
    x = q(_ln(x, fl(sd["ln_post.weight"]), fl(sd["ln_post.bias"])))
    one = 0.0 if mistake == "alpha_without_one" else 1.0
    maps, seq, cur = None, None, 0
    for name, v in feats:
        if not isinstance(v, list):
            T = v.shape[1]
            g = q(x[:, cur:cur + T] @ wt("seq_proj"))
            t = fl(v) * (g + one)
            seq = t if seq is None else torch.cat([seq, t], dim=1)
            cur += T
            continue
        new = []
        for i, m in enumerate(v):
            alpha = x[:, cur + i] @ wt(f"spatial_ch_projs.{i}.weight").T + fl(sd[f"spatial_ch_projs.{i}.bias"])
            new.append(q(fl(m)) * (alpha[:, :, None, None] + one))
        maps = [q(t) for t in new] if maps is None else [q(a + b) for a, b in zip(maps, new)]
        cur += 4
    return maps, seq


# ------------------------------------------------------------------------------------------------------------- hint conditioning
# name -> [(co-adapter condition | False, "spatial" | "tokens", T, seed, cfg_only)]: the hints of one request, for UNetWithT2I.__init__
# (gyre_amd.hints.build_t2i_conditioning).  A style hint that is no co-adapter returns tokens of the UNet's context width, which the
# tiny configurations make equal to the fuser's width.
HINT_CASES = {"style_alone": [(False, "tokens", 3, 61, True)],
              "one_spatial_coadapter": [("sketch", "spatial", 0, 62, False)],
              "two_spatial_one_style_coadapter": [("canny", "spatial", 0, 63, False), ("style", "tokens", 3, 64, False), ("depth", "spatial", 0, 65, False)],
              "same_type_twice": [("sketch", "spatial", 0, 66, True), ("sketch", "spatial", 0, 67, True), ("style", "tokens", 3, 68, True),
                                  ("style", "tokens", 3, 69, True)],
              "mixed_cfg_only": [("sketch", "spatial", 0, 70, True), ("depth", "spatial", 0, 71, False), ("style", "tokens", 3, 72, False)],
              "standard_and_coadapter": [(False, "spatial", 0, 73, True), ("color", "spatial", 0, 74, False), (False, "tokens", 2, 75, False)]}


def hint_states(kind, T, seed, cfg, N=1):
    """what a hint's call returns: four weighted states, or style tokens"""
    return fuser_inputs([("sketch", kind, T, seed)], cfg, N=N)[0][1]


def hint_context(B, width, S=7):
    return torch.randn((B, S, width), generator=torch.Generator().manual_seed(9000 + B))


# ------------------------------------------------------------------------------------------------------------------ the style hint
STYLE_LAYERS = ("final", "penultimate", 3)                           # clip_layer of the recorded style_call cases
STYLE_HINT_WEIGHT = 0.5
STYLE_EXTRACTOR = dict(image_mean=[0.48, 0.46, 0.41], image_std=[0.27, 0.26, 0.28], size={"shortest_edge": 8})


def style_hint_image():
    return torch.rand((1, 3, 12, 20), generator=torch.Generator().manual_seed(91))


class FakeVision:
    """a stand-in for CLIPModel.vision_model: seeded hidden states [1, 5, width], one per layer, and a last_hidden_state that is none
    of them; records the image it was given and whether every layer was asked for"""

    def __init__(self, width):
        g = torch.Generator().manual_seed(92)
        self.hidden = [torch.randn((1, 5, width), generator=g) for _ in range(5)]
        self.last = torch.randn((1, 5, width), generator=g)

    def __call__(self, image, output_hidden_states=False, return_dict=True):
        from types import SimpleNamespace
        self.seen, self.asked_all = image, bool(output_hidden_states)
        return SimpleNamespace(last_hidden_state=self.last, hidden_states=self.hidden if output_hidden_states else None)
