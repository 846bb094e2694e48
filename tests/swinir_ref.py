"""CPU reference for the SwinIR upscaler tests (imported by the tests, not collected).

net(sd, cfg, x, store)   the reference's SwinIR.forward (gyre/pipeline/upscalers/models/network_swinir.py, upsampler "nearest+conv")
                         over torch.nn.functional in fp32, the same operations in the same order.  With store = a 16-bit dtype, the
                         matrix / convolution weights and every tensor the native graph keeps in memory are rounded to it (biases, norm
                         parameters and the position table stay fp32, as in the weight store): the emulation whose distance from the
                         fp32 net sets the model gates.  Like the native graph, an image of one window per side (H == 8 or W == 8) is
                         not shifted.
case(...)                random data for ONE call of the window-attention kernel (kernels_swin.hip k_win_attn)
value64 / bound / emulate    float64 value, element-wise error bound, fp32 host emulation of such a call; MISTAKES: seeded errors of
                         the emulation, for the self-test of the bound

The call.  qkv [B H W, ld_qkv] in token order, q / k / v of head h at columns 32 h / 32 (heads + h) / 32 (2 heads + h) (30 live, 2
zero); token (i, j) of window (wy, wx) under shift s is pixel ((8 wy + i + s) mod H, (8 wx + j + s) mod W);
    l[a][b] = c (q_a . k_b) + bias[h][a][b] + mask[a][b],  c = fl32(30^-1/2),  mask = -100 where the region ids differ and s > 0
    p = softmax_b(l) in fp32, rounded to storage;  o[a] = sum_b p[a][b] v_b, rounded once to storage, head h at columns [30 h, 30 h + 30)

Error bound.  u = 2^-8 (bf16) or 2^-11 (fp16), fl = half the smallest storage subnormal (2^-134, 2^-25), e = 2^-24.  q, k, v are storage
values, so every product is exact in fp32.  With A = sum_d |q_a,d| |k_b,d| and L = |c (q . k)| + |bias| + |mask|:
    logit        dl[a][b] <= c 2 32 e A + 3 e L        (accumulation of 32 products, doubled like tests/gemm_ref.py because the adder
                                                         tree inside the MFMA is not documented; the fma, the mask addition and one spare)
    exponent     x = l - m carries dl of its own logit, dl of the maximum (D[a] = max_b dl[a][b] covers both) and e |x| of the
                 subtraction; exp(x) as exp2(x log2 e): e |x| from the product and 2 e from v_exp_f32; so the relative error of the
                 exponential is  r[a][b] = 2 D[a] + 2 e |x| + 4 e
    row sum      relative error  R[a] = sum_b p r + 64 e   (the p-weighted mean of the terms' errors, plus the 64 additions)
    probability  p = exp / sum: relative  r + R + 4 e  (reciprocal and product), absolute 2^-126 more where the exponential of a
                 masked pair (about e^-100) is flushed to zero; rounding to storage adds u p + fl:
                     dp[a][b] = p (r + R + 4 e) (1 + u) + u p + fl + 2^-126
    output       t[a][d] = sum_b dp |v_b,d| + 2 64 e sum_b p |v_b,d|       (the error of P, then the accumulation of 64 exact products)
    bound = t + u (|E| + t) + fl                                          (one rounding to storage of something within t of E)
"""
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
E = 2.0 ** -24
MEAN = (0.4488, 0.4371, 0.4040)
# (B, H, W, heads, shift) of the GPU list (tests/test_gpu_swin_kernels.py): 2 x 3 windows with interior, last-row, last-column and corner
# windows; a tall image with 6 heads; one window and 8 heads; a square image
CASES = [(2, 16, 24, 2, 0), (2, 16, 24, 2, 4), (1, 24, 16, 6, 4), (1, 8, 8, 8, 0), (1, 16, 16, 6, 4)]
MISTAKES = ("shift_sign_flipped", "reverse_shift_dropped", "bias_transposed", "mask_omitted", "mask_hw_swapped", "scale_after_bias")


def f32(v):
    """the float32 number nearest to v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


SCALE = f32(30.0 ** -0.5)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------------ window helpers
def window_partition(x, ws=8):
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def window_reverse(windows, ws, H, W):
    B = int(windows.shape[0] / (H * W / ws / ws))
    x = windows.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def relative_position_index(ws=8):
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def calculate_mask(H, W, shift, ws=8):
    """SwinTransformerBlock.calculate_mask: [nW, 64, 64] of 0 / -100"""
    img = torch.zeros((1, H, W, 1))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))


def region_mask(H, W, shift, swapped=False):
    """the same mask from the closed form the kernel uses: id = 3 r(8 wy + i, H) + r(8 wx + j, W), r(Y, L) = 0 if Y < L - 8, 1 if
    Y < L - shift, else 2.  swapped: the two lengths exchanged (a seeded mistake)"""
    def r(Y, L):
        return (Y >= L - 8).long() + (Y >= L - shift).long()
    LH, LW = (W, H) if swapped else (H, W)
    ids = 3 * r(torch.arange(H), LH)[:, None] + r(torch.arange(W), LW)[None, :]
    mw = window_partition(ids.view(1, H, W, 1).float()).view(-1, 64)
    return torch.where(mw.unsqueeze(1) != mw.unsqueeze(2), -100.0, 0.0)


def expanded_bias(table):
    """table [225, heads] -> [heads, 64, 64]: bias[h][a][b] = table[index[a][b]][h]"""
    return table[relative_position_index().view(-1)].view(64, 64, -1).permute(2, 0, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------- the network
def net(sd, cfg, x, store=None, compute=torch.float32):
    """compute: the dtype every operation runs in (fp32 for the tests; tools/swinir_time.py times the same code in fp16 on the GPU)"""
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: fl(t.to(store)))
    wt = lambda name: q(fl(sd[name + ".weight"]))
    bs = lambda name: fl(sd[name + ".bias"])
    C, heads, scale_up = cfg["embed_dim"], cfg["num_heads"], cfg["upscale"]
    three = cfg["resi_connection"] == "3conv"
    index = relative_position_index().to(x.device)

    def c3(t, name):
        return F.conv2d(t, wt(name), bs(name), stride=1, padding=1)

    def lin(t, name):
        return F.linear(t, wt(name), bs(name))

    def norm(t, name):
        return F.layer_norm(t, (C,), fl(sd[name + ".weight"]), fl(sd[name + ".bias"]), 1e-5)

    def resi(t, name, add):
        """the 1conv / 3conv block on an image, plus `add`; every stored intermediate rounded"""
        if not three:
            return q(c3(t, name) + add)
        t = q(F.leaky_relu(q(c3(t, name + ".0")), 0.2))
        t = q(F.leaky_relu(q(F.conv2d(t, wt(name + ".2"), bs(name + ".2"))), 0.2))
        return q(c3(t, name + ".4") + add)

    def attention(xw, p, nh, mask):
        B_, N, _ = xw.shape
        qkv = q(lin(xw, p + ".qkv")).reshape(B_, N, 3, nh, C // nh).permute(2, 0, 3, 1, 4)
        qq, kk, vv = qkv[0], qkv[1], qkv[2]
        qq = qq * (C // nh) ** -0.5
        attn = qq @ kk.transpose(-2, -1)
        bias = fl(sd[p + ".relative_position_bias_table"])[index.view(-1)].view(64, 64, -1).permute(2, 0, 1).contiguous()
        attn = attn + bias.unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = attn.view(B_ // nW, nW, nh, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, nh, N, N)
        attn = q(torch.softmax(attn, dim=-1))
        return q((attn @ vv).transpose(1, 2).reshape(B_, N, C))

    def block(t, p, nh, shift, H, W):
        B = t.shape[0]
        shortcut = t
        t = q(norm(t, p + ".norm1")).view(B, H, W, C)
        if shift > 0:
            t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
        xw = window_partition(t).view(-1, 64, C)
        aw = attention(xw, p + ".attn", nh, fl(calculate_mask(H, W, shift)).to(t.device) if shift > 0 else None)
        aw = lin(aw, p + ".attn.proj")
        t = window_reverse(aw.view(-1, 8, 8, C), 8, H, W)
        if shift > 0:
            t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
        t = q(shortcut + t.view(B, H * W, C))
        h = q(lin(q(norm(t, p + ".norm2")), p + ".mlp.fc1"))
        return q(t + lin(q(F.gelu(h)), p + ".mlp.fc2"))

    H0, W0 = x.shape[2:]
    x = F.pad(fl(x), (0, -W0 % 8, 0, -H0 % 8), "reflect")
    H, W = x.shape[2:]
    mean = torch.Tensor(MEAN).view(1, 3, 1, 1).to(x)
    t = q((x - mean) * cfg["img_range"])
    first = q(c3(t, "conv_first"))
    t = q(norm(first.flatten(2).transpose(1, 2), "patch_embed.norm"))
    for i, depth in enumerate(cfg["depths"]):
        keep = t
        for j in range(depth):
            shift = 4 if j % 2 and H > 8 and W > 8 else 0
            t = block(t, f"layers.{i}.residual_group.blocks.{j}", heads[i], shift, H, W)
        img = t.transpose(1, 2).view(-1, C, H, W)
        if three:
            t = resi(img, f"layers.{i}.conv", keep.transpose(1, 2).view(-1, C, H, W)).flatten(2).transpose(1, 2)
        else:
            t = q(c3(img, f"layers.{i}.conv").flatten(2).transpose(1, 2) + keep)
    t = q(norm(t, "norm")).transpose(1, 2).view(-1, C, H, W)
    t = resi(t, "conv_after_body", first)
    t = q(F.leaky_relu(q(c3(t, "conv_before_upsample.0")), 0.01))
    t = q(F.leaky_relu(q(c3(F.interpolate(t, scale_factor=2, mode="nearest"), "conv_up1")), 0.2))
    if scale_up == 4:
        t = q(F.leaky_relu(q(c3(F.interpolate(t, scale_factor=2, mode="nearest"), "conv_up2")), 0.2))
    t = q(c3(q(F.leaky_relu(q(c3(t, "conv_hr")), 0.2)), "conv_last"))
    t = q(t / cfg["img_range"] + mean)
    return t[:, :, :H0 * scale_up, :W0 * scale_up]


# ------------------------------------------------------------------------------------------------------------ one kernel call
def case(sdt, B, H, W, heads, shift, seed=0, pad_cols=8):
    """qkv with q, k, v ~ N(0, 1) rounded to sdt (columns 30, 31 of every group zero, `pad_cols` NaN columns behind the last group), a
    bias table of std 1 (the initialiser's 0.02 would let every bias mistake pass), o NaN-filled with stride 30 heads + pad_cols"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * H + 7 * W + 3 * heads + shift)
    rows = B * H * W
    qkv = torch.randn((rows, 3 * heads, 32), generator=g)
    qkv[:, :, 30:] = 0
    qkv = torch.cat([qkv.view(rows, 96 * heads), torch.full((rows, pad_cols), float("nan"))], 1).to(sdt)
    table = torch.randn((225, heads), generator=g)
    o = torch.full((rows, 30 * heads + pad_cols), float("nan")).to(sdt)
    return dict(qkv=qkv, table=table, o=o, B=B, H=H, W=W, heads=heads, shift=shift)


def _windows(L, dt, shift_sign=1):
    """q, k, v [B nW, heads, 64, 30] of the call in dtype dt"""
    B, H, W, nh, s = L["B"], L["H"], L["W"], L["heads"], L["shift"]
    t = L["qkv"][:, :96 * nh].to(dt).view(B, H, W, 96 * nh)
    if s:
        t = torch.roll(t, shifts=(-s * shift_sign, -s * shift_sign), dims=(1, 2))
    w = window_partition(t).view(-1, 64, 3, nh, 32)[..., :30].permute(2, 0, 3, 1, 4)
    return w[0], w[1], w[2]


def _unwindow(L, ow, reverse=True):
    """[B nW, heads, 64, 30] -> [B H W, 30 heads] in token order"""
    B, H, W, nh, s = L["B"], L["H"], L["W"], L["heads"], L["shift"]
    t = window_reverse(ow.transpose(1, 2).reshape(-1, 8, 8, 30 * nh), 8, H, W)
    if s and reverse:
        t = torch.roll(t, shifts=(s, s), dims=(1, 2))
    return t.reshape(B * H * W, 30 * nh)


def _mask(L, dt):
    if not L["shift"]:
        return None
    nW = (L["H"] // 8) * (L["W"] // 8)
    return calculate_mask(L["H"], L["W"], L["shift"]).to(dt).repeat(L["B"], 1, 1).view(L["B"] * nW, 1, 64, 64)


def value64(L):
    """(E, t): float64 value of the live columns [B H W, 30 heads] and the error t of the bound before the output rounding"""
    d = torch.float64
    sdt = L["o"].dtype
    u, fl = U[sdt], FL[sdt]
    qq, kk, vv = _windows(L, d)
    bias = expanded_bias(L["table"].double()).unsqueeze(0)
    dot = qq @ kk.transpose(-2, -1)
    A = qq.abs() @ kk.abs().transpose(-2, -1)
    l = SCALE * dot + bias
    Lm = (SCALE * dot).abs() + bias.abs()
    m = _mask(L, d)
    if m is not None:
        l = l + m
        Lm = Lm + m.abs()
    dl = SCALE * 2 * 32 * E * A + 3 * E * Lm
    D = dl.amax(-1, keepdim=True)
    x = l - l.amax(-1, keepdim=True)
    p = torch.softmax(l, dim=-1)
    r = 2 * D + 2 * E * x.abs() + 4 * E
    R = (p * r).sum(-1, keepdim=True) + 64 * E
    dp = p * (r + R + 4 * E) * (1 + u) + u * p + fl + 2.0 ** -126
    val = p @ vv
    t = dp @ vv.abs() + 2 * 64 * E * (p @ vv.abs())
    return _unwindow(L, val), _unwindow(L, t)


def bound(L):
    sdt = L["o"].dtype
    v, t = value64(L)
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def emulate(L, mistake=None):
    """the output buffer after the call, computed on the host in fp32 with the kernel's roundings (mistake: one of MISTAKES)"""
    assert mistake is None or mistake in MISTAKES
    sdt = L["o"].dtype
    f = torch.float32
    qq, kk, vv = _windows(L, f, shift_sign=-1 if mistake == "shift_sign_flipped" else 1)
    bias = expanded_bias(L["table"].float()).unsqueeze(0)
    if mistake == "bias_transposed":
        bias = bias.transpose(-2, -1)
    c = torch.tensor(SCALE, dtype=f)
    dot = qq @ kk.transpose(-2, -1)
    l = (dot + bias) * c if mistake == "scale_after_bias" else c * dot + bias
    if L["shift"] and mistake != "mask_omitted":
        nW = (L["H"] // 8) * (L["W"] // 8)
        m = region_mask(L["H"], L["W"], L["shift"], swapped=mistake == "mask_hw_swapped")
        l = l + m.repeat(L["B"], 1, 1).view(L["B"] * nW, 1, 64, 64)
    p = torch.softmax(l, dim=-1).to(sdt).float()
    ow = (p @ vv).to(sdt).float()
    buf = L["o"].clone()
    buf[:, :30 * L["heads"]] = _unwindow(L, ow, reverse=mistake != "reverse_shift_dropped").to(sdt)
    return buf


def verdict(L, got):
    """(worst |got - E| / bound over the live columns, True when every other element still has the bits it had)"""
    v, bd = bound(L)
    n = 30 * L["heads"]
    worst = float(((got[:, :n].double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    return worst, torch.equal(bits(got)[:, n:], bits(L["o"])[:, n:])


# ------------------------------------------------------------------------------------------------------ the element-wise pieces
def gelu64(x):
    return 0.5 * x.double() * (1.0 + torch.erf(x.double() * 0.5 ** 0.5))


def act_ref(x, mode, slope):
    """(ref, bound) of launch_swin_act on storage values x.  Leaky ReLU: one fp32 product of exact operands - its value is within
    e |ref| of the float64 one, then one rounding.  GELU: x / sqrt 2 (1 rounding, moving erf by at most |x| e erf' <= 0.5 e in
    absolute terms ...), erff (a few ulp: 4), 1 + . (1), 0.5 x (exact) and the product (1): relative to |x| >= |gelu(x)|, 8 e |x| in all
    - measured against |x| because near the negative tail 1 + erf cancels."""
    if mode == 0:
        return gelu64(x), 8 * E * x.double().abs()
    v = x.double()
    ref = torch.where(v > 0, v, f32(slope) * v)
    return ref, E * ref.abs()


def act_bound(x, mode, slope):
    ref, t = act_ref(x, mode, slope)
    return ref, t + U[x.dtype] * (ref.abs() + t) + FL[x.dtype]


def entry_ref(x, img_range, sdt):
    """x [B, 3, HW] -> (ref [B, HW, 8], bound): (x - mean) * range, two fp32 roundings relative to (|x| + |mean|) range, one rounding to storage"""
    mean = torch.tensor([f32(m) for m in MEAN], dtype=torch.float64).view(1, 3, 1)
    r = f32(img_range)
    v = (x.double() - mean) * r
    t = 2 * E * (x.double().abs() + mean) * r
    B = x.shape[0]
    pad = lambda a: F.pad(a.reshape(B, 3, -1).transpose(1, 2), (0, 5))
    v, t = pad(v), pad(t)
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt] * (v != 0)


def exit_ref(x, img_range, odt):
    """(ref [B, 3, HW], bound) of x [B, HW, ld] storage: x / range + mean, two fp32 roundings, one rounding to the output dtype"""
    mean = torch.tensor([f32(m) for m in MEAN], dtype=torch.float64).view(1, 3, 1)
    r = f32(img_range)
    v = x[..., :3].double().transpose(1, 2) / r + mean
    t = 2 * E * (x[..., :3].double().transpose(1, 2).abs() / r + mean)
    uo = U.get(odt, E)
    return v, t + uo * (v.abs() + t) + FL.get(odt, 2.0 ** -150)


# ------------------------------------------------------------------------------------------------------------- model test cases
# name -> (keywords of gyre_amd.config.tiny_swinir, image shape): the two tiny configurations, and one block pair at each real width
# (180 -> 192 and 240 -> 256 padded channels)
MODEL_CASES = {"tiny": (dict(), (2, 3, 16, 24)),
               "tiny3": (dict(embed_dim=120, num_heads=[4], depths=[2], resi_connection="3conv", upscale=2), (2, 3, 16, 24)),
               "w180": (dict(embed_dim=180, num_heads=[6], depths=[2]), (1, 3, 16, 16)),
               "w240": (dict(embed_dim=240, num_heads=[8], depths=[2], resi_connection="3conv"), (1, 3, 16, 24))}


def model_case(name):
    """(cfg, state dict, image) of a MODEL_CASES entry: synthetic N(0, 1 / fan_in) weights, the position tables at std 1"""
    from gyre_amd import config as gcfg, weights
    kw, shape = MODEL_CASES[name]
    cfg = gcfg.tiny_swinir(**kw)
    shapes = {k: v for k, v in weights.swinir_param_shapes(cfg).items() if not weights.swinir_is_buffer(k)}
    sd = weights.synthetic_state_dict(shapes)
    for k in sd:
        if k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(len(k)))
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0))
    return cfg, sd, x
