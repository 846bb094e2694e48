"""CPU reference for the HAT upscaler tests (imported by the tests, not collected).

net(sd, cfg, x, store)   the reference's HAT.forward (gyre/pipeline/upscalers/models/hat_arch.py, upsampler "pixelshuffle", "1conv")
                         over torch.nn.functional in fp32, the same operations in the same order.  With store = a 16-bit dtype, the
                         matrix / convolution weights and every tensor the native graph keeps in memory are rounded to it (biases, norm
                         parameters, the position tables and the two 1 x 1 convolutions of the channel attention stay fp32, as in the
                         weight store): the emulation whose distance from the fp32 net sets the model gates.
case(...)                random data for ONE call of the attention kernel (kernels_hat.hip k_hat_attn), mode "sa" or "oca"
value64 / bound / emulate / verdict    float64 value, element-wise error bound, fp32 host emulation of such a call; MISTAKES: seeded
                         errors of the emulation, for the self-test of the bound
cab_case / cab_value64 / cab_emulate / cab_verdict    the same for pool -> gate -> scale-add (the CAB entries of MISTAKES are seeded
                         there: at 0.01 of the residual stream they are too small to hold at the level of the net); pool_ref, gate_ref

The attention call.  qkv [B H W, ld_qkv] in token order, q / k / v of head h at columns 32 h / 32 (heads + h) / 32 (2 heads + h) (30
live, 2 zero).  SA: token (i, j) of window (wy, wx) under shift s is pixel ((16 wy + i + s) mod H, (16 wx + j + s) mod W), 256 keys, bias
table[(i - i' + 15) 31 + (j - j' + 15)], mask -100 where the region ids differ and s > 0.  OCA: query (i, j) is pixel (16 wy + i, 16 wx + j),
key (ey, ex) is pixel (16 wy - 4 + ey, 16 wx - 4 + ex) with k = v = 0 outside the image, 576 keys, bias table[((ey - i - 7) 39 + (ex - j - 7))
mod 1521].
    l[a][b] = c (q_a . k_b) + bias[h][a][b] + mask[a][b],  c = fl32(30^-1/2)
    p = softmax_b(l) in fp32, rounded to storage;  o[a] = sum_b p[a][b] v_b, rounded once to storage, head h at columns [30 h, 30 h + 30)

Error bound, derived as in tests/swinir_ref.py with its 64 keys replaced by nk = 256 / 576 and one more term for the kernel's two-pass
softmax.  u = 2^-8 (bf16) or 2^-11 (fp16), fl = half the smallest storage subnormal (2^-134, 2^-25), e = 2^-24.  q, k, v are storage
values, so every product is exact in fp32.  With A = sum_d |q_a,d| |k_b,d| and L = |c (q . k)| + |bias| + |mask|:
    logit        dl[a][b] <= c 2 32 e A + 3 e L        (accumulation of 32 products, doubled like tests/gemm_ref.py because the adder
                                                         tree inside the MFMA is not documented; the fma, the mask addition and one spare)
    exponent     x = l - M carries dl of its own logit, dl of the maximum (D[a] = max_b dl[a][b] covers both) and e |x| of the
                 subtraction; exp(x) as exp2(x log2 e): e |x| from the product and 2 e from v_exp_f32; so the relative error of the
                 exponential is  r[a][b] = 2 D[a] + 2 e |x| + 4 e
    row sum      the kernel's first pass adds exp(l - m) under a running maximum m and multiplies the sum by exp(m_old - m_new) when a
                 tile raises it, then merges the two lanes of a query the same way: a term reaches the sum as a product of at most
                 T = nk / 32 + 2 exponentials whose arguments are all <= 0 and add up to l - M exactly (each m cancels), so the
                 argument-proportional part of the error is still 2 e |x| and the constant part grows from 4 e to 5 e T (2 e of the
                 instruction, e of the subtraction, e of the product, one spare - per factor).  Relative error of the sum
                     R[a] = sum_b p (2 D + 2 e |x|) + 5 e T + nk e     (p-weighted mean of the terms' errors, plus the nk additions)
    probability  p = exp / sum: relative  r + R + 4 e  (reciprocal and product), absolute 2^-126 more where the exponential of a
                 masked pair (about e^-100) is flushed to zero; rounding to storage adds u p + fl:
                     dp[a][b] = p (r + R + 4 e) (1 + u) + u p + fl + 2^-126
    output       t[a][d] = sum_b dp |v_b,d| + 2 nk e sum_b p |v_b,d|       (the error of P, then the accumulation of nk exact products)
    bound = t + u (|E| + t) + fl                                          (one rounding to storage of something within t of E)

The CAB passes.  pool: HW storage values per channel added in fp32 in chains of at most 8 + 8 + ceil(HW / 64) additions, one division:
dpool <= (ceil(HW / 64) + 18) e mean|x|.  gate: h = relu(b1 + W1 pool) as a chain of C fmas, z = b2 + W2 h as a chain of C / 30,
s = scale / (1 + exp(-z)) (libm expf: 2 e; the addition, the division and the product: 3 e; one spare):
    dh <= |W1| dpool + (C + 1) e (|b1| + |W1| |pool|);  dz <= |W2| dh + (Cs + 1) e (|b2| + |W2| |h|);  ds <= s (1 - sigmoid) dz + 6 e s
(d sigmoid / dz = sigmoid (1 - sigmoid)).  scale-add: one fma of storage values and s, t = |c2| ds + e |y + c2 s|, then the storage
rounding  t + u (|E| + t) + fl.
"""
import math

import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
E = 2.0 ** -24
MEAN = (0.4488, 0.4371, 0.4040)
WS, SHIFT, OWS, PAD = 16, 8, 24, 4
# (B, H, W, heads, shift) of the GPU list (tests/test_gpu_hat_kernels.py).  SA: 1 x 2 windows unshifted; 2 x 3 windows with interior,
# last-row, last-column and corner windows; one window that wraps onto itself, 6 heads; a tall image with 8 heads.  OCA: 2 x 3 windows;
# one window padded on every side, 6 heads; 3 x 3 windows whose centre has no padding, 1 head
SA_CASES = [(2, 16, 32, 2, 0), (2, 32, 48, 2, 8), (1, 16, 16, 6, 8), (1, 48, 32, 8, 8)]
OCA_CASES = [(2, 32, 48, 2), (1, 16, 16, 6), (1, 48, 48, 1)]
CASES = [("sa",) + c for c in SA_CASES] + [("oca",) + c + (0,) for c in OCA_CASES]
MISTAKES = {"sa": ("shift_sign_flipped", "reverse_shift_dropped", "bias_transposed", "mask_omitted", "mask_hw_swapped", "scale_after_bias",
                   "one_window_not_shifted"),
            "oca": ("pad_keys_excluded", "pad_keys_clamped", "pad_keys_biased", "index_not_wrapped", "origin_not_centred", "bias_transposed"),
            "cab": ("pool_per_window", "conv_scale_dropped", "sigmoid_dropped")}


def f32(v):
    """the float32 number nearest to v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


SCALE = f32(30.0 ** -0.5)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------------ window helpers
def window_partition(x, ws=WS):
    b, h, w, c = x.shape
    x = x.view(b, h // ws, ws, w // ws, ws, c)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, c)


def window_reverse(windows, ws, h, w):
    b = int(windows.shape[0] / (h * w / ws / ws))
    x = windows.view(b, h // ws, w // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(b, h, w, -1)


def rpi_sa(ws=WS):
    """HAT.calculate_rpi_sa: [256, 256]"""
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def rpi_oca(ws=WS, ext=OWS):
    """HAT.calculate_rpi_oca: [256, 576], negative for most pairs"""
    ori = torch.flatten(torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")), 1)
    big = torch.flatten(torch.stack(torch.meshgrid([torch.arange(ext), torch.arange(ext)], indexing="ij")), 1)
    rel = (big[:, None, :] - ori[:, :, None]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - ext + 1
    rel[:, :, 1] += ws - ext + 1
    rel[:, :, 0] *= ws + ext - 1
    return rel.sum(-1)


def sa_index_closed():
    """the kernel's form: (i - i' + 15) 31 + (j - j' + 15) for query a = 16 i + j, key b = 16 i' + j'"""
    a, b = torch.arange(256)[:, None], torch.arange(256)[None, :]
    return ((a >> 4) - (b >> 4) + 15) * 31 + ((a & 15) - (b & 15) + 15)


def oca_index_closed(wrapped=True, transposed=False):
    """the kernel's form: ((ey - i - 7) 39 + (ex - j - 7)) mod 1521 for query 16 i + j, key 24 ey + ex.  wrapped=False: negative
    indices clamped to 0; transposed: the two axes exchanged (seeded mistakes)"""
    a, b = torch.arange(256)[:, None], torch.arange(576)[None, :]
    dy, dx = b // 24 - (a >> 4) - 7, b % 24 - (a & 15) - 7
    idx = dx * 39 + dy if transposed else dy * 39 + dx
    return torch.where(idx < 0, idx + 1521, idx) if wrapped else idx.clamp_min(0)


def calculate_mask(H, W, ws=WS, shift=SHIFT):
    """HAT.calculate_mask: [nW, 256, 256] of 0 / -100"""
    img = torch.zeros((1, H, W, 1))
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img, ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(-100.0)).masked_fill(m == 0, float(0.0))


def region_mask(H, W, swapped=False):
    """the same mask from the closed form the kernel uses: id = 3 r(16 wy + i, H) + r(16 wx + j, W), r(Y, L) = 0 if Y < L - 16, 1 if
    Y < L - 8, else 2.  swapped: the two lengths exchanged (a seeded mistake)"""
    def r(Y, L):
        return (Y >= L - WS).long() + (Y >= L - SHIFT).long()
    LH, LW = (W, H) if swapped else (H, W)
    ids = 3 * r(torch.arange(H), LH)[:, None] + r(torch.arange(W), LW)[None, :]
    mw = window_partition(ids.view(1, H, W, 1).float()).view(-1, 256)
    return torch.where(mw.unsqueeze(1) != mw.unsqueeze(2), -100.0, 0.0)


def pixel_shuffle_nhwc(x):
    """[B, H, W, 4 C] -> [B, 2 H, 2 W, C]: out[b, 2 y + i, 2 x + j, c] = x[b, y, x, 4 c + 2 i + j] (nn.PixelShuffle(2) on NHWC)"""
    B, H, W, C4 = x.shape
    return x.view(B, H, W, C4 // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, C4 // 4)


# ---------------------------------------------------------------------------------------------------------------- the network
def net(sd, cfg, x, store=None, compute=torch.float32):
    """compute: the dtype every operation runs in (fp32 for the tests; tools/hat_time.py times the same code in fp16 on the GPU)"""
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: fl(t.to(store)))
    wt = lambda name: q(fl(sd[name + ".weight"]))
    bs = lambda name: fl(sd[name + ".bias"])
    C, heads, scale_up = cfg["embed_dim"], cfg["num_heads"], cfg["upscale"]
    conv_scale = cfg["conv_scale"]
    idx_sa, idx_oca = rpi_sa().to(x.device), rpi_oca().to(x.device)

    def c3(t, name):
        return F.conv2d(t, wt(name), bs(name), stride=1, padding=1)

    def lin(t, name):
        return F.linear(t, wt(name), bs(name))

    def norm(t, name):
        return F.layer_norm(t, (C,), fl(sd[name + ".weight"]), fl(sd[name + ".bias"]), 1e-5)

    def mlp(t, p):
        h = q(lin(q(norm(t, p + ".norm2")), p + ".mlp.fc1"))
        return q(t + lin(q(F.gelu(h)), p + ".mlp.fc2"))

    def cab(t, p):
        """CAB on an image [B, C, H, W] of LN1's output; returns conv_x [B, C, H, W] (before conv_scale)"""
        c = q(c3(q(F.gelu(q(c3(t, p + ".0")))), p + ".2"))
        y = F.adaptive_avg_pool2d(c, 1)
        y = F.relu(F.conv2d(y, fl(sd[p + ".3.attention.1.weight"]), bs(p + ".3.attention.1")))
        y = F.conv2d(y, fl(sd[p + ".3.attention.3.weight"]), bs(p + ".3.attention.3"))
        return c * torch.sigmoid(y)

    def win_attention(xw, p, nh, mask):
        b_, n, c = xw.shape
        qkv = q(lin(xw, p + ".qkv")).reshape(b_, n, 3, nh, c // nh).permute(2, 0, 3, 1, 4)
        qq, kk, vv = qkv[0], qkv[1], qkv[2]
        qq = qq * (c // nh) ** -0.5
        attn = qq @ kk.transpose(-2, -1)
        bias = fl(sd[p + ".relative_position_bias_table"])[idx_sa.view(-1)].view(WS * WS, WS * WS, -1).permute(2, 0, 1).contiguous()
        attn = attn + bias.unsqueeze(0)
        if mask is not None:
            nw = mask.shape[0]
            attn = attn.view(b_ // nw, nw, nh, n, n) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, nh, n, n)
        attn = q(torch.softmax(attn, dim=-1))
        return lin(q((attn @ vv).transpose(1, 2).reshape(b_, n, c)), p + ".proj")

    def hab(t, p, nh, shift, h, w, mask):
        b, _, c = t.shape
        shortcut = t
        t = q(norm(t, p + ".norm1")).view(b, h, w, c)
        conv_x = cab(t.permute(0, 3, 1, 2), p + ".conv_block.cab")
        conv_x = conv_x.permute(0, 2, 3, 1).contiguous().view(b, h * w, c)
        shifted = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else t
        xw = window_partition(shifted, WS).view(-1, WS * WS, c)
        aw = win_attention(xw, p + ".attn", nh, mask if shift > 0 else None)
        shifted = window_reverse(aw.view(-1, WS, WS, c), WS, h, w)
        attn_x = torch.roll(shifted, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else shifted
        attn_x = attn_x.view(b, h * w, c)
        if store is None:
            t = shortcut + attn_x + conv_x * conv_scale
        else:
            t = q(q(shortcut + attn_x) + conv_x * conv_scale)        # the projection's epilogue, then the scale-add pass
        return mlp(t, p)

    def ocab(t, p, nh, h, w):
        b, _, c = t.shape
        shortcut = t
        t = q(norm(t, p + ".norm1")).view(b, h, w, c)
        qkv = q(lin(t, p + ".qkv")).reshape(b, h, w, 3, c).permute(3, 0, 4, 1, 2)
        qq = qkv[0].permute(0, 2, 3, 1)
        kv = torch.cat((qkv[1], qkv[2]), dim=1)
        qw = window_partition(qq, WS).view(-1, WS * WS, c)
        kvw = F.unfold(kv, kernel_size=(OWS, OWS), stride=WS, padding=PAD)
        nw = kvw.shape[-1]
        # rearrange 'b (nc ch owh oww) nw -> nc (b nw) (owh oww) ch'
        kvw = kvw.view(b, 2, c, OWS * OWS, nw).permute(1, 0, 4, 3, 2).reshape(2, b * nw, OWS * OWS, c).contiguous()
        kw, vw = kvw[0], kvw[1]
        b_, nq, _ = qw.shape
        n, d = kw.shape[1], c // nh
        qq = qw.reshape(b_, nq, nh, d).permute(0, 2, 1, 3)
        kk = kw.reshape(b_, n, nh, d).permute(0, 2, 1, 3)
        vv = vw.reshape(b_, n, nh, d).permute(0, 2, 1, 3)
        qq = qq * d ** -0.5
        attn = qq @ kk.transpose(-2, -1)
        bias = fl(sd[p + ".relative_position_bias_table"])[idx_oca.view(-1)].view(WS * WS, OWS * OWS, -1).permute(2, 0, 1).contiguous()
        attn = attn + bias.unsqueeze(0)
        attn = q(torch.softmax(attn, dim=-1))
        aw = q((attn @ vv).transpose(1, 2).reshape(b_, nq, c))
        t = window_reverse(aw.view(-1, WS, WS, c), WS, h, w).view(b, h * w, c)
        t = q(lin(t, p + ".proj") + shortcut)
        return mlp(t, p)

    H, W = x.shape[2:]
    assert H % WS == 0 and W % WS == 0, "the reference has no padding: H and W are multiples of 16"
    mean = torch.Tensor(MEAN).view(1, 3, 1, 1).to(x).to(compute)
    t = q((fl(x) - mean) * cfg["img_range"])
    first = q(c3(t, "conv_first"))
    mask = fl(calculate_mask(H, W)).to(x.device)
    t = q(norm(first.flatten(2).transpose(1, 2), "patch_embed.norm"))
    for i, depth in enumerate(cfg["depths"]):
        keep = t
        rg = f"layers.{i}.residual_group"
        for j in range(depth):
            t = hab(t, f"{rg}.blocks.{j}", heads[i], SHIFT if j % 2 else 0, H, W, mask)
        t = ocab(t, f"{rg}.overlap_attn", heads[i], H, W)
        img = t.transpose(1, 2).contiguous().view(t.shape[0], C, H, W)
        t = q(c3(img, f"layers.{i}.conv").flatten(2).transpose(1, 2) + keep)
    t = q(norm(t, "norm")).transpose(1, 2).contiguous().view(t.shape[0], C, H, W)
    t = q(c3(t, "conv_after_body") + first)
    t = q(F.leaky_relu(q(c3(t, "conv_before_upsample.0")), 0.01))
    t = F.pixel_shuffle(q(c3(t, "upsample.0")), 2)
    if scale_up == 4:
        t = F.pixel_shuffle(q(c3(t, "upsample.2")), 2)
    t = q(c3(t, "conv_last"))
    return q(t / cfg["img_range"] + mean)


# ------------------------------------------------------------------------------------------------------------ one kernel call
def case(sdt, mode, B, H, W, heads, shift=0, seed=0, pad_cols=8):
    """qkv with q, k, v ~ N(0, 1) rounded to sdt (columns 30, 31 of every group zero, `pad_cols` NaN columns behind the last group), a
    bias table of std 1 (the initialiser's 0.02 would let every bias mistake pass), o NaN-filled with stride 30 heads + pad_cols;
    kvbias: what the seeded mistake "pad_keys_biased" puts into the keys and values outside the image"""
    g = torch.Generator().manual_seed(1000 * seed + 31 * H + 7 * W + 3 * heads + shift + (500 if mode == "oca" else 0))
    rows = B * H * W
    qkv = torch.randn((rows, 3 * heads, 32), generator=g)
    qkv[:, :, 30:] = 0
    qkv = torch.cat([qkv.view(rows, 96 * heads), torch.full((rows, pad_cols), float("nan"))], 1).to(sdt)
    table = torch.randn((961 if mode == "sa" else 1521, heads), generator=g)
    kvbias = torch.randn((2 * heads * 30,), generator=g).to(sdt)
    o = torch.full((rows, 30 * heads + pad_cols), float("nan")).to(sdt)
    return dict(mode=mode, qkv=qkv, table=table, o=o, B=B, H=H, W=W, heads=heads, shift=shift, kvbias=kvbias)


def _sa_windows(L, dt, shift):
    """q, k, v [B nW, heads, 256, 30] of the SA call in dtype dt, rolled by -shift"""
    B, H, W, nh = L["B"], L["H"], L["W"], L["heads"]
    t = L["qkv"][:, :96 * nh].to(dt).view(B, H, W, 96 * nh)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    w = window_partition(t).view(-1, 256, 3, nh, 32)[..., :30].permute(2, 0, 3, 1, 4)
    return w[0], w[1], w[2]


def _oca_windows(L, dt, mistake=None):
    """q [B nW, heads, 256, 30], k, v [B nW, heads, 576, 30], valid [B nW, 1, 1, 576] (key inside the image) of the OCA call"""
    B, H, W, nh = L["B"], L["H"], L["W"], L["heads"]
    t = L["qkv"][:, :96 * nh].to(dt).view(B, H, W, 3, nh, 32)[..., :30]
    qq = window_partition(t[:, :, :, 0].reshape(B, H, W, nh * 30)).view(-1, 256, nh, 30).permute(0, 2, 1, 3)
    kv = t[:, :, :, 1:].reshape(B, H, W, 2 * nh * 30).permute(0, 3, 1, 2)
    if mistake == "pad_keys_biased":
        kv = kv - L["kvbias"].to(dt).view(1, -1, 1, 1)
    lo, hi = (0, 2 * PAD) if mistake == "origin_not_centred" else (PAD, PAD)
    kv = F.pad(kv, (lo, hi, lo, hi), mode="replicate" if mistake == "pad_keys_clamped" else "constant")
    un = F.unfold(kv, kernel_size=(OWS, OWS), stride=WS)                                      # [B, ch 576, nW]
    nw = un.shape[-1]
    un = un.view(B, 2, nh, 30, 576, nw).permute(1, 0, 5, 2, 4, 3).reshape(2, B * nw, nh, 576, 30)
    if mistake == "pad_keys_biased":
        un = un + L["kvbias"].to(dt).view(2, 1, nh, 1, 30)
    ones = F.pad(torch.ones((1, 1, H, W), dtype=dt), (lo, hi, lo, hi))
    valid = F.unfold(ones, kernel_size=(OWS, OWS), stride=WS).view(1, 576, nw).permute(0, 2, 1).repeat(B, 1, 1).reshape(B * nw, 1, 1, 576) > 0
    return qq, un[0], un[1], valid


def _unwindow(L, ow, shift):
    """[B nW, heads, 256, 30] -> [B H W, 30 heads] in token order, rolled back by shift"""
    B, H, W, nh = L["B"], L["H"], L["W"], L["heads"]
    t = window_reverse(ow.transpose(1, 2).reshape(-1, WS, WS, 30 * nh), WS, H, W)
    if shift:
        t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
    return t.reshape(B * H * W, 30 * nh)


def _operands(L, dt):
    """(q, k, v, bias [1, heads, 256, nk], mask or None) of the call as the reference computes them"""
    nh = L["heads"]
    if L["mode"] == "sa":
        qq, kk, vv = _sa_windows(L, dt, L["shift"])
        bias = L["table"].to(dt)[rpi_sa().view(-1)].view(256, 256, nh).permute(2, 0, 1).unsqueeze(0)
        mask = None
        if L["shift"]:
            nW = (L["H"] // WS) * (L["W"] // WS)
            mask = calculate_mask(L["H"], L["W"]).to(dt).repeat(L["B"], 1, 1).view(L["B"] * nW, 1, 256, 256)
        return qq, kk, vv, bias, mask
    qq, kk, vv, _ = _oca_windows(L, dt)
    bias = L["table"].to(dt)[rpi_oca().view(-1)].view(256, 576, nh).permute(2, 0, 1).unsqueeze(0)      # (negative indices wrap)
    return qq, kk, vv, bias, None


def value64(L):
    """(E, t): float64 value of the live columns [B H W, 30 heads] and the error t of the bound before the output rounding"""
    d = torch.float64
    sdt = L["o"].dtype
    u, fl = U[sdt], FL[sdt]
    qq, kk, vv, bias, m = _operands(L, d)
    nk = kk.shape[-2]
    T = nk // 32 + 2
    dot = qq @ kk.transpose(-2, -1)
    A = qq.abs() @ kk.abs().transpose(-2, -1)
    l = SCALE * dot + bias
    Lm = (SCALE * dot).abs() + bias.abs()
    if m is not None:
        l = l + m
        Lm = Lm + m.abs()
    dl = SCALE * 2 * 32 * E * A + 3 * E * Lm
    D = dl.amax(-1, keepdim=True)
    x = l - l.amax(-1, keepdim=True)
    p = torch.softmax(l, dim=-1)
    r = 2 * D + 2 * E * x.abs() + 4 * E
    R = (p * (2 * D + 2 * E * x.abs())).sum(-1, keepdim=True) + 5 * E * T + nk * E
    dp = p * (r + R + 4 * E) * (1 + u) + u * p + fl + 2.0 ** -126
    val = p @ vv
    t = dp @ vv.abs() + 2 * nk * E * (p @ vv.abs())
    s = L["shift"] if L["mode"] == "sa" else 0
    return _unwindow(L, val, s), _unwindow(L, t, s)


def bound(L):
    sdt = L["o"].dtype
    v, t = value64(L)
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def emulate(L, mistake=None):
    """the output buffer after the call, computed on the host in fp32 with the kernel's roundings (mistake: one of MISTAKES[mode])"""
    mode = L["mode"]
    assert mistake is None or mistake in MISTAKES[mode]
    sdt, f, nh = L["o"].dtype, torch.float32, L["heads"]
    c = torch.tensor(SCALE, dtype=f)
    if mode == "sa":
        s = L["shift"]
        if mistake == "one_window_not_shifted" and (L["H"] == WS or L["W"] == WS):
            s = 0
        qq, kk, vv = _sa_windows(L, f, -s if mistake == "shift_sign_flipped" else s)
        bias = L["table"].float()[sa_index_closed().view(-1)].view(256, 256, nh).permute(2, 0, 1).unsqueeze(0)
        if mistake == "bias_transposed":
            bias = bias.transpose(-2, -1)
        dot = qq @ kk.transpose(-2, -1)
        l = (dot + bias) * c if mistake == "scale_after_bias" else c * dot + bias
        if s and mistake != "mask_omitted":
            nW = (L["H"] // WS) * (L["W"] // WS)
            l = l + region_mask(L["H"], L["W"], swapped=mistake == "mask_hw_swapped").repeat(L["B"], 1, 1).view(L["B"] * nW, 1, 256, 256)
        back = 0 if mistake == "reverse_shift_dropped" else s
    else:
        qq, kk, vv, valid = _oca_windows(L, f, mistake)
        idx = oca_index_closed(wrapped=mistake != "index_not_wrapped", transposed=mistake == "bias_transposed")
        bias = L["table"].float()[idx.view(-1)].view(256, 576, nh).permute(2, 0, 1).unsqueeze(0)
        l = c * (qq @ kk.transpose(-2, -1)) + bias
        if mistake == "pad_keys_excluded":
            l = l.masked_fill(~valid, float("-inf"))
        back = 0
    p = torch.softmax(l, dim=-1).to(sdt).float()
    ow = (p @ vv).to(sdt).float()
    buf = L["o"].clone()
    buf[:, :30 * nh] = _unwindow(L, ow, back).to(sdt)
    return buf


def verdict(L, got):
    """(worst |got - E| / bound over the live columns, True when every other element still has the bits it had)"""
    v, bd = bound(L)
    n = 30 * L["heads"]
    worst = float(((got[:, :n].double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    return worst, torch.equal(bits(got)[:, n:], bits(L["o"])[:, n:])


# ------------------------------------------------------------------------------------------------------------- the CAB passes
# (B, H, W, C, ld): the tiny and the real width, more than one 64-row chunk, a last chunk that is not full
CAB_CASES = [(2, 16, 32, 60, 64), (3, 16, 20, 180, 192), (1, 9, 7, 240, 256)]


def cab_case(sdt, B, H, W, C, ld, seed=0):
    """y and c2 [B, HW, ld] storage (the channels [C, ld) zero, as the graph keeps them), the gate's fp32 weights, conv_scale 0.01; a
    per-channel offset in c2 keeps the pooled means away from zero"""
    g = torch.Generator().manual_seed(100 * seed + H + 3 * W + C)
    HW, Cs = H * W, C // 30
    y, c2 = torch.randn((B, HW, ld), generator=g), torch.randn((B, HW, ld), generator=g) + torch.randn((1, 1, ld), generator=g)
    y[..., C:] = 0
    c2[..., C:] = 0
    return dict(y=y.to(sdt), c2=c2.to(sdt), B=B, H=H, W=W, C=C, Cs=Cs, ld=ld, scale=0.01,
                w1=torch.randn((Cs, C), generator=g) / C ** 0.5 * 4, b1=torch.randn((Cs,), generator=g) * 0.1,
                w2=torch.randn((C, Cs), generator=g), b2=torch.randn((C,), generator=g) * 0.1)


def pool_ref(x, C):
    """(mean over HW [B, C] in float64, its bound) of x [B, HW, ld] storage"""
    v = x[..., :C].double()
    nchunk = math.ceil(x.shape[1] / 64)
    return v.mean(1), (nchunk + 18) * E * v.abs().mean(1)


def gate_ref(pool, dpool, L):
    """(s [B, C] float64, bound) of k_chan_gate on pool values within dpool of `pool`"""
    w1, b1, w2, b2 = (L[k].double() for k in ("w1", "b1", "w2", "b2"))
    C, Cs, scale = L["C"], L["Cs"], f32(L["scale"])
    pre = pool @ w1.T + b1
    h = pre.clamp_min(0)
    dh = dpool @ w1.abs().T + (C + 1) * E * (b1.abs() + pool.abs() @ w1.abs().T)
    z = h @ w2.T + b2
    dz = dh @ w2.abs().T + (Cs + 1) * E * (b2.abs() + h @ w2.abs().T)
    sg = torch.sigmoid(z)
    s = scale * sg
    return s, s * (1 - sg) * dz + 6 * E * s


def cab_value64(L):
    """(E [B, HW, ld], bound) of y after pool -> gate -> scale-add"""
    sdt = L["y"].dtype
    pool, dpool = pool_ref(L["c2"], L["C"])
    s, ds = gate_ref(pool, dpool, L)
    pad = L["ld"] - L["C"]
    s, ds = F.pad(s, (0, pad)).unsqueeze(1), F.pad(ds, (0, pad)).unsqueeze(1)
    y, c2 = L["y"].double(), L["c2"].double()
    v = y + c2 * s
    t = c2.abs() * ds + E * v.abs()
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt] * (v != 0)


def cab_emulate(L, mistake=None):
    assert mistake is None or mistake in MISTAKES["cab"]
    f, sdt, C = torch.float32, L["y"].dtype, L["C"]
    c2 = L["c2"].float()
    pool = c2[:, :WS * WS, :C].mean(1) if mistake == "pool_per_window" else c2[..., :C].mean(1)
    z = F.relu(pool @ L["w1"].T + L["b1"]) @ L["w2"].T + L["b2"]
    s = (z if mistake == "sigmoid_dropped" else torch.sigmoid(z)) * (1.0 if mistake == "conv_scale_dropped" else torch.tensor(L["scale"], dtype=f))
    s = F.pad(s, (0, L["ld"] - C)).unsqueeze(1)
    return (L["y"].float() + c2 * s).to(sdt)


def cab_verdict(L, got):
    v, bd = cab_value64(L)
    return float(((got.double() - v).abs() / bd.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------- model test cases
# name -> (keywords of gyre_amd.config.tiny_hat, image shape): the tiny configuration on 1 x 2 windows, one RHAG at x2 on 2 x 3 windows,
# and one HAB pair at the real width (180 -> 192 padded channels, 60 -> 64 in the CAB)
MODEL_CASES = {"tiny": (dict(), (2, 3, 16, 32)),
               "tiny2": (dict(depths=[2], num_heads=[2], upscale=2), (1, 3, 32, 48)),
               "w180": (dict(embed_dim=180, num_heads=[6], depths=[2]), (1, 3, 32, 32))}


def model_case(name):
    """(cfg, state dict, image) of a MODEL_CASES entry: synthetic N(0, 1 / fan_in) weights, the position tables at std 1"""
    from gyre_amd import config as gcfg, weights
    kw, shape = MODEL_CASES[name]
    cfg = gcfg.tiny_hat(**kw)
    shapes = {k: v for k, v in weights.hat_param_shapes(cfg).items() if not weights.hat_is_buffer(k)}
    sd = weights.synthetic_state_dict(shapes)
    for k in sd:
        if k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(len(k)))
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0))
    return cfg, sd, x
