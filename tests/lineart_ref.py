"""References for the line-art hinter (gyre_amd/hinters.py, model_lineart.hip, kernels_inorm.hip).

net(sd, cfg, x) restates the reference's DrawingGenerator (gyre/pipeline/hinters/models/informative_drawings.py) in torch functional
calls, fp32; tests/test_reference_lineart.py holds it bit for bit to the reference's own module where that tree is present.
store = a 16-bit dtype rounds every tensor the native graph stores (the entry image, every weight, every convolution output, every
apply-pass output, the result) - the storage emulation whose distance from the fp32 net the GPU model gate is twice of.  mistake =
one of MISTAKES seeds a wrong reading of the graph; the transposed-convolution mistakes run the layer in the sub-pixel form the native
graph uses (tconv_subpixel), which without a mistake equals F.conv_transpose2d.

Element bounds of the kernel hooks, float64 absolute-value forms, u = unit roundoff of the storage type, e = 2^-24, fl = its smallest
subnormal step (the way tests/norm_fwd_ref.py derives GroupNorm's):

Instance normalisation.  The kernel sums d = x - s (s = the plane's first value; the difference of two storage values, one fp32
rounding) and d^2 in fp32: per thread a chain of at most 64 rows, then at most 32 row lanes, then the ceil(HW / 512) chunks in eight
interleaved slices and the slices in order (never more non-zero additions than there are chunks) - a chain of at most
L = 96 + ceil(HW / 512) additions.  With A1 = mean|d|, A2 = mean d^2 and md = mean d:
    dm   <= (L + 2) e A1                                  (S1 / n; + e |s + md| for the last addition)
    dvar <= (L + 4) e A2 + 2 |md| dm + 3 e md^2           (S2 / n - md^2)
    rstd = 1 / sqrt(var + eps): relative error <= dvar / (2 (var + eps)) + 3 e      (first order; sqrtf and the division are correctly rounded)
    y = (x - m) rstd:  t = rstd dm + |y| (dvar / (2 (var + eps)) + 5 e)             (the subtraction, the product)
    + residual r: t += e |y + r|;   stored: bound = t + u (|E| + t) + fl   with E the exact value.  ReLU is 1-Lipschitz and exact.
A constant plane gives d = 0 everywhere: S1 = S2 = 0, m = s, y = 0 exactly.

7x7 convolutions.  Products of two storage values are exact in fp32 (8 + 8 or 11 + 11 significant bits); the MFMA chain adds K of them
(K = 49 * 8 slots of which 147 are live, or 49 * 64) and the bias:  t = (K + 2) e (sum |x| |w| + |b|).  The sigmoid has slope <= 1 / 4 and
libm's expf, the addition and the division cost 4 e more:  t' = t / 4 + 4 e.  Then the rounding of the output dtype as above.

Transposed convolution as built (patch rows -> GEMM on the composed weights -> shuffled read): the patch rows and the shuffled read move
bits; the GEMM adds K = 4 Cin products (7 / 16 of them exact zeros) in fp32 in an order the planner picks:  t = (K + 2) e (sum |x| |w| + |b|),
one rounding to storage.  The weight composition moves values that are storage values already: exact.
"""
import math

import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
E = 2.0 ** -24
EPS = 1e-5
MISTAKES = ("zero_padding", "unbiased_variance", "relu_missing", "residual_dropped", "tconv_parities_swapped", "tconv_kernel_not_flipped",
            "tconv_edge_wrapped", "eps_1e-3", "final_bias_dropped")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def out_size(h):
    """the output side of an input side h: 4 ceil(ceil(h / 2) / 2)"""
    return 4 * ((((h + 1) // 2) + 1) // 2)


# ------------------------------------------------------------------------------------------------------- sub-pixel transposed convolution
def compose_tconv(w, flipped=True):
    """[Cin, Cout, 3, 3] -> [4 Cout, 4 Cin]: rows (a, b, co), columns (dy, dx, ci); a = 0: ky 1 at dy 0; a = 1: ky 2 at dy 0, ky 0 at dy 1
    (flipped = False seeds the mistake of reading the kernel in correlation order: ky 0 at dy 0, ky 2 at dy 1)"""
    cin, cout = w.shape[:2]
    out = torch.zeros(2, 2, cout, 2, 2, cin, dtype=w.dtype)
    tap = {(0, 0): 1, (1, 0): 2, (1, 1): 0} if flipped else {(0, 0): 1, (1, 0): 0, (1, 1): 2}
    for (a, dy), ky in tap.items():
        for (b, dx), kx in tap.items():
            out[a, b, :, dy, dx, :] = w[:, :, ky, kx].t()
    return out.reshape(4 * cout, 4 * cin)


def patch_rows(x, wrapped=False):
    """NHWC [B, H, W, C] -> [B, H, W, 4 C]: pixels (y + dy, x + dx) in (dy, dx, c) order, zeros past the edge (wrapped = the mistake)"""
    B, H, W, C = x.shape
    if wrapped:
        xp = torch.cat([x, x[:, :1]], 1)
        xp = torch.cat([xp, xp[:, :, :1]], 2)
    else:
        xp = F.pad(x, (0, 0, 0, 1, 0, 1))
    return torch.cat([xp[:, dy:dy + H, dx:dx + W] for dy in (0, 1) for dx in (0, 1)], -1)


def unshuffle_rows(y, cout, swapped=False):
    """[B, H, W, (a, b, Cout)] -> the image NHWC [B, 2 H, 2 W, Cout] (swapped = the mistake of reading it as (b, a, Cout))"""
    B, H, W, _ = y.shape
    y = y.reshape(B, H, W, 2, 2, cout)
    if swapped:
        y = y.transpose(3, 4)
    return y.permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, cout)


def shuffle_rows(img):
    """the inverse of unshuffle_rows: NHWC [B, 2 H, 2 W, C] -> [B, H, W, (a, b, C)]"""
    B, H2, W2, C = img.shape
    return img.reshape(B, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 // 2, W2 // 2, 4 * C)


def tconv_subpixel(x, w, b, mistake=None):
    """conv_transpose2d(x, w, b, stride 2, padding 1, output_padding 1) of NCHW x the way the native graph runs it"""
    wc = compose_tconv(w, flipped=mistake != "tconv_kernel_not_flipped")
    rows = patch_rows(x.permute(0, 2, 3, 1), wrapped=mistake == "tconv_edge_wrapped")
    y = F.linear(rows, wc, b.repeat(4))
    return unshuffle_rows(y, w.shape[1], swapped=mistake == "tconv_parities_swapped").permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------------- the net
def net(sd, cfg, x, store=None, mistake=None, compute=torch.float32):
    """compute: the dtype every operation runs in (fp32 for the tests; tools/lineart_time.py times the same code in fp16 on the GPU)"""
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: fl(t.to(store)))
    wt = lambda name: q(fl(sd[name + ".weight"]))
    bs = lambda name: fl(sd[name + ".bias"])
    eps = 1e-3 if mistake == "eps_1e-3" else EPS

    def pad(t, p):
        return F.pad(t, (p,) * 4, "constant" if mistake == "zero_padding" else "reflect")

    def inorm(t):
        if mistake == "unbiased_variance":
            m, v = t.mean((2, 3), keepdim=True), t.var((2, 3), keepdim=True, unbiased=True)
            return (t - m) / torch.sqrt(v + eps)
        return F.instance_norm(t, eps=eps)

    def tconv(t, name):
        if mistake is not None and mistake.startswith("tconv"):
            return tconv_subpixel(t, wt(name), bs(name), mistake)
        return F.conv_transpose2d(t, wt(name), bs(name), stride=2, padding=1, output_padding=1)

    t = q(fl(x))
    t = q(F.relu(inorm(q(F.conv2d(pad(t, 3), wt("model0.1"), bs("model0.1"))))))
    for name in ("model1.0", "model1.3"):
        t = q(F.relu(inorm(q(F.conv2d(t, wt(name), bs(name), stride=2, padding=1)))))
    for i in range(cfg["n_residual_blocks"]):
        p = f"model2.{i}.conv_block."
        h = inorm(q(F.conv2d(pad(t, 1), wt(p + "1"), bs(p + "1"))))
        h = q(h if mistake == "relu_missing" else F.relu(h))
        h = inorm(q(F.conv2d(pad(h, 1), wt(p + "5"), bs(p + "5"))))
        t = q(h if mistake == "residual_dropped" else t + h)
    for name in ("model3.0", "model3.3"):
        t = q(F.relu(inorm(q(tconv(t, name)))))
    t = F.conv2d(pad(t, 3), wt("model4.1"), None if mistake == "final_bias_dropped" else bs("model4.1"))
    return q(torch.sigmoid(t) if cfg["sigmoid"] else t)


# name -> (n_residual_blocks, sigmoid, image shape): every kind of layer once on a size that is no multiple of the 7x7 tile; the shipped
# depth on a batch; a size whose levels are odd (13 x 18 -> 7 x 9 -> 4 x 5, output 16 x 20); the constructor's default depth; and
# "quiet": first-layer weights at a tenth of their scale, so that the first normalisation sees planes whose variance (about 1e-3, a
# different one per channel) is of the order at which a wrong eps rescales every channel differently - the next convolution mixes the
# channels, so no later normalisation removes it
MODEL_CASES = {"tiny": (1, False, (1, 3, 8, 12)),
               "shipped": (3, True, (2, 3, 32, 40)),
               "odd": (3, False, (1, 3, 13, 18)),
               "deep": (9, True, (1, 3, 16, 16)),
               "quiet": (3, True, (1, 3, 16, 24))}
QUIET_FIRST_LAYER = 0.1


def model_case(name):
    """(cfg, state dict, image) of a MODEL_CASES entry: synthetic N(0, 1 / fan_in) weights; the one bias of the closing convolution is
    set to 0.5 - at the synthetic 0.05 scale dropping it would move a sigmoid output by less than the storage rounding does"""
    from gyre_amd import config as gcfg, weights
    blocks, sigmoid, shape = MODEL_CASES[name]
    cfg = gcfg.lineart_config(3, 1, blocks, sigmoid)
    sd = weights.synthetic_state_dict(weights.lineart_param_shapes(cfg))
    sd["model4.1.bias"] = torch.full((1,), 0.5)
    if name == "quiet":
        sd["model0.1.weight"] = sd["model0.1.weight"] * QUIET_FIRST_LAYER
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0))
    return cfg, sd, x


# ------------------------------------------------------------------------------------------------------- instance-normalisation kernels
# (B, H, W, C) of the GPU list: the smallest plane the graph reaches, one that is no multiple of any chunk, several 512-row chunks
INORM_SHAPES = [(1, 2, 2, 256), (3, 2, 2, 64), (1, 13, 18, 128), (3, 13, 18, 64), (1, 96, 80, 64), (3, 96, 80, 256), (1, 96, 80, 128)]
INORM_FAMILIES = ("plain", "offset", "constant", "quiet")


def inorm_input(sdt, B, H, W, C, family="plain", seed=0):
    """NHWC storage tensor: N(0.3, 1); "offset": the mean at 100 times the spread; "constant": sample 0 / channel 0 (and every
    channel of the last sample) one value per plane; "quiet": N(0.009, 0.03^2)"""
    g = torch.Generator().manual_seed(seed + 7919 * (H * W + C))
    x = torch.randn((B, H, W, C), generator=g) + 0.3
    if family == "offset":
        x = x * 0.5 + 50.0 * (1 + torch.arange(C) % 3)
    if family == "quiet":                                  # a variance of eps' own order: where a wrong eps shows
        x = x * 0.03
    x = x.to(sdt)
    if family == "constant":
        x[0, :, :, 0] = x[0, 0, 0, 0]
        x[-1] = x[-1, :1, :1]
    return x


def inorm_stats_ref(x, eps=EPS):
    """float64 statistics of NHWC x and the bounds of the module docstring, each [B, 1, 1, C]: (mean, rstd, var, dm, dvar, drstd) with
    dm / drstd the absolute bounds of the fp32 mean and rstd the statistics kernel leaves"""
    xd = x.double()
    n = x.shape[1] * x.shape[2]
    s = xd[:, :1, :1]
    d = xd - s
    md, a1, a2 = d.mean((1, 2), keepdim=True), d.abs().mean((1, 2), keepdim=True), (d * d).mean((1, 2), keepdim=True)
    var = (a2 - md * md).clamp_min(0)
    m, rstd = s + md, 1 / torch.sqrt(var + eps)
    L = 96 + math.ceil(n / 512)
    dm = (L + 2) * E * a1 + E * m.abs()
    dvar = (L + 4) * E * a2 + 2 * md.abs() * dm + 3 * E * md * md
    return m, rstd, var, dm, dvar, rstd * (dvar / (2 * (var + eps)) + 3 * E)


def inorm_ref(x, eps=EPS):
    """(mean, rstd, y, t) in float64 over NHWC x: t = the fp32 arithmetic's share of the bound (module docstring), before the rounding"""
    m, rstd, var, dm, dvar, _ = inorm_stats_ref(x, eps)
    y = (x.double() - m) * rstd
    t = rstd * dm + y.abs() * (dvar / (2 * (var + eps)) + 5 * E)
    return m, rstd, y, t


def stored_bound(ref, t, dt):
    return t + U[dt] * (ref.abs() + t) + FL[dt]


def inorm_emulate(x, eps=EPS):
    """the kernels' arithmetic in fp32 on the host (shifted sums in chunks of 512 rows, in order): (mean, rstd, y) fp32"""
    B, H, W, C = x.shape
    xf = x.float().reshape(B, H * W, C)
    s = xf[:, :1]
    d = xf - s
    s1 = torch.zeros(B, 1, C)
    s2 = torch.zeros(B, 1, C)
    for r0 in range(0, H * W, 512):
        s1 = s1 + d[:, r0:r0 + 512].sum(1, keepdim=True)
        s2 = s2 + (d[:, r0:r0 + 512] ** 2).sum(1, keepdim=True)
    n = torch.tensor(float(H * W))
    md = s1 / n
    var = (s2 / n - md * md).clamp_min(0)
    m, rstd = s + md, 1 / torch.sqrt(var + eps)
    return m, rstd, ((xf - m) * rstd).reshape(B, H, W, C)


def reflect_nhwc(t, p):
    return F.pad(t.permute(0, 3, 1, 2), (p,) * 4, "reflect").permute(0, 2, 3, 1) if p else t


def verdict(got, ref, bound):
    """worst |got - ref| / bound (nan / inf in got: inf)"""
    g = got.double()
    if not torch.isfinite(g).all():
        return float("inf")
    return float(((g - ref).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------------------- 7x7 convolutions
# (B, H, W): a side of 4 (the reflection reaches the far edge) both ways, and a size that crosses the 8 x 16 tile in both directions
CONV7_SHAPES = [(1, 4, 9), (2, 9, 4), (1, 37, 70)]


def conv7_in_case(sdt, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + H * 131 + W)
    x = torch.rand((B, 3, H, W), generator=g).to(sdt)
    w = (torch.randn((64, 3, 7, 7), generator=g) / 147 ** 0.5).to(sdt)
    b = torch.randn((64,), generator=g) * 0.05
    return x, w, b


def conv7_in_ref(x, w, b, mistake=None):
    """(value, t) NHWC float64"""
    mode = "constant" if mistake == "zero_padding" else "reflect"
    ref = F.conv2d(F.pad(x.double(), (3,) * 4, mode), w.double(), b.double())
    mag = F.conv2d(F.pad(x.double().abs(), (3,) * 4, mode), w.double().abs(), b.double().abs())
    return ref.permute(0, 2, 3, 1), ((49 * 8 + 2) * E * mag).permute(0, 2, 3, 1)


def conv7_out_case(sdt, B, H, W, seed=0):
    """xp: the pad-3 image NHWC [B, H + 6, W + 6, 64] (any values: the kernel does not know it is mirrored)"""
    g = torch.Generator().manual_seed(seed + H * 131 + W)
    xp = torch.randn((B, H + 6, W + 6, 64), generator=g).to(sdt)
    w = (torch.randn((1, 64, 7, 7), generator=g) / 56.0).to(sdt)
    b = torch.full((1,), 0.25)
    return xp, w, b


def conv7_out_ref(xp, w, b, sigmoid, mistake=None):
    """(value, t) NCHW [B, 1, H, W] float64"""
    x = xp.double().permute(0, 3, 1, 2)
    bias = None if mistake == "final_bias_dropped" else b.double()
    ref = F.conv2d(x, w.double(), bias)
    t = (49 * 64 + 2) * E * F.conv2d(x.abs(), w.double().abs(), b.double().abs())
    if sigmoid:
        ref, t = torch.sigmoid(ref), t / 4 + 4 * E
    return ref, t


# --------------------------------------------------------------------------------------------------------- transposed convolution as built
TCONV_SHAPES = [(1, 1, 1), (2, 2, 3), (1, 17, 9)]              # (B, H, W) of the input
TCONV_WIDTHS = [(256, 128), (128, 64)]


def tconv_case(sdt, B, H, W, cin, cout, seed=0):
    g = torch.Generator().manual_seed(seed + H * 131 + W + cin)
    x = torch.randn((B, H, W, cin), generator=g).to(sdt)
    w = (torch.randn((cin, cout, 3, 3), generator=g) / (2.25 * cin) ** 0.5).to(sdt)
    b = torch.randn((cout,), generator=g) * 0.05
    return x, w, b


def tconv_ref(x, w, b):
    """(value, t) NHWC [B, 2 H, 2 W, Cout] float64 from NHWC x"""
    xd = x.double().permute(0, 3, 1, 2)
    kw = dict(stride=2, padding=1, output_padding=1)
    ref = F.conv_transpose2d(xd, w.double(), b.double(), **kw)
    mag = F.conv_transpose2d(xd.abs(), w.double().abs(), b.double().abs(), **kw)
    return ref.permute(0, 2, 3, 1), ((4 * w.shape[0] + 2) * E * mag).permute(0, 2, 3, 1)
