"""References for the HED edge detector (gyre_amd/hinters.py, model_hed.hip, kernels_hed.hip).

net(sd, x) restates the reference's HED.forward (gyre/pipeline/hinters/models/hed.py) in torch functional calls, in fp32 (held bit for
bit to the reference's own module by tests/test_reference_hed.py) or, compute=torch.float64, as the yardstick of the GPU gates.
store = a 16-bit dtype rounds what the native graph stores in that type - the entry image, every convolution weight, every convolution
output - and leaves the scores and everything behind them in fp32, the result rounded once: the storage emulation whose distance from the
fp64 net the GPU model gate is twice of.  mistake = one of MISTAKES seeds a wrong reading of the graph.

Geometry.  conv1_1 has padding 35: stage 1 works at n + 68; MaxPool2d(2, 2, ceil_mode=True) halves upwards; side map k (1-based) is
upsampled by a bilinear transposed convolution of kernel 2 s, stride s = 2^(k-1), to (n_k + 1) s and centre-cropped to n with the offset
int(round(d / 2.)) - Python's round, halves to even.

Element bounds of the kernel hooks, float64 absolute-value forms, E = 2^-24, gamma(n) = n E / (1 - n E), u = the unit roundoff and fl
the smallest subnormal step of the output type:

Tail score.  so = bias + sum_c w_c relu(x_c): C + 1 terms.  The kernel forms each product inside an fma (no rounding of its own) and adds
the terms in an order that is a function of C; in ANY order a sum of n terms carries at most n - 1 rounded additions per term, so
    |so - exact| <= gamma(C + 1) (sum_c |w_c relu(x_c)| + |bias|) + E |exact|       (the last term: slack for the closing rounding)
The pooled output moves storage values (max and ReLU are exact): bit-equal to relu(max_pool2d(x, 2, 2, ceil_mode=True)).

Fuse.  The interpolation weights fy fx are multiples of 1 / (4 s^2) <= 1, exact in fp32, s <= 16.  l_1 is a copy (t_1 = 0); l_k, k >= 2,
adds at most four fma terms: t_k = gamma(4) sum |fy fx so|.  The fuse logit f = bf + sum_k wf_k l_k is six terms:
t_f = sum_k |wf_k| t_k + gamma(6) (|bf| + sum_k |wf_k l_k|).  The sigmoid has slope <= 1 / 4, and expf (1 ulp), the addition and the
division cost 4 E:  t' = t / 4 + 4 E.  Stored in the output type: bound = t' + u (|exact| + t') + fl.
"""
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
E = 2.0 ** -24
BORDER = 34
STAGES = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
MISTAKES = ("crop_floor", "crop_half_up", "pool_floor", "score_before_relu", "filter_centre_s", "border_33", "border_35",
            "fuse_weights_swapped", "side_sigmoid_missing", "pool_reads_past")
# (H, W): the smallest image; two sizes at which round-half-up and round-half-even crops differ; one at which floor-mode pooling changes
# maps 4 - 6 only; one odd / even size at which the two roundings agree; and 13x4, the case of the pooling window that reads past an odd
# side: stage 4 is odd both ways (11 x 9) and the crop of the 6 x 5 stage-5 map lies next to its last row and column, which is where such
# a read lands after the three convolutions of stage 5 (tests/test_hed_ref_host.py: what the other five cases see of it)
MODEL_CASES = {"1x1": (1, 1), "5x7": (5, 7), "16x16": (16, 16), "33x20": (33, 20), "64x47": (64, 47), "13x4": (13, 4)}
BATCH = 2
FUSE_WEIGHTS = (0.31, -0.27, 0.34, -0.29, 0.3)
FUSE_BIAS = 0.05


def gamma(n):
    return n * E / (1 - n * E)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def stored_bound(ref, t, dt):
    return t + U[dt] * (ref.abs() + t) + FL[dt]


def verdict(got, ref, bound):
    """worst |got - ref| / bound (nan / inf in got: inf)"""
    g = got.double()
    if not torch.isfinite(g).all():
        return float("inf")
    return float(((g - ref).abs() / bound).max())


# ---------------------------------------------------------------------------------------------------------------------------- geometry
def stage_sizes(n):
    """the side of the five stages for an image side n"""
    s = [n + 2 * BORDER]
    for _ in range(4):
        s.append(-(-s[-1] // 2))
    return s


def crop_offset(d, rule="half_even"):
    if rule == "floor":
        return d // 2
    if rule == "half_up":
        return (d + 1) // 2
    return int(round(d / 2.))


def crop_offsets(n, rule="half_even"):
    """the crop offset of the five maps for an image side n"""
    s = stage_sizes(n)
    return [crop_offset(s[0] - n, rule)] + [crop_offset((s[k] + 1) * 2 ** k - n, rule) for k in range(1, 5)]


def bilinear(s, dtype, centre_s=False):
    """the [1, 1, 2 s, 2 s] filter of the transposed convolution of stride s: f[t] = 1 - |t - (s - 0.5)| / s per axis"""
    t = torch.arange(2 * s, dtype=torch.float64)
    f = 1 - (t - (s if centre_s else s - 0.5)).abs() / s
    return (f[:, None] * f[None, :]).to(dtype)[None, None]


# ----------------------------------------------------------------------------------------------------------------------------- the net
def _pool_reading_past(t):
    """the 2x2 pooling of a kernel that reads the NHWC buffer past an odd side instead of shortening the window: the pixel right of a
    row's end is the next row's first, the row below a sample's end is the next sample's first (the first sample's for the last)"""
    B, C, H, W = t.shape
    if W % 2:
        nxt = torch.cat([t[:, :, 1:, :1], torch.roll(t, -1, 0)[:, :, :1, :1]], 2)
        t = torch.cat([t, nxt], 3)
    if H % 2:
        t = torch.cat([t, torch.roll(t, -1, 0)[:, :, :1]], 2)
    return F.max_pool2d(t, 2, 2)


def net(sd, x, store=None, mistake=None, compute=torch.float32):
    """the six maps [so1 .. so5, fuse], each [B, 1, H, W] and sigmoided.  compute: the dtype every operation runs in"""
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: fl(t.to(store)))
    wt = lambda name: q(fl(sd[name + ".weight"]))
    bs = lambda name: fl(sd[name + ".bias"])
    rule = {"crop_floor": "floor", "crop_half_up": "half_up"}.get(mistake, "half_even")
    H, W = x.shape[2:]

    def crop(t):
        h, w = t.shape[2:]
        y1, x1 = crop_offset(h - H, rule), crop_offset(w - W, rule)
        return t[:, :, y1:y1 + H, x1:x1 + W]

    t = q(fl(x))
    pad = {"border_33": BORDER, "border_35": BORDER + 2}.get(mistake, BORDER + 1)
    scores = []
    for k, (n, _) in enumerate(STAGES):
        for j in range(n):
            raw = q(F.conv2d(t, wt(f"conv{k + 1}_{j + 1}"), bs(f"conv{k + 1}_{j + 1}"), padding=pad if (k, j) == (0, 0) else 1))
            t = F.relu(raw)
        name = f"score_dsn{k + 1}"
        scores.append(F.conv2d(raw if mistake == "score_before_relu" else t, fl(sd[name + ".weight"]), bs(name)))
        if k < 4:
            if mistake == "pool_reads_past":
                t = _pool_reading_past(t)
            else:
                t = F.max_pool2d(t, 2, 2, ceil_mode=mistake != "pool_floor")
    sides = [crop(scores[0])]
    for k in range(1, 5):
        f = bilinear(2 ** k, compute, mistake == "filter_centre_s").to(scores[k].device)
        sides.append(crop(F.conv_transpose2d(scores[k], f, stride=2 ** k)))
    wf = fl(sd["score_final.weight"])
    if mistake == "fuse_weights_swapped":
        wf = wf[:, [1, 0, 2, 3, 4]]
    fuse = F.conv2d(torch.cat(sides, 1), wf, bs("score_final"))
    out = [torch.sigmoid(r) for r in sides + [fuse]]
    if mistake == "side_sigmoid_missing":
        out[2] = sides[2]
    return [q(r) for r in out]


def pipeline(module, tensor):
    """the reference's HedPipeline over any module: channel normalisation, the module's device and dtype, the ImageNet mean, BGR x 255,
    the fused map, the per-sample range normalisation, back on the input's device and in its dtype"""
    if tensor.ndim == 3:
        tensor = tensor[None]
    tensor = tensor[:, [0, 1, 2]] if tensor.shape[1] >= 3 else tensor[:, [0, 0, 0]]
    p = next(module.parameters())
    sample = tensor.to(p.device, p.dtype)
    mean = torch.tensor([0.485, 0.456, 0.406]).to(sample)[None, :, None, None]
    sample = (sample - mean)[:, [2, 1, 0]] * 255
    r = module(sample)[-1]
    dmin, dmax = torch.amin(r, dim=[1, 2, 3], keepdim=True), torch.amax(r, dim=[1, 2, 3], keepdim=True)
    return ((r - dmin) / (dmax - dmin)).to(tensor.device, tensor.dtype)


# ------------------------------------------------------------------------------------------------------------------------- model cases
_WEIGHTS = {}


def model_weights():
    """the seeded weights of every model test (generated once): convolutions N(0, 2 / fan_in) with biases of variance 0.5 - He's
    initialisation keeps the activations' scale through thirteen ReLU layers, and the biases keep the deep maps from collapsing to a
    constant; side scores N(0, 1 / (6400 C)) with biases of variance 0.3, which under the pipeline's x 255 input puts the side logits
    at a spread of up to 0.9 around means within +-2.5 instead of saturating the sigmoids (ReLU outputs have a positive mean that
    grows with the image - an rms of 96 at stage 5 of 64 x 47 - and a score vector's chance projection on it moves a whole deep map:
    at N(0, 1 / (1600 C)) map 5 of 64 x 47 sat at a logit of 3.8 +- 1 and failed the condition of test_hed_ref_host.py); score_final
    of mixed sign around 0.3, no two sides alike"""
    if not _WEIGHTS:
        from gyre_amd import weights
        g = torch.Generator().manual_seed(20)
        for key, shape in weights.hed_param_shapes().items():
            score = key.startswith("score_dsn")
            if key == "score_final.weight":
                t = torch.tensor(FUSE_WEIGHTS).reshape(shape)
            elif key == "score_final.bias":
                t = torch.full(shape, FUSE_BIAS)
            elif key.endswith(".bias"):
                t = torch.randn(shape, generator=g) * (0.3 if score else 0.5) ** 0.5
            else:
                fan_in = shape[1] * shape[2] * shape[3]
                t = torch.randn(shape, generator=g) * ((1.0 / (6400 * shape[1])) if score else (2.0 / fan_in)) ** 0.5
            _WEIGHTS[key] = t
    return _WEIGHTS


def model_input(name, batch=BATCH, seed=0):
    """what the pipeline feeds: (rand - 0.45) 255, mostly positive like a photo less its mean"""
    H, W = MODEL_CASES[name]
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    return (torch.rand((batch, 3, H, W), generator=g) - 0.45) * 255


def model_case(name):
    return model_weights(), model_input(name)


def informative_fraction(maps):
    """per map, the share of pixels inside (0.02, 0.98): where a sigmoid still tells logits apart"""
    return [float(((m > 0.02) & (m < 0.98)).double().mean()) for m in maps]


# ------------------------------------------------------------------------------------------------------------------------- tail kernel
TAIL_WIDTHS = (64, 128, 256, 512)
TAIL_SIZES = ((1, 1), (2, 3), (5, 5), (9, 18), (69, 69))       # one element; an odd column; odd both ways; even / odd; stage 1 of 1 x 1
TAIL_BATCHES = (1, 3)


def tail_case(sdt, B, Hs, Ws, C, seed=0):
    """x NHWC storage (about half of it negative, some windows wholly so), w fp32 [C], bias fp32 [1]"""
    g = torch.Generator().manual_seed(seed + 7919 * (Hs * Ws) + C + B)
    x = torch.randn((B, Hs, Ws, C), generator=g)
    x[:, ::2, 1::3] = -x[:, ::2, 1::3].abs() - 0.01                # pixels that are negative in every channel
    if Hs >= 4 and Ws >= 4:
        x[:, :2, :2] = -x[:, :2, :2].abs() - 0.01                  # a whole window that is
    w = torch.randn((C,), generator=g) / C ** 0.5
    b = torch.full((1,), 0.37)
    return x.to(sdt), w, b


def tail_ref(x, w, b, before_relu=False):
    """(pooled NHWC in x's dtype - exact; score [B, Hs, Ws] float64; its bound)"""
    xc = x.float().permute(0, 3, 1, 2)
    pooled = F.relu(F.max_pool2d(xc, 2, 2, ceil_mode=True)).permute(0, 2, 3, 1).to(x.dtype)
    r = x.double() if before_relu else x.double().clamp_min(0)
    so = (r * w.double()).sum(-1) + b.double()
    mag = (r * w.double()).abs().sum(-1) + b.double().abs()
    return pooled, so, gamma(x.shape[-1] + 1) * mag + E * so.abs()


# ------------------------------------------------------------------------------------------------------------------------- fuse kernel
def fuse_case(name, B=BATCH, seed=0):
    """random fp32 score maps [B, n_k, m_k] of a MODEL_CASES geometry (logits of spread 1.5), score_final's weights and bias"""
    H, W = MODEL_CASES[name]
    g = torch.Generator().manual_seed(seed + 31 * H + W)
    so = [torch.randn((B, h, w), generator=g) * 1.5 for h, w in zip(stage_sizes(H), stage_sizes(W))]
    return so, torch.tensor(FUSE_WEIGHTS), torch.full((1,), FUSE_BIAS)


def fuse_ref(so, wf, bf, H, W, rule="half_even", centre_s=False):
    """(six maps [6, B, 1, H, W] float64, t: the fp32 arithmetic's share of the bound, before the output rounding)"""
    oy, ox = crop_offsets(H, rule), crop_offsets(W, rule)
    ls, ts = [], []
    for k in range(5):
        s = so[k].double()[:, None]
        if k:
            f = bilinear(2 ** k, torch.float64, centre_s)
            up, mag = F.conv_transpose2d(s, f, stride=2 ** k), F.conv_transpose2d(s.abs(), f, stride=2 ** k)
        else:
            up, mag = s, s * 0
        ls.append(up[:, :, oy[k]:oy[k] + H, ox[k]:ox[k] + W])
        ts.append(gamma(4) * mag[:, :, oy[k]:oy[k] + H, ox[k]:ox[k] + W])
    wd, bd = wf.double(), bf.double()
    fuse = bd + sum(wd[k] * ls[k] for k in range(5))
    tf = sum(wd[k].abs() * ts[k] for k in range(5)) + gamma(6) * (bd.abs() + sum((wd[k] * ls[k]).abs() for k in range(5)))
    ref = torch.sigmoid(torch.stack(ls + [fuse]))
    return ref, torch.stack(ts + [tf]) / 4 + 4 * E
