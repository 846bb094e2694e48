"""References for the MLSD line detector (gyre_amd/hinters.py, model_mlsd.hip, kernels_mlsd.hip).

net(sd, x) restates the reference's MobileV2_MLSD_Large.forward (gyre/pipeline/hinters/models/mbv2_mlsd_large.py) in torch functional
calls: in fp32 (held to the reference's own module by tests/test_reference_mlsd.py and to its stored outputs by
tests/test_mlsd_ref_host.py) or, compute=torch.float64, as the yardstick of the GPU gates.  store = a 16-bit dtype is the storage
emulation of the native graph: every BatchNorm folded into its convolution in fp32 as gyre_mlsd_finalize does (s = gamma / sqrt(var +
1e-5), w' = w s rounded once to storage, b' = beta + (conv_bias - mean) s kept fp32), every tensor the graph stores rounded to storage
where the graph rounds it - the expand output before its ReLU6, the residual sum after the add, the upsampled map once - and everything
between in `compute`.  Its distance from the fp64 net is what the GPU model gate is twice of.  mistake = one of MISTAKES seeds a wrong
reading of the graph.

Element bounds of the kernel hooks, float64 absolute-value forms, E = 2^-24, gamma(n) = n E / (1 - n E), u = the unit roundoff (half an
ulp, relative) and fl the smallest subnormal step of the storage type.  A value v computed in fp32 with |v - exact| <= t and rounded once
to storage lies within  t + u (|exact| + t) + fl  of the exact value (stored_bound).

Depthwise, entry.  acc = sum of n products formed inside fmas, then + bias: n + 1 terms, in ANY order at most n rounded additions per
term:  t = gamma(n + 1) (sum |w x| + |bias|), n = 9 (depthwise) or 36 (entry).  ReLU6 is 1-Lipschitz and exact: the bound carries over.
Dilated convolution.  576 products and the bias on the MFMA, whose internal adder tree is undocumented: as tests/gemm_ref.py does, the
any-order bound is allowed twice:  t = 2 gamma(578) (sum |w x| + |bias|).
Upsample.  The source coordinate o (in - 1) / (out - 1) is split exactly into quotient and remainder; the fraction l = rem / (out - 1)
is one rounding (relative E), 1 - l another (absolute E / 2), each weight product a third: every one of the four weights is within 4 E
(absolute) of its exact value, and the four fma terms add gamma(4):  t = (4 E + gamma(4)) sum_q |v_q| over the four corners (a coarse
form: the weights are at most 1).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
E = 2.0 ** -24
SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1))
TAPS = (1, 3, 6, 10, 13)
MISTAKES = ("symmetric_padding", "align_corners_false", "relu_for_relu6", "dilation_1", "add_before_relu", "slice_first_9")
# name -> (B, H, W).  16x16: the deepest map is 1 x 1 and only the centre tap of the dilated convolution lies inside the 8 x 8 image;
# 17x49: odd sides, a batch of two; 64x32; 96x160
MODEL_CASES = {"16x16": (1, 16, 16), "17x49": (2, 17, 49), "64x32": (1, 64, 32), "96x160": (1, 96, 160)}


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


def size_ok(n):
    return n >= 16 and (n // 2) % 8 == 0


# ----------------------------------------------------------------------------------------------------------------------------- the net
def upsample2_ac(x):
    return F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=True)


def net(sd, x, store=None, mistake=None, compute=torch.float32, stats=None):
    """x[:, 7:] of the 16-channel map, [B, 9, H // 2, W // 2].  compute: the dtype every operation runs in.  stats: a dict that
    receives 'relu6_total' and 'relu6_at_6', the count of ReLU6 outputs and of those that sit at 6."""
    fl = lambda t: t.to(compute)
    q = (lambda t: t) if store is None else (lambda t: fl(t.to(store)))
    relu6 = (lambda t: F.relu(t)) if mistake == "relu_for_relu6" else (lambda t: F.relu6(t))

    def count(t):
        if stats is not None:
            stats["relu6_total"] = stats.get("relu6_total", 0) + t.numel()
            stats["relu6_at_6"] = stats.get("relu6_at_6", 0) + int((t >= 6).sum())
        return t

    def conv_bn(t, conv, bn, res=None, **kw):
        """BatchNorm(conv(t)) (+ res), rounded to storage once.  With a storage type the BatchNorm is folded as the native path does"""
        w, cb = sd[conv + ".weight"], sd.get(conv + ".bias")
        g, b, m, v = (sd[f"{bn}.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))
        if store is None:
            y = F.conv2d(t, fl(w), None if cb is None else fl(cb), **kw)
            y = F.batch_norm(y, fl(m), fl(v), fl(g), fl(b), False, 0.0, 1e-5)
        else:
            s = g.float() / torch.sqrt(v.float() + 1e-5)
            wf = q(fl(w.float() * s[:, None, None, None]))
            bf = b.float() + ((0 if cb is None else cb.float()) - m.float()) * s
            y = F.conv2d(t, wf, fl(bf), **kw)
        return q(y if res is None else y + res)

    def stride2(t, conv, bn, groups=1):
        """the reference's ConvBNReLU at stride 2: one zero pixel on the right and bottom only, padding 0"""
        if mistake == "symmetric_padding":
            h, w = t.shape[2] // 2, t.shape[3] // 2
            return conv_bn(t, conv, bn, stride=2, padding=1, groups=groups)[:, :, :h, :w]
        return conv_bn(F.pad(t, (0, 1, 0, 1)), conv, bn, stride=2, groups=groups)

    t = count(relu6(stride2(fl(x), "backbone.features.0.0", "backbone.features.0.1")))
    taps, cin, f = [], 32, 1
    for tt, c, n, s in SETTING:
        for i in range(n):
            p, stride, hid, j, inp = f"backbone.features.{f}.conv", (s if i == 0 else 1), tt * cin, 0, t
            if tt != 1:
                t = count(relu6(conv_bn(t, f"{p}.0.0", f"{p}.0.1")))
                j = 1
            if stride == 2:
                t = stride2(t, f"{p}.{j}.0", f"{p}.{j}.1", groups=hid)
            else:
                t = conv_bn(t, f"{p}.{j}.0", f"{p}.{j}.1", padding=1, groups=hid)
            t = count(relu6(t))
            t = conv_bn(t, f"{p}.{j + 1}", f"{p}.{j + 2}", res=inp if stride == 1 and cin == c else None)
            if f in TAPS:
                taps.append(t)
            cin, f = c, f + 1
    c1, c2, c3, c4, c5 = taps

    def block_a(name, a, b, upscale):
        b = F.relu(conv_bn(b, name + ".conv1.0", name + ".conv1.1"))
        a = F.relu(conv_bn(a, name + ".conv2.0", name + ".conv2.1"))
        if upscale:
            b = q(F.interpolate(b, scale_factor=2.0, mode="bilinear", align_corners=mistake != "align_corners_false"))
        return torch.cat((a, b), 1)

    def block_b(name, t):
        if mistake == "add_before_relu":
            t = q(F.relu(conv_bn(t, name + ".conv1.0", name + ".conv1.1", padding=1) + t))
        else:
            t = q(F.relu(conv_bn(t, name + ".conv1.0", name + ".conv1.1", padding=1)) + t)
        return F.relu(conv_bn(t, name + ".conv2.0", name + ".conv2.1", padding=1))

    t = block_b("block16", block_a("block15", c4, c5, False))
    t = block_b("block18", block_a("block17", c3, t, True))
    t = block_b("block20", block_a("block19", c2, t, True))
    t = block_b("block22", block_a("block21", c1, t, True))
    d = 1 if mistake == "dilation_1" else 5
    t = F.relu(conv_bn(t, "block23.conv1.0", "block23.conv1.1", padding=d, dilation=d))
    t = F.relu(conv_bn(t, "block23.conv2.0", "block23.conv2.1", padding=1))
    t = q(F.conv2d(t, q(fl(sd["block23.conv3.weight"])), fl(sd["block23.conv3.bias"])))
    return t[:, :9] if mistake == "slice_first_9" else t[:, 7:]


# ------------------------------------------------------------------------------------------------------------------------- model cases
_WEIGHTS = {}
# BatchNorm gains by the role of the layer: the ReLU6 layers are driven to a pre-activation spread of 3 - 5 so that a few per cent to a
# third of their outputs sit at 6 (test_mlsd_ref_host.py asserts 1 % .. 50 % over the net: a ReLU in place of ReLU6 must not pass);
# the linear projections bring the residual stream back to a spread near 1; the decoder keeps its scale
GAIN = {"first": 5.0, "expand": 4.0, "depthwise": 1.5, "project": 0.4, "decoder": 1.0}


def _role(bn):
    if bn == "backbone.features.0.1":
        return "first"
    if not bn.startswith("backbone"):
        return "decoder"
    parts = bn.split(".")                               # backbone.features.F.conv.J[.1]
    f, j, leaf_is_seq = int(parts[2]), int(parts[4]), len(parts) == 6
    if not leaf_is_seq:
        return "project"
    return "depthwise" if (f == 1 or j == 1) else "expand"


def model_weights():
    """the seeded weights of every model test (generated once): weights.synthetic_state_dict for the convolutions (N(0, 1 / fan_in),
    biases N(0, 0.05^2)); per BatchNorm gamma = GAIN[role] U[0.75, 1.25], beta N(0, 0.1^2), running_mean N(0, 0.1^2), running_var
    U[0.5, 1.5], num_batches_tracked 0"""
    if not _WEIGHTS:
        from gyre_amd import weights
        shapes = weights.mlsd_param_shapes()
        sd = weights.synthetic_state_dict(shapes, seed=23)
        g = torch.Generator().manual_seed(23)
        for key in shapes:
            if key.endswith(".running_var"):
                bn = key[:-len(".running_var")]
                n = shapes[key]
                sd[bn + ".weight"] = GAIN[_role(bn)] * (0.75 + 0.5 * torch.rand(n, generator=g))
                sd[bn + ".bias"] = 0.1 * torch.randn(n, generator=g)
                sd[bn + ".running_mean"] = 0.1 * torch.randn(n, generator=g)
                sd[key] = 0.5 + torch.rand(n, generator=g)
                sd[bn + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)
        _WEIGHTS.update(sd)
    return _WEIGHTS


def model_input(name, seed=0):
    """what the pipeline feeds: RGB in [-1, 1] and the constant plane 1 / 127.5 - 1"""
    B, H, W = MODEL_CASES[name]
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    rgb = 2 * torch.rand((B, 3, H, W), generator=g) - 1
    return torch.cat([rgb, torch.full((B, 1, H, W), 1 / 127.5 - 1)], 1)


def model_case(name):
    return model_weights(), model_input(name)


_REF64 = {}


def model_ref64(name):
    """the fp64 net on a case, computed once and shared"""
    if name not in _REF64:
        sd, x = model_case(name)
        _REF64[name] = net(sd, x, compute=torch.float64)
    return _REF64[name]


# ------------------------------------------------------------------------------------------------------------------------- kernel cases
def fold(w, cb, g, b, m, v, sdt):
    """the native BatchNorm fold: (w' in storage, b' fp32)"""
    s = g.float() / torch.sqrt(v.float() + 1e-5)
    return (w.float() * s.reshape(-1, *([1] * (w.ndim - 1)))).to(sdt), b.float() + ((0 if cb is None else cb.float()) - m.float()) * s


def dw_case(sdt, B, H, W, C, seed=0):
    """x NHWC storage with values on both sides of 0 and of 6, w [C, 1, 3, 3] storage, bias fp32"""
    g = torch.Generator().manual_seed(seed + 7919 * (H * W) + C + B)
    x = (torch.randn((B, H, W, C), generator=g) * 4 + 2).to(sdt)
    w = (torch.randn((C, 1, 3, 3), generator=g) / 3).to(sdt)
    return x, w, torch.randn((C,), generator=g)


def dw_ref(x, w, b, stride, relu6_in):
    """(relu6(depthwise(x) + b) NHWC float64, its fp32 share t of the bound)"""
    xc = x.double().permute(0, 3, 1, 2)
    if relu6_in:
        xc = F.relu6(xc)
    C = xc.shape[1]

    def conv(t, wt):
        if stride == 2:
            return F.conv2d(F.pad(t, (0, 1, 0, 1)), wt, stride=2, groups=C)
        return F.conv2d(t, wt, padding=1, groups=C)

    acc = conv(xc, w.double()) + b.double()[None, :, None, None]
    mag = conv(xc.abs(), w.double().abs()) + b.double().abs()[None, :, None, None]
    return F.relu6(acc).permute(0, 2, 3, 1), (gamma(10) * mag).permute(0, 2, 3, 1)


def entry_case(sdt, idt, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * H + W)
    x = (2 * torch.rand((B, 4, H, W), generator=g) - 1).to(idt)
    w = (torch.randn((32, 4, 3, 3), generator=g) * 1.5).to(sdt)
    return x, w, torch.randn((32,), generator=g)


def entry_ref(x, w, b):
    """(relu6(conv3x3 / 2 of the right-bottom padded x + b) NHWC float64, t)"""
    xp = F.pad(x.double(), (0, 1, 0, 1))
    acc = F.conv2d(xp, w.double(), b.double(), stride=2)
    mag = F.conv2d(xp.abs(), w.double().abs(), b.double().abs(), stride=2)
    return F.relu6(acc).permute(0, 2, 3, 1), (gamma(37) * mag).permute(0, 2, 3, 1)


def up2_case(sdt, B, H, W, C=64, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * H + W)
    return (torch.randn((B, H, W, C), generator=g) * 2).to(sdt)


def up2_ref(x, relu_in, align_corners=True):
    """(bilinear x2 NHWC float64, t)"""
    xc = x.double().permute(0, 3, 1, 2)
    if relu_in:
        xc = F.relu(xc)
    up = F.interpolate(xc, scale_factor=2.0, mode="bilinear", align_corners=align_corners)
    # the four corners of an output pixel lie inside the 2 x 2 source window at floor(coordinate): their absolute sum is at most the
    # window sum, which an all-ones 2 x 2 correlation of the edge-replicated map gives
    win = F.conv2d(F.pad(xc.abs(), (0, 1, 0, 1), mode="replicate"), torch.ones((xc.shape[1], 1, 2, 2), dtype=torch.float64), groups=xc.shape[1])
    H, W = xc.shape[2:]
    iy = (torch.arange(2 * H) * (H - 1)) // max(2 * H - 1, 1)
    ix = (torch.arange(2 * W) * (W - 1)) // max(2 * W - 1, 1)
    mag = win[:, :, iy][:, :, :, ix]
    return up.permute(0, 2, 3, 1), ((4 * E + gamma(4)) * mag).permute(0, 2, 3, 1)


def dconv_case(sdt, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * H + W)
    x = torch.randn((B, H, W, 64), generator=g).to(sdt)
    w = (torch.randn((64, 64, 3, 3), generator=g) / 24).to(sdt)
    return x, w, torch.randn((64,), generator=g) * 0.5


def dconv_ref(x, w, b, dilation=5):
    """(relu(conv3x3 dilation 5 + b) NHWC float64, t)"""
    xc = x.double().permute(0, 3, 1, 2)
    acc = F.conv2d(xc, w.double(), b.double(), padding=dilation, dilation=dilation)
    mag = F.conv2d(xc.abs(), w.double().abs(), b.double().abs(), padding=dilation, dilation=dilation)
    return F.relu(acc).permute(0, 2, 3, 1), (2 * gamma(578) * mag).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------- the pipeline decode
def decode_np(tp, size, input_size, score_threshold=0.1, distance_threshold=0.1, top_k=200):
    """numpy restatement of the upstream M-LSD decode, independent of gyre_amd.hinters.mlsd_decode: tp [B, 9, h, w] float32 -> a list
    of [n, 5] float32 arrays (x0, y0, x1, y1, score) in pixels of an image of size (H, W)"""
    tp = np.asarray(tp, dtype=np.float32)
    H, W = size
    out = []
    for b in range(tp.shape[0]):
        h, w = tp.shape[2:]
        heat = (1.0 / (1.0 + np.exp(-tp[b, 0].astype(np.float64)))).astype(np.float32)
        pad = np.full((h + 2, w + 2), -np.inf, dtype=np.float32)
        pad[1:-1, 1:-1] = heat
        peak = np.max(np.stack([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), 0)
        score = np.where(heat == peak, heat, np.float32(0)).ravel()
        order = np.argsort(-score, kind="stable")[:top_k]
        d = tp[b, 1:5].reshape(4, -1)
        rows = []
        for i in order:
            length = np.hypot(d[0, i] - d[2, i], d[1, i] - d[3, i])
            if score[i] > score_threshold and length > distance_threshold:
                x, y = np.float32(i % w), np.float32(i // w)
                rows.append([(x + d[0, i]) * 2 * np.float32(W / input_size), (y + d[1, i]) * 2 * np.float32(H / input_size),
                             (x + d[2, i]) * 2 * np.float32(W / input_size), (y + d[3, i]) * 2 * np.float32(H / input_size), score[i]])
        out.append(np.asarray(rows, dtype=np.float32).reshape(-1, 5))
    return out


def rasterise_np(lines, H, W):
    """numpy restatement of the rasteriser: n = max(|round(x1) - round(x0)|, |round(y1) - round(y0)|) + 1 points per segment, each
    rounded half to even (np.rint), the points outside the image dropped"""
    img = np.zeros((H, W), dtype=np.float32)
    for x0, y0, x1, y1 in np.asarray(lines, dtype=np.float32)[:, :4]:
        n = int(max(abs(np.rint(x1) - np.rint(x0)), abs(np.rint(y1) - np.rint(y0)))) + 1
        for i in range(n):
            t = np.float32(i) / np.float32(max(n - 1, 1))
            px, py = int(np.rint(x0 + (x1 - x0) * t)), int(np.rint(y0 + (y1 - y0) * t))
            if 0 <= px < W and 0 <= py < H:
                img[py, px] = 1
    return img
