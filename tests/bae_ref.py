"""Plain float64 restatement of the BAE surface-normal decoder in test mode (the reference's gyre/pipeline/hinters/baenormal/submodules/
decoder.py, architecture 'BN') and of the kernels of kernels_bae.hip, the reference of tests/test_reference_bae.py and
tests/test_gpu_bae.py.  Maps are NCHW float64 throughout.

decoder / up_block / refine_stage / norm_normalize: the reference's operations in its order.  rnd, where given, rounds every tensor the
native graph stores in its 16-bit type (entry maps, resized map, folded weights, each convolution's output before and after its
activation, the prediction a stage reads, the hidden activations in front of layers 2 and 3) and folds the BatchNorms as finalize does:
the storage emulation of the whole-decoder gate.  refine_bound / lerp_bound: the element-wise error bounds of k_bae_refine (raw output)
and of the fp32 lerp (derivation: docstring of tests/test_gpu_bae.py).
"""
import torch
import torch.nn.functional as F

TINY = dict(num_features=512, skip_features=(8, 16, 24, 40))
E = 2.0 ** -24


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def norm_normalize(o):
    x, y, z, k = torch.split(o, 1, dim=1)
    n = torch.sqrt(x ** 2.0 + y ** 2.0 + z ** 2.0) + 1e-10
    return torch.cat([x / n, y / n, z / n, F.elu(k) + 1.0 + 0.01], dim=1)


def interp(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True)


def taps(n_in, n_out):
    """(i0, i1, l1) of align_corners=True, exact: src = dst (in - 1) / (out - 1).  A source that IS a pixel other than the first is
    written as the end of the segment before it (l1 = 1): the same value, and the corner an fp32 coordinate just below it reads"""
    dst = torch.arange(n_out)
    num, den = dst * (n_in - 1), max(n_out - 1, 1)
    i0, rem = num // den, num % den
    end = (rem == 0) & (i0 > 0)
    i0, rem = i0 - end.long(), torch.where(end, torch.full_like(rem, den), rem)
    return i0, (i0 + 1).clamp(max=n_in - 1), rem.double() / den


def corners(t, Ho, Wo):
    """the four corner maps (a, b, c, d) of t at the output size and the weights: value = ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d)"""
    y0, y1, ly = taps(t.shape[2], Ho)
    x0, x1, lx = taps(t.shape[3], Wo)
    r0, r1 = t[:, :, y0], t[:, :, y1]
    return (r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]), ly.view(-1, 1), lx.view(1, -1)


def lerp(c, ly, lx):
    return (1 - ly) * ((1 - lx) * c[0] + lx * c[1]) + ly * ((1 - lx) * c[2] + lx * c[3])


def lerp_bound(t, dt, Ho, Wo):
    """(value, bound) of the fp32 lerp of t (known to dt) at Ho x Wo.  Per axis the coordinate fl(fl(s) dst) is within 2 e src of the
    exact one, l1 = src - i0 is exact and l0 = fl(1 - l1) adds e: (2 src + 2) e with a spare; each of the four weights moves by at most the
    sum of the two axes, and the five roundings of h0 (w0 a + w1 b) + h1 (w0 c + w1 d) add 6 e of the corner sum with a spare"""
    c, ly, lx = corners(t, Ho, Wo)
    dc, _, _ = corners(dt, Ho, Wo)
    s4 = sum(v.abs() + dv for v, dv in zip(c, dc))
    srcy = torch.arange(Ho).double().view(-1, 1) * (t.shape[2] - 1) / max(Ho - 1, 1)
    srcx = torch.arange(Wo).double().view(1, -1) * (t.shape[3] - 1) / max(Wo - 1, 1)
    return lerp(c, ly, lx), lerp(dc, ly, lx) + ((2 * srcy + 2) + (2 * srcx + 2) + 6) * E * s4


def fold(w, b, bn, rnd):
    g, beta, mean, var = bn
    s = g / torch.sqrt(var + 1e-5)
    return rnd(w * s.view(-1, 1, 1, 1)), beta + (b - mean) * s


def up_block(sd, p, x, skip, rnd=None):
    f = torch.cat([interp(x, skip.shape[2:]) if rnd is None else rnd(interp(x, skip.shape[2:])), skip], dim=1)
    for j in (0, 3):
        w, b = sd[f"{p}.{j}.weight"], sd[f"{p}.{j}.bias"]
        bn = [sd[f"{p}.{j + 1}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]
        if rnd is None:
            f = F.leaky_relu(F.batch_norm(F.conv2d(f, w, b, padding=1), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5), 0.01)
        else:
            f = rnd(F.leaky_relu(rnd(F.conv2d(f, *fold(w, b, bn, rnd), padding=1)), 0.01))
    return f


def refine_stage(sd, p, x, pred, normalize=True, rnd=None):
    r = rnd or (lambda t: t)
    B, _, H, W = x.shape
    f = torch.cat([interp(x, (2 * H, 2 * W)), interp(r(pred), (2 * H, 2 * W))], dim=1).view(B, -1, 4 * H * W)
    f = r(F.relu(F.conv1d(f, sd[p + ".0.weight"], sd[p + ".0.bias"])))
    f = r(F.relu(F.conv1d(f, sd[p + ".2.weight"], sd[p + ".2.bias"])))
    f = F.relu(F.conv1d(f, sd[p + ".4.weight"], sd[p + ".4.bias"]))
    o = F.conv1d(f, sd[p + ".6.weight"], sd[p + ".6.bias"]).view(B, 4, 2 * H, 2 * W)
    return norm_normalize(o) if normalize else o


def decoder(sd, blocks, rnd=None):
    """[out_res8, out_res4, out_res2, out_res1] for blocks = [x_block0 .. x_block4]"""
    r = rnd or (lambda t: t)
    b = [r(t) for t in blocks]
    d = [r(F.conv2d(b[4], r(sd["conv2.weight"]), sd["conv2.bias"]))]
    for k in range(4):
        d.append(up_block(sd, f"up{k + 1}._net", d[-1], b[3 - k], rnd))
    outs = [norm_normalize(r(F.conv2d(d[2], r(sd["out_conv_res8.weight"]), sd["out_conv_res8.bias"], padding=1)))]
    for k, name in enumerate(("out_conv_res4", "out_conv_res2", "out_conv_res1")):
        outs.append(refine_stage(sd, name, d[2 + k], outs[-1], True, rnd))
    return outs


def refine_bound(x, pred, w1, b1, w2, b2, w3, b3, w4, b4, u, fl):
    """(value, bound) of the raw output of k_bae_refine for storage-valued x, w1, w2, w3 and fp32 pred, biases, w4: u = the storage
    rounding unit, fl = half its smallest subnormal; w: [O, I] matrices"""
    B, CF, Hs, Ws = x.shape
    mm = lambda w, t: torch.einsum("oi,bihw->bohw", w, t)
    bias = lambda b: b.view(1, -1, 1, 1)
    f = torch.cat([x, pred], dim=1)
    t = mm(w1, f) + bias(b1)
    dp = u * pred.abs() + fl                                                               # the prediction is rounded to storage
    dt = mm(w1[:, CF:].abs(), dp) + (2 * (CF + 4) + 2) * E * (mm(w1.abs(), f.abs()) + mm(w1[:, CF:].abs(), dp) + bias(b1.abs()))
    a, da = lerp_bound(t, dt, 2 * Hs, 2 * Ws)                                              # t stays fp32: no rounding of its own
    h, dh = F.relu(a), da
    for w, b, rounded in ((w2, b2, True), (w3, b3, True), (w4, b4, False)):
        if rounded:
            dh = dh + u * (h + dh) + fl                                                    # the one rounding of an MFMA operand
        z = mm(w, h) + bias(b)
        dz = mm(w.abs(), dh) + (2 * 128 + 4) * E * (mm(w.abs(), h + dh) + bias(b.abs()))   # chains of 32 doubled, the bias, the shuffles
        h, dh = (F.relu(z), dz) if w.shape[0] == 128 else (z, dz)
    return h, dh


def refine_case(CF, Hs, Ws, sdt, B=2):
    """operands of one k_bae_refine call as a state dict of one stage ("s.0.weight" ...), float64: x and the matrices the MFMAs read are
    storage values, the layer-1 bias is LARGE against the activations and the prediction's columns have the size of the others"""
    g = torch.Generator().manual_seed(1000 * CF + 37 * Hs + Ws)
    r = lambda *s: torch.randn(s, generator=g)
    q = lambda t: t.to(sdt).double()
    sd = {"s.0.weight": q(r(128, CF + 4, 1) / CF ** 0.5), "s.0.bias": (4 * r(128)).double(),
          "s.2.weight": q(r(128, 128, 1) / 8), "s.2.bias": (0.5 * r(128)).double(),
          "s.4.weight": q(r(128, 128, 1) / 8), "s.4.bias": (0.5 * r(128)).double(),
          "s.6.weight": (r(4, 128, 1) / 8).double(), "s.6.bias": r(4).double()}
    return q(r(B, CF, Hs, Ws)), norm_normalize(r(B, 4, Hs, Ws)).double(), sd


def seeded_state_dict(shapes, seed=0):
    """fp32 weights of a size at which every layer matters: matrices ~ N(0, 1.5^2 / fan_in), BatchNorm weights near one, biases and running
    means nonzero, running variances in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes.items():
        if k.endswith("num_batches_tracked"):
            continue
        r = torch.randn(s, generator=g)
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(s, generator=g)
        elif k.endswith("running_mean") or k.endswith(".bias"):
            sd[k] = 0.2 * r
        elif len(s) == 1:
            sd[k] = 1 + 0.1 * r
        else:
            sd[k] = r * (1.5 / torch.Size(s[1:]).numel() ** 0.5)
    return sd


def features(blocks):
    """the encoder's feature list with x_block0 .. x_block4 at the entries the decoder reads"""
    return [blocks[(4, 5, 6, 8, 11).index(i)] if i in (4, 5, 6, 8, 11) else None for i in range(12)]


def seeded_blocks(cfg, B, H, W, seed=1):
    g, out = torch.Generator().manual_seed(seed), []
    for c in (*cfg["skip_features"], cfg["num_features"]):
        out.append(torch.randn((B, c, H, W), generator=g))
        H, W = -(-H // 2), -(-W // 2)
    return out
