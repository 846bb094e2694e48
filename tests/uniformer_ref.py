"""Plain float64 restatement of the UniFormer backbone of the segmentation annotator (the reference's gyre/pipeline/hinters/models/
uniformer.py with global attention in stages 3 and 4) and of the kernels of kernels_uniformer.hip, the reference of
tests/test_uniformer_ref_host.py and tests/test_gpu_uniformer.py.  Maps are NHWC [B, H, W, C] float64 throughout.

fold         a BatchNorm (eval) in front of a 1x1 convolution folded into it: W' = W diag(s), b' = b + W (beta - mean s), s = gamma /
             sqrt(var + eps) - exact, the norm feeds the convolution directly
local        x + conv2(dw5x5(conv1'(x))): the 5x5's zero padding is applied to conv1'(x), so a position outside the map contributes 0;
             halo_bias=True is the seeded MISTAKE of padding x instead, which puts conv1'(0) = b1 there
local_bound  the element-wise error bound of k_uf_local (derivation: docstring of tests/test_gpu_uniformer.py)
gather       space-to-depth by 2 with floor division, column (2 dy + dx) C + c
net          the four maps of UniFormer.forward(x).  rnd: a function applied to every tensor the native graph stores (identity by
             default; the storage emulation of the model bar passes a rounding), the folded weights included
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def fold(w, b, bn, rnd=lambda t: t):
    """w [O, I], b [O], bn = (gamma, beta, mean, var) -> (W', b')"""
    g, beta, mean, var = bn
    s = g / torch.sqrt(var + BN_EPS)
    return rnd(w * s), b + w @ (beta - mean * s)


def dw(x, w, b, pad_value=None):
    """depthwise k x k, w [C, 1, k, k]; the padding is zero, or pad_value [C]"""
    k = w.shape[-1] // 2
    xp = F.pad(x.permute(0, 3, 1, 2), (k, k, k, k))
    if pad_value is not None:
        inside = F.pad(torch.ones_like(x[..., :1]).permute(0, 3, 1, 2), (k, k, k, k))
        xp = xp + (1 - inside) * pad_value.view(1, -1, 1, 1)
    return F.conv2d(xp, w, b, groups=x.shape[-1]).permute(0, 2, 3, 1)


def cpe(x, w, b):
    return x + dw(x, w, b)


def local(x, w1, b1, wd, bd, w2, b2, rnd=lambda t: t, halo_bias=False):
    t = rnd(x @ w1.T + b1)
    d = rnd(dw(t, wd, bd, rnd(b1) if halo_bias else None))
    return rnd(x + d @ w2.T + b2)


def local_bound(x, w1, b1, wd, bd, w2, b2, u, fl):
    """(value, bound) of local() for storage-valued x, w1, w2 and fp32 b1, wd, bd, b2: u = the storage rounding unit, fl = half its
    smallest subnormal, e = 2^-24"""
    e, C = 2.0 ** -24, x.shape[-1]
    t = x @ w1.T + b1
    dt = (2 * C + 2) * e * (x.abs() @ w1.abs().T + b1.abs())              # C products of an MFMA chain, doubled; the bias add
    dt = dt + u * (t.abs() + dt) + fl                                      # one rounding to storage (exact zeros outside the map)
    d = dw(t, wd, bd)
    dd = dw(dt, wd.abs(), None) + 26 * e * dw(t.abs() + dt, wd.abs(), bd.abs())       # the error of t through the taps; 25 fma and bd
    dd = dd + u * (d.abs() + dd) + fl
    val = x + d @ w2.T + b2
    dy = dd @ w2.abs().T + (2 * C + 3) * e * ((d.abs() + dd) @ w2.abs().T + b2.abs() + x.abs())
    return val, dy + u * (val.abs() + dy) + fl


def local_case(C, H, W, sdt, B=2):
    """storage-valued operands of one k_uf_local call, float64; the conv1 bias is LARGE against the activations"""
    g = torch.Generator().manual_seed(1000 * C + 37 * H + W)
    r = lambda *s: torch.randn(s, generator=g)
    x, w1, w2 = r(B, H, W, C).to(sdt).double(), (r(C, C) / C ** 0.5).to(sdt).double(), (r(C, C) / C ** 0.5).to(sdt).double()
    return x, w1, (4 * r(C)).double(), (0.3 * r(C, 1, 5, 5)).double(), (0.2 * r(C)).double(), w2, (0.2 * r(C)).double()


def gather(x):
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, 4 * C)


def net(sd, cfg, x, rnd=lambda t: t):
    """the four maps of UniFormer.forward(x) for the state dict sd (float64 tensors) and cfg (layers, embed_dim); x NCHW"""
    ln = lambda t, p, eps: F.layer_norm(t, t.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], eps)
    lin = lambda t, p: F.linear(t, sd[p + ".weight"].flatten(1), sd[p + ".bias"])
    bn = lambda p: tuple(sd[p + k] for k in (".weight", ".bias", ".running_mean", ".running_var"))
    t, outs = rnd(x.double()), []
    for i, depth in enumerate(cfg["layers"]):
        p = f"patch_embed{i + 1}"
        k = 2 if i else 4
        t = rnd(F.conv2d(t, sd[p + ".proj.weight"], sd[p + ".proj.bias"], stride=k).permute(0, 2, 3, 1))
        t = rnd(ln(t, p + ".norm", 1e-5))
        C = t.shape[-1]
        for j in range(depth):
            p = f"blocks{i + 1}.{j}"
            u = rnd(cpe(t, sd[p + ".pos_embed.weight"], sd[p + ".pos_embed.bias"]))
            if i < 2:
                w1, b1 = fold(sd[p + ".conv1.weight"].flatten(1), sd[p + ".conv1.bias"], bn(p + ".norm1"), rnd)
                v = local(u, w1, b1, sd[p + ".attn.weight"], sd[p + ".attn.bias"], sd[p + ".conv2.weight"].flatten(1), sd[p + ".conv2.bias"], rnd)
                wf, bf = fold(sd[p + ".mlp.fc1.weight"].flatten(1), sd[p + ".mlp.fc1.bias"], bn(p + ".norm2"), rnd)
                hdn = rnd(F.gelu(rnd(v @ wf.T + bf)))
            else:
                B, h, w, _ = u.shape
                qkv = rnd(lin(rnd(ln(u, p + ".norm1", 1e-6)), p + ".attn.qkv")).view(B, h * w, 3, C // 64, 64).permute(2, 0, 3, 1, 4)
                a = torch.softmax(qkv[0] @ qkv[1].transpose(-2, -1) * 64 ** -0.5, -1) @ qkv[2]
                v = rnd(u + lin(rnd(a.transpose(1, 2).reshape(B, h, w, C)), p + ".attn.proj"))
                hdn = rnd(F.gelu(rnd(lin(rnd(ln(v, p + ".norm2", 1e-6)), p + ".mlp.fc1"))))
            t = rnd(v + lin(hdn, p + ".mlp.fc2"))
        outs.append(rnd(ln(t, f"norm{i + 1}", 1e-6)).permute(0, 3, 1, 2).contiguous())
        t = t.permute(0, 3, 1, 2)
    return outs


TINY = dict(layers=[1, 2, 2, 1], embed_dim=[64, 128, 192, 256])


def seeded_state_dict(shapes, seed=0):
    """fp32 weights of a size at which every layer matters: matrices ~ N(0, 1.5^2 / fan_in), norms near one, biases and running means
    nonzero, running variances in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes.items():
        if k.endswith("num_batches_tracked"):
            continue
        r = torch.randn(s, generator=g)
        if k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(s, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.2 * r
        elif "norm" in k:
            sd[k] = 1 + 0.1 * r if k.endswith("weight") else 0.1 * r
        elif k.endswith(".bias"):
            sd[k] = 0.2 * r
        else:
            sd[k] = r * (1.5 / torch.Size(s[1:]).numel() ** 0.5)
    return sd
