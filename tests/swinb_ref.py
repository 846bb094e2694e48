"""Plain float64 restatement of the Swin-B backbone of InSPyReNet (the reference's gyre/pipeline/hinters/inspyrenet/backbones/
SwinTransformer.py at window 12), the reference of tests/test_swinb_ref_host.py and tests/test_gpu_swinb.py.

win_attn     SwinTransformerBlock.forward between qkv and proj on a map [B, H, W]: the map is padded to multiples of 12 with the value
             a zero token projects to (the qkv bias), rolled by -shift, partitioned; logits = scale q k^T + bias[index] + mask, the
             mask being BasicLayer.forward's -100 between the nine regions of the PADDED map; softmax; P V; reversed, rolled back, cropped.
net          patch embedding (zero-padded to a multiple of 4) + norm, four stages of blocks (shift 6 in every odd block), the
             stage norms, patch merging on zero-padded odd maps.  rnd: a function applied to every tensor the native graph stores
             (identity by default; the storage emulation of the model bar passes a rounding).
"""
import torch
import torch.nn.functional as F

WS = 12


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def relative_position_index():
    c = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (WS - 1)
    return rel[..., 0] * (2 * WS - 1) + rel[..., 1]


def region_mask(Hp, Wp, shift):
    """[nW, 144, 144]: -100 where the two tokens of a window lie in different regions of the padded, shifted map"""
    img = torch.zeros((Hp, Wp))
    cnt = 0
    for hs in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
        for ws in (slice(0, -WS), slice(-WS, -shift), slice(-shift, None)):
            img[hs, ws] = cnt
            cnt += 1
    mw = img.view(Hp // WS, WS, Wp // WS, WS).permute(0, 2, 1, 3).reshape(-1, WS * WS)
    return torch.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0).double()


def win_attn(qkv, pad_value, table, heads, shift, detail=False):
    """qkv [B, H, W, 96 heads] float64 -> o [B, H, W, 32 heads]; pad_value [96 heads]: q / k / v of a padded token.  detail: also the
    pieces the element-wise bound needs, in window order, and the function that brings a window-ordered tensor back to the map"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    x = pad_value.view(1, 1, 1, C3).expand(B, Hp, Wp, C3).clone()
    x[:, :H, :W] = qkv
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    nW = (Hp // WS) * (Wp // WS)
    xw = x.view(B, Hp // WS, WS, Wp // WS, WS, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, WS * WS, 3, heads, 32).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0], xw[1], xw[2]
    bias = table.double()[relative_position_index().view(-1)].view(WS * WS, WS * WS, heads).permute(2, 0, 1).unsqueeze(0)
    mask = region_mask(Hp, Wp, shift).repeat(B, 1, 1).unsqueeze(1) if shift else None
    scale = float(torch.tensor(32.0 ** -0.5, dtype=torch.float32))
    l = scale * (q @ k.transpose(-2, -1)) + bias + (mask if shift else 0.0)

    def back(ow):
        o = ow.transpose(1, 2).reshape(B, Hp // WS, Wp // WS, WS, WS, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)
        if shift:
            o = torch.roll(o, (shift, shift), (1, 2))
        return o[:, :H, :W]
    o = back(torch.softmax(l, -1) @ v)
    return (o, dict(q=q, k=k, v=v, bias=bias, mask=mask, l=l, scale=scale, back=back)) if detail else o


def net(sd, cfg, x, rnd=lambda t: t):
    """the five maps of SwinTransformer.forward(x) for the state dict sd (float64 tensors) and cfg (embed_dim, depths, num_heads)"""
    d = torch.float64
    E = cfg["embed_dim"]
    ln = lambda t, p: F.layer_norm(t, t.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], 1e-5)
    lin = lambda t, p: F.linear(t, sd[p + ".weight"], sd.get(p + ".bias"))
    B, _, H, W = x.shape
    x = F.pad(rnd(x.to(d)), (0, -W % 4, 0, -H % 4))
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=4).permute(0, 2, 3, 1)
    t = rnd(ln(t, "patch_embed.norm"))
    outs = [t.permute(0, 3, 1, 2).contiguous()]
    for i, depth in enumerate(cfg["depths"]):
        heads = cfg["num_heads"][i]
        for j in range(depth):
            p = f"layers.{i}.blocks.{j}"
            qkv = rnd(lin(rnd(ln(t, p + ".norm1")), p + ".attn.qkv"))
            ao = rnd(win_attn(qkv, rnd(sd[p + ".attn.qkv.bias"]), sd[p + ".attn.relative_position_bias_table"], heads, 6 if j % 2 else 0))
            t = rnd(t + lin(ao, p + ".attn.proj"))
            hdn = rnd(F.gelu(rnd(lin(rnd(ln(t, p + ".norm2")), p + ".mlp.fc1"))))
            t = rnd(t + lin(hdn, p + ".mlp.fc2"))
        outs.append(rnd(ln(t, f"norm{i}")).permute(0, 3, 1, 2).contiguous())
        if i < 3:
            h, w = t.shape[1:3]
            t = F.pad(t, (0, 0, 0, w % 2, 0, h % 2))
            t = torch.cat([t[:, 0::2, 0::2], t[:, 1::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 1::2]], -1)
            t = rnd(lin(rnd(ln(t, f"layers.{i}.downsample.norm")), f"layers.{i}.downsample.reduction"))
    return outs


TINY = dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])


def seeded_state_dict(shapes, seed=0):
    """fp32 weights of a size at which every layer matters: matrices ~ N(0, 1 / fan_in) scaled up, norms near one, tables ~ N(0, 0.5)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes.items():
        if k.endswith("relative_position_index"):
            continue
        r = torch.randn(s, generator=g)
        if k.endswith("bias_table"):
            sd[k] = 0.5 * r
        elif "norm" in k:
            sd[k] = 1 + 0.1 * r if k.endswith("weight") else 0.1 * r
        elif k.endswith(".bias"):
            sd[k] = 0.2 * r
        else:
            fan_in = 1
            for n in s[1:]:
                fan_in *= n
            sd[k] = r * (1.5 / fan_in ** 0.5)
    return sd
