"""fp32 restatement of the two T2I adapters over a state dict (torch.nn.functional only): the reference for the native model
(tests/test_gpu_t2i.py), itself checked against arrays the reference's own classes produced (tests/golden/t2i_vectors.npz,
tests/test_t2i_host.py).  cfg: the mapping gyre_amd.config.t2i_config returns."""
import torch
import torch.nn.functional as F


def _conv(x, sd, p, stride=1):
    w = sd[p + ".weight"]
    return F.conv2d(x, w, sd[p + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def _pair(x, sd, p, res):
    return _conv(F.relu(_conv(x, sd, p + ".block1")), sd, p + ".block2") + res


def t2i_forward(sd, cfg, image):
    """image [B, cin // 64, H, W] -> list of one feature map per level."""
    sd = {k: v.to(torch.float32) for k, v in sd.items()}
    x = F.pixel_unshuffle(image.to(torch.float32), 8)
    feats = []
    levels, nums_rb = len(cfg["channels"]), cfg["nums_rb"]
    if cfg.get("type", "main") == "light":
        for i in range(levels):
            p = f"body.{i}"
            if i:
                x = F.avg_pool2d(x, 2, 2)
            x = _conv(x, sd, p + ".in_conv")
            for j in range(nums_rb):
                x = _pair(x, sd, f"{p}.body.{j}", x)
            x = _conv(x, sd, p + ".out_conv")
            feats.append(x)
        return feats
    x = _conv(x, sd, "conv_in")
    for i in range(levels):
        for j in range(nums_rb):
            p = f"body.{i * nums_rb + j}"
            if i and j == 0:
                x = _conv(x, sd, p + ".down_opt.op", stride=2) if cfg["use_conv"] else F.avg_pool2d(x, 2, 2)
            if p + ".in_conv.weight" in sd:
                x = _conv(x, sd, p + ".in_conv")
            x = _pair(x, sd, p, _conv(x, sd, p + ".skep") if p + ".skep.weight" in sd else x)
        feats.append(x)
    return feats
