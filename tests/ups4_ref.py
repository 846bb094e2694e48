"""The four-parity form of an upsampler convolution (GemmParams::ups4, csrc/kernels.h), stated in Python.  CPU only: no GPU import.

nearest 2x followed by a 3x3 / pad 1 convolution reads, for an output pixel (Y, X) = (2 i + a, 2 j + b), only the 2 x 2 source pixels
with origin (i - 1 + a, j - 1 + b): per parity (a, b) it is a 2x2 convolution of the SOURCE image with weights that are sums of the
nine taps, and the zero border of the upsampled image is the zero border of the source.

  compose(W)        the four [N][2][2][C] matrices from W [N][3][3][C]; optionally each sum rounded once to a storage type
  forward(x, Wc)    the four 2x2 convolutions, every result row scattered to the output row of its pixel
  blocked(Wc)       the [4 N][4 C] matrix (rows parity * N + n, K = tap * C + c, tap = 2 ty + tx) in the 1-KiB blocked weight order

`bug` seeds a mistake (tests/test_ups4_ref_host.py shows that each is caught by the comparison with gemm_ref.conv_gather)."""
import torch

F64 = torch.float64


def tap_groups(parity_bit, bug=None):
    """Nine-tap offsets k (0 .. 2) that land on 2x2 tap t = 0 / 1 along one axis, for output parity a (or b)."""
    if parity_bit == 0 or bug == "a1_grouping":
        return ([0], [1, 2])
    return ([0, 1], [2])


def compose(W, hdt=None, bug=None):
    """W [N][3][3][C] -> [4][N][2][2][C] (parity 2 a + b): ky ascending outer, kx ascending inner; hdt: one rounding of each sum."""
    N, _, _, Cc = W.shape
    W = W.to(F64)
    out = torch.zeros(4, N, 2, 2, Cc, dtype=F64)
    for a in (0, 1):
        for b in (0, 1):
            gy = tap_groups(a, bug if bug == "a1_grouping" else None)
            gx = tap_groups(b)
            for ty in (0, 1):
                for tx in (0, 1):
                    for ky in gy[ty]:
                        for kx in gx[tx]:
                            out[2 * a + b, :, ty, tx] += W[:, ky, kx]
    return out if hdt is None else out.to(torch.float32).to(hdt).to(F64)


def out_rows(B, Hi, Wi, a, b, bug=None):
    """Output row of every source pixel (n, i, j), row-major over (n, i, j), for parity (a, b)."""
    n = torch.arange(B)[:, None, None]
    i = torch.arange(Hi)[None, :, None]
    j = torch.arange(Wi)[None, None, :]
    if bug == "hw_swapped":
        return (n * 4 * Hi * Wi + (2 * j + b) * 2 * Hi + 2 * i + a).reshape(-1)       # the row map of the transposed image
    return (n * 4 * Hi * Wi + (2 * i + a) * 2 * Wi + 2 * j + b).reshape(-1)


def gather2(x, a, b, bug=None):
    """x [B][Hi][Wi][C] -> [B Hi Wi][4][C]: the 2x2 window with origin (i - 1 + a, j - 1 + b), zeros outside the image."""
    B, Hi, Wi, Cc = x.shape
    taps = []
    for ty in (0, 1):
        for tx in (0, 1):
            iy = torch.arange(Hi) - 1 + a + ty
            ix = torch.arange(Wi) - 1 + b + tx
            oky, okx = (iy >= 0) & (iy < Hi), (ix >= 0) & (ix < Wi)
            if bug == "replicate":
                oky, okx = torch.ones_like(oky), torch.ones_like(okx)
            g = x[:, iy.clamp(0, Hi - 1)][:, :, ix.clamp(0, Wi - 1)]
            taps.append(g * (oky[:, None] & okx[None, :]).to(x.dtype)[None, :, :, None])
    return torch.stack(taps, dim=3).reshape(B * Hi * Wi, 4, Cc)


def forward(x, Wc, bug=None, absolute=False):
    """x [B][Hi][Wi][C], Wc [4][N][2][2][C] (compose) -> [B 2Hi 2Wi][N] float64 (absolute: the sum of |x| |w| instead)."""
    B, Hi, Wi, Cc = x.shape
    N = Wc.shape[1]
    x = x.to(F64)
    out = torch.zeros(B * 4 * Hi * Wi, N, dtype=F64)
    for a in (0, 1):
        for b in (0, 1):
            A = gather2(x, a, b, bug).reshape(B * Hi * Wi, 4 * Cc)
            Wm = Wc[2 * a + b].reshape(N, 4 * Cc)
            out[out_rows(B, Hi, Wi, a, b, bug)] = (A.abs() @ Wm.abs().T) if absolute else (A @ Wm.T)
    return out


def blocked(Wc):
    """[4][N][2][2][C] -> the flat blocked order of the [4 N][4 C] matrix: block (r >> 3, k >> 6) of 8 rows x 64 k, row-major inside."""
    P, N, _, _, Cc = Wc.shape
    R, K = P * N, 4 * Cc
    assert R % 8 == 0 and K % 64 == 0
    m = Wc.reshape(R, K)
    return m.reshape(R // 8, 8, K // 64, 64).permute(0, 2, 1, 3).reshape(-1)


def oracle_with_rounded_upsamplers(M, sd, cfg, inputs, hdt, composed, store=False):
    """The fp32 oracle's UNet answer with every upsampler conv's weight rounded to `hdt` (composed = False), or with those convs
    computed in the four-parity form on composed weights rounded once more to `hdt` (composed = True): the two differ by the one
    extra weight rounding of the form and nothing else.  store = True: the output of every convolution, linear layer and GroupNorm
    is rounded to `hdt` as well, in both runs - the device keeps its activations in 16 bits, and a perturbation d that meets a rounding
    step of spacing u comes out of it as 0 or u, with root mean square about sqrt(d u) > d: an emulation in fp32 activations would
    model a machine on which the extra rounding stays as small as it went in.  M: oracle.models_ref."""
    plain, plain_lin, plain_gn = M._conv, M._lin, M._gn

    def rnd(y, p=""):
        return y.to(hdt).to(y.dtype) if store and p != "conv_out" else y

    def conv(x, sd_, p, stride=1, padding=1):
        if not p.endswith("upsamplers.0.conv"):
            return rnd(plain(x, sd_, p, stride, padding), p)
        w = sd_[p + ".weight"].to(hdt).to(F64)                               # [N][C][3][3], as the device stores it
        b = sd_[p + ".bias"].to(F64)
        B, Cc, H2, W2 = x.shape
        if not composed:
            return rnd(torch.nn.functional.conv2d(x.to(F64), w, b, padding=1).to(x.dtype))
        src = x[:, :, ::2, ::2].permute(0, 2, 3, 1).to(F64)                  # the image before the nearest 2x
        y = forward(src, compose(w.permute(0, 2, 3, 1), hdt=hdt)) + b
        return rnd(y.reshape(B, H2, W2, -1).permute(0, 3, 1, 2).to(x.dtype))
    M._conv = conv
    M._lin = lambda x, sd_, p: rnd(plain_lin(x, sd_, p))
    M._gn = lambda x, sd_, p, groups, eps: rnd(plain_gn(x, sd_, p, groups, eps))
    try:
        return M.unet_forward(sd, cfg, *inputs)
    finally:
        M._conv, M._lin, M._gn = plain, plain_lin, plain_gn
