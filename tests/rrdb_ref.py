"""CPU reference for the RRDBNet upscaler tests (imported by the tests, not collected).

net(sd, cfg, x, store)   BasicSR's RRDBNet forward (ESRGAN+ dense block when cfg["plus"]) over torch.nn.functional in fp32.  With
                         store = a 16-bit dtype, the weights, the image and every tensor the native graph keeps in memory are
                         rounded to it: the emulation whose distance from the fp32 net sets the model gates.
launch(...)              a dict describing ONE call of the dense-block convolution (kernels_rdb.hip): prefix source, optional
                         nearest 2x, slice output, epilogue
value64 / bound / emulate    float64 value, element-wise error bound, fp32 host emulation of such a call

The epilogue, in fp32 with one rounding to storage at the end:
    v = alpha (acc + bias);   v = v > 0 ? v : 0.2f v  (if act);   v = v + beta1 r1;   v = v + beta2 r2

Error bound.  u = 2^-8 (bf16) or 2^-11 (fp16), fl = half the smallest storage subnormal (2^-134, 2^-25), e = 2^-24.  Operands are
storage values, so each product is exact in fp32.  S = the sum of the K = 9 Cin products, A = the sum of their magnitudes.
    accumulation   |acc - S| <= 2 K e A     (any summation order gives (K - 1) e A to first order; doubled like tests/gemm_ref.py
                                             because the adder tree inside the MFMA is not documented)
    epilogue       at most 7 rounded operations (add bias, times alpha, times 0.2f, two products, two sums), each relative e on a
                   number no larger than  G = |alpha| (A + |bias|) + |beta1 r1| + |beta2 r2|;  leaky relu never amplifies an error
    t = |alpha| 2 K e A + 8 e G + 2^-146    (one e and the constant for second-order terms and fp32 underflow)
    bound = t + u (|E| + t) + fl            (E = the float64 value; one rounding to storage of something within t of it)
"""
import torch
import torch.nn.functional as F

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
E = 2.0 ** -24
FORMS = ("plain", "act", "block", "rrdb", "plus", "body")
MISTAKES = ("dropped_tap", "wrong_slice", "act_after_residual", "beta2_dropped", "rounded_before_residual")


def f32(v):
    """the float32 number nearest to v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------- the network
def net(sd, cfg, x, store=None):
    q = (lambda t: t) if store is None else (lambda t: t.to(store).float())
    wt = lambda name: q(sd[name + ".weight"].float())

    def c3(t, name):
        return F.conv2d(t, wt(name), sd[name + ".bias"].float(), padding=1)

    def lr(t):
        return F.leaky_relu(t, 0.2)

    def dense(t, p):
        parts = [t]
        for k in (1, 2, 3, 4):
            y = lr(c3(torch.cat(parts, 1), f"{p}.conv{k}"))
            if k == 2 and cfg.get("plus", False):
                y = y + q(F.conv2d(t, wt(p + ".conv1x1")))
            parts.append(q(y))
        return c3(torch.cat(parts, 1), p + ".conv5") * 0.2 + t          # not rounded here: the caller knows whether more follows

    r = {4: 1, 2: 2, 1: 4}[cfg["scale"]]
    t = q(x.float())
    if r > 1:
        t = F.pixel_unshuffle(t, r)
    first = q(c3(t, "conv_first"))
    t = first
    for i in range(cfg["num_block"]):
        keep = t
        t = q(dense(t, f"body.{i}.rdb1"))
        t = q(dense(t, f"body.{i}.rdb2"))
        t = q(dense(t, f"body.{i}.rdb3") * 0.2 + keep)
    t = q(first + c3(t, "conv_body"))
    for name in ("conv_up1", "conv_up2"):
        t = q(lr(c3(F.interpolate(t, scale_factor=2, mode="nearest"), name)))
    return q(c3(q(lr(c3(t, "conv_hr"))), "conv_last"))


# ------------------------------------------------------------------------------------------------------------ one kernel call
def launch(sdt, B, H, W, Cin, NT, live, ldx, ldo, c0, form="act", ups=0, lattice=False, seed=0):
    """Random (or exact-lattice) data for one call.  Source channels >= Cin are NaN, the output buffer is NaN everywhere except a
    "plus" call's own slice (its in-place residual).  lattice: integers in [-2, 2], about 16 non-zero +-1 weights per output channel,
    integer bias / residuals / factors - all partial sums are small integers, the result is an integer below 2^8."""
    assert form in FORMS
    g = torch.Generator().manual_seed(1000 * seed + 31 * H + 7 * W + Cin + NT + 3 * ups + FORMS.index(form))
    Ho, Wo = (2 * H, 2 * W) if ups else (H, W)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    rn = lambda *s: torch.randn(s, generator=g)
    if lattice:
        x, bias = ri(-2, 2, B, H, W, ldx), ri(-3, 3, live)
        w = ri(-1, 1, NT, 3, 3, Cin) * (torch.rand((NT, 3, 3, Cin), generator=g) < 16.0 / (9 * Cin)).float()
        res = lambda ld: ri(-4, 4, B, Ho, Wo, ld).to(sdt)
    else:
        x, bias = rn(B, H, W, ldx), 0.1 * rn(live)
        w = rn(NT, 3, 3, Cin) / (9 * Cin) ** 0.5
        res = lambda ld: rn(B, Ho, Wo, ld).to(sdt)
    w[live:] = 0
    x[..., Cin:] = float("nan")
    out = torch.full((B, Ho, Wo, ldo), float("nan")).to(sdt)
    L = dict(x=x.to(sdt), Cin=Cin, w=w.to(sdt), bias=bias, live=live, NT=NT, out=out, c0=c0, ups=ups,
             alpha=1.0, act=0, r1=None, beta1=0.0, r2=None, beta2=0.0, alias=False)
    if form in ("act", "plus"):
        L["act"] = 1
    if form == "plus":
        out[..., c0:c0 + live] = res(live)
        L.update(alias=True, r1=out[..., c0:c0 + live].clone(), beta1=1.0)
    if form in ("block", "body"):
        L.update(r1=res(64)[..., :live], beta1=1.0, alpha=1.0 if (lattice or form == "body") else 0.2)
    if form == "rrdb":
        L.update(r1=res(192)[..., :live], r2=res(64)[..., :live], beta2=1.0, alpha=1.0 if lattice else 0.04, beta1=2.0 if lattice else 0.2)
    return L


def _sum(L, dt, magnitudes=False, skip_last_tap=False):
    x = L["x"][..., :L["Cin"]].to(dt).permute(0, 3, 1, 2)
    w = L["w"][:L["live"]].to(dt).permute(0, 3, 1, 2).clone()
    if skip_last_tap:
        w[..., 2, 2] = 0
    if magnitudes:
        x, w = x.abs(), w.abs()
    if L["ups"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, padding=1).permute(0, 2, 3, 1)


def value64(L):
    """(E, A, G): float64 value of the written slice [B, Ho, Wo, live] and the two magnitudes of the bound"""
    d = torch.float64
    al, b1, b2 = f32(L["alpha"]), f32(L["beta1"]), f32(L["beta2"])
    bias = L["bias"].double()
    A = _sum(L, d, magnitudes=True)
    v = al * (_sum(L, d) + bias)
    if L["act"]:
        v = torch.where(v > 0, v, f32(0.2) * v)
    G = abs(al) * (A + bias.abs())
    for r, b in ((L["r1"], b1), (L["r2"], b2)):
        if r is not None:
            v = v + b * r.double()
            G = G + (b * r.double()).abs()
    return v, A, G


def bound(L):
    sdt = L["out"].dtype
    v, A, G = value64(L)
    t = abs(f32(L["alpha"])) * 2 * (9 * L["Cin"]) * E * A + 8 * E * G + 2.0 ** -146
    return v, t + U[sdt] * (v.abs() + t) + FL[sdt]


def steps32(acc, bias, alpha, act, r1, beta1, r2, beta2, mistake=None):
    """the epilogue on fp32 tensors, one rounded operation per line, before the rounding to storage"""
    one = lambda s: torch.tensor(s, dtype=torch.float32)
    leaky = lambda t: torch.where(t > 0, t, one(0.2) * t)
    v = acc if bias is None else acc + bias.float()
    v = one(alpha) * v
    late = mistake == "act_after_residual"
    if act and not late:
        v = leaky(v)
    if mistake == "rounded_before_residual" and r1 is not None:
        v = v.to(r1.dtype).float()
    if r1 is not None:
        v = v + one(beta1) * r1.float()
    if r2 is not None and mistake != "beta2_dropped":
        v = v + one(beta2) * r2.float()
    return leaky(v) if act and late else v


def emulate(L, mistake=None):
    """the output buffer after the call, computed on the host in fp32 (mistake: one of MISTAKES, for the self-test of the bound)"""
    assert mistake is None or mistake in MISTAKES
    acc = _sum(L, torch.float32, skip_last_tap=mistake == "dropped_tap")
    v = steps32(acc, L["bias"], L["alpha"], L["act"], L["r1"], L["beta1"], L["r2"], L["beta2"], mistake)
    buf = L["out"].clone()
    at = L["c0"] + (8 if mistake == "wrong_slice" else 0)
    buf[..., at:at + L["live"]] = v.to(buf.dtype)
    return buf


def lattice_expected(L):
    """What a lattice call must produce, bit for bit: ONE rounding to storage of the float64 value - every partial sum is a small
    integer, and where the leaky relu multiplies by 0.2f the product is rounded to fp32 and then to storage, which for these values
    is the rounding of the exact product (tests/test_rrdb_ref_host.py checks that the fp32 chain agrees).  The one exception is a call
    with the leaky relu AND a residual ("plus"): the residual can cancel 0.2f v down to the fp32 rounding of that product, which
    float64 keeps and fp32 cannot, so there the answer is defined by the fp32 operation chain over the exact accumulator - emulate()."""
    s = slice(L["c0"], L["c0"] + L["live"])
    if L["act"] and (L["r1"] is not None or L["r2"] is not None):
        return emulate(L)[..., s]
    return value64(L)[0].to(L["out"].dtype)


def verdict(L, got):
    """(worst |got - E| / bound over the slice, True when every element outside the slice still has the bits it had)"""
    v, bd = bound(L)
    s = slice(L["c0"], L["c0"] + L["live"])
    worst = float(((got[..., s].double() - v).abs() / bd).nan_to_num(nan=float("inf")).max())
    rest = torch.ones(got.shape[-1], dtype=torch.bool)
    rest[s] = False
    return worst, torch.equal(bits(got)[..., rest], bits(L["out"])[..., rest])


def epilogue_inplace(buf, c0, live, bias, alpha, act, r1, beta1, r2, beta2):
    """k_rdb_epilogue on the host: buf[..., c0:c0+live] is both the accumulator and the destination"""
    out = buf.clone()
    out[..., c0:c0 + live] = steps32(buf[..., c0:c0 + live].float(), bias, alpha, act, r1, beta1, r2, beta2).to(buf.dtype)
    return out


def unshuffle(x, r, sdt):
    """k_pixel_unshuffle on the host: NCHW -> NHWC storage in pixel_unshuffle(r) channel order, zero channels up to a multiple of 32"""
    y = (F.pixel_unshuffle(x.float(), r) if r > 1 else x.float()).permute(0, 2, 3, 1)
    return F.pad(y, (0, -y.shape[-1] % 32)).to(sdt).contiguous()
