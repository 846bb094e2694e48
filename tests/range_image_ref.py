"""Builders, exponent derivation, judges and host emulations for the range-edge family of the image-model kernels
(tests/range_image_cases.py).  CPU only.  TEST INFRASTRUCTURE shared by tests/test_range_image_ref_host.py (CPU) and
tests/test_gpu_range_image.py (-m gpu).

The operations are not restated: hed_ref, lineart_ref, hat_ref, swinir_ref, ctrl_ref, rrdb_ref and norm_fwd_ref hold the float64
values and the element-wise bounds every row is judged with; range_ref holds k_top, quantised, excluded_mask, check1, judge_scaling,
cast_specials and same_bits.

Every op has four functions, found through OPS[row["op"]]:
  base(row, hdt)              the O(1) BASE problem: a dict of tensors holding storage values (and fp32 parameters)
  derive(row, P, hdt)         the exponents, from the base problem and its float64 reference alone
  scaled(row, P, exps, hdt)   the SCALED problem
  outputs(row, P, hdt)        what a run must produce: name -> Out(value float64, tol float64 absolute, odt, k, exact)
                              k: the power of two between base and scaled run (check 1); exact: the stored value is ONE rounding of
                              `value` (lattice rows, moved values) and nothing is excluded from check 1
                              sure: (saturating sigmoids) the elements whose expectation is exact - the others, base logits within twice
                              their fp32 error bound of zero, may come out as any number in [0, 1] and count as excluded
  emulate(row, P, hdt, mistake=None)    name -> tensor: a correct kernel's stored outputs on the host, or one with a seeded mistake
The GPU test supplies launch(row, P) with the same output names.  judge() applies check 1 and check 2 to all outputs of a row and
prints its one `[range]` line.

Exponents.  fp16: the largest k that keeps the scaled float64 maximum (of the operands that are scaled and of the outputs) <= 65504,
which puts it in (top / 2, top].  bf16 stores in fp32's exponent range: the binding limit is the largest fp32 intermediate in
absolute-value form, <= 2^126.  Subnormal rows: the quantum of the data times 2^k is 2^-24, the fp16 subnormal lattice; the bf16
flavour runs the same numbers."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

import ctrl_ref as CR
import hat_ref as HT
import hed_ref as HD
import lineart_ref as LA
import norm_fwd_ref as N
import range_ref as R
import rrdb_ref as RB
import swinir_ref as SW

F64, F32 = torch.float64, torch.float32
NAME, TOP, NORMAL_MIN = R.NAME, R.TOP, R.NORMAL_MIN
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
FL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}
E = 2.0 ** -24
DT = R.SRC_DT
SAT = 128.0                              # |logit| from which 1 / (1 + exp(-l)) is exactly 0 or 1 in fp32 (exp(104) is inf, exp(-17.4) < 2^-25)
MISTAKES = ("flush_subnormal_operands", "flush_subnormal_results", "pool_16bit_partials", "variance_unshifted", "rounded_before_residual",
            "rounded_before_accumulate", "nan_dropped_by_max", "scale_folded_into_q", "p_narrowed_twice")
Out = namedtuple("Out", "value tol odt k exact sure offset", defaults=(None, 0.0))


def stored_tol(value, t, dt, floor_everywhere=True):
    """t + u (|value| + t) + fl: one rounding to dt of something within t of value (the form of every per-kernel reference)"""
    return t + U[dt] * (value.abs() + t) + (FL[dt] if floor_everywhere else FL[dt] * (value != 0))


def fmax0(t):
    """max(t, 0) the way C's fmaxf does it: a NaN operand is dropped (the seeded mistake nan_dropped_by_max)"""
    return torch.fmax(t, torch.zeros_like(t))


def relu_of(t, mistake):
    return fmax0(t) if mistake == "nan_dropped_by_max" else torch.relu(t)


def _flush_in(t, hdt, mistake):
    return R.flush(t.double(), hdt).to(t.dtype) if mistake == "flush_subnormal_operands" else t


def _flush_out(t, mistake):
    return R.flush(t.double(), t.dtype).to(t.dtype) if mistake == "flush_subnormal_results" and t.dtype != F32 else t


def classes(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    t = t.double()
    return torch.isposinf(t).long() + 2 * torch.isneginf(t).long() + 3 * torch.isnan(t).long()


# ---- HED stage tail ---------------------------------------------------------------------------------------------------------------------------
class hed_tail:
    UNIT = 2.0 ** -6

    @staticmethod
    def base(row, hdt):
        x, w, b = HD.tail_case(hdt, row["B"], *row["size"], row["C"])
        return dict(x=R.quantised(x.float(), hdt, hed_tail.UNIT), w=w, b=b if row["prop"] == "specials" else torch.zeros(1))

    @staticmethod
    def derive(row, P, hdt):
        if row["end"] == "down":
            return (-24 - R.floor_log2(hed_tail.UNIT),)
        if hdt == torch.float16:
            return (R.k_top(float(P["x"].abs().max()), TOP[hdt]),)
        mag = (P["x"].double().clamp_min(0) * P["w"].double()).abs().sum(-1)
        return (R.k_top(float(mag.max()), TOP[hdt]),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        return dict(P, x=P["x"] * 2.0 ** exps[0], k=exps[0])

    @staticmethod
    def outputs(row, P, hdt):
        pooled, so, bd = HD.tail_ref(P["x"].to(hdt), P["w"], P["b"])
        k = P.get("k", 0)
        return {"pool": Out(pooled.double(), torch.zeros_like(pooled, dtype=F64), hdt, k, True), "so": Out(so, bd, F32, k, False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        x = _flush_in(P["x"], hdt, mistake).float()
        r = relu_of(x, mistake)
        so = (r * P["w"]).sum(-1) + P["b"]
        xc = x.permute(0, 3, 1, 2)
        if mistake == "nan_dropped_by_max":          # fmaxf over the window: a NaN is dropped there too
            B, C, H, W = xc.shape
            xp = F.pad(r.permute(0, 3, 1, 2), (0, W % 2, 0, H % 2), value=0.0)
            win = xp.reshape(B, C, (H + 1) // 2, 2, (W + 1) // 2, 2)
            pool = win[:, :, :, 0, :, 0]
            for a, b in ((0, 1), (1, 0), (1, 1)):
                pool = torch.fmax(pool, win[:, :, :, a, :, b])
        else:
            pool = F.relu(F.max_pool2d(xc, 2, 2, ceil_mode=True))
        return {"pool": _flush_out(pool.permute(0, 2, 3, 1).to(hdt), mistake), "so": so}

    @staticmethod
    def specials(row, P, hdt):
        """sample 0: a NaN and a +inf; sample 1: a -inf (relu takes it to 0) and a NaN in a window's second row; sample 2 clean"""
        x = P["x"].clone()
        x[0, 0, 0, 3], x[0, 2, 3, 5], x[1, 4, 4, 9], x[1, 1, 2, 17] = float("nan"), float("inf"), float("-inf"), float("nan")
        return dict(P, x=x)

    @staticmethod
    def torch_eval(row, P, hdt):
        x = P["x"].to(hdt).float()
        pool = F.relu(F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, ceil_mode=True)).permute(0, 2, 3, 1)
        return {"pool": pool, "so": (torch.relu(x) * P["w"]).sum(-1) + P["b"]}

    @staticmethod
    def clean(row, P, name, out):
        m = torch.zeros(out.shape, dtype=torch.bool)
        m[2] = True
        return m


# ---- instance normalisation -----------------------------------------------------------------------------------------------------------------------
class inorm:
    UNIT = 2.0 ** -2

    @staticmethod
    def base(row, hdt):
        """the `offset` family of lineart_ref (means of 50 .. 150 around a spread of 0.5, where a variance formed without the shift
        cancels) on the quantum 1 / 4; shuffled_res: a residual of the plain family"""
        x = R.quantised(LA.inorm_input(hdt, *row["shape"], family="offset").float(), hdt, inorm.UNIT)
        P = dict(x=x, eps=R.eps_scaled(0), relu=int(row.get("relu", row.get("form") == "pad3")), form=row.get("form", "plain"))
        if P["form"] == "shuffled_res":
            P["res"] = torch.randn(row["shape"], generator=torch.Generator().manual_seed(5)).to(hdt).float()
        return P

    @staticmethod
    def shifted(x):
        xd = x.double()
        return xd - xd[:, :1, :1]

    @staticmethod
    def derive(row, P, hdt):
        x = P["x"]
        d = inorm.shifted(x)
        if row["end"] == "up":
            if hdt == torch.float16:
                return (R.k_top(float(x.abs().max()), TOP[hdt]),)
            return (R.k_top(float((d * d).sum((1, 2)).max()), TOP[hdt]) // 2,)
        if hdt == torch.float16:
            return (-24 - R.floor_log2(inorm.UNIT),)
        m = min(R.EPS, float(d[d != 0].abs().min()) ** 2)
        return (math.ceil((-125 - math.log2(m)) / 2),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        return dict(P, x=P["x"] * 2.0 ** exps[0], eps=R.eps_scaled(exps[0]), k=exps[0])

    @staticmethod
    def layout(P, y):
        return LA.reflect_nhwc(y, 3) if P["form"] == "pad3" else y

    @staticmethod
    def outputs(row, P, hdt):
        x = P["x"].to(hdt)
        k = P.get("k", 0)
        m, rstd, _, dm, _, dr = LA.inorm_stats_ref(x, P["eps"])
        _, _, y, t = LA.inorm_ref(x, P["eps"])
        if P["relu"]:
            y = y.clamp_min(0)
        if "res" in P:
            y = y + P["res"].double()
            t = t + E * y.abs()
        B, C = x.shape[0], x.shape[-1]
        return {"mean": Out(m.reshape(B, C), dm.reshape(B, C) + FL[F32], F32, k, False),
                "rstd": Out(rstd.reshape(B, C), dr.reshape(B, C) + FL[F32], F32, -k, False),
                "out": Out(inorm.layout(P, y), inorm.layout(P, stored_tol(y, t, hdt)), hdt, 0, False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        """lineart_ref.inorm_emulate with the eps of the problem (shifted sums in chunks of 512 rows, in order)"""
        x = P["x"].float()
        B, H, W, C = x.shape
        xf = x.reshape(B, H * W, C)
        n = torch.tensor(float(H * W))
        eps = torch.tensor(P["eps"], dtype=F32)
        if mistake == "variance_unshifted":
            mean = xf.sum(1, keepdim=True) / n
            var = ((xf * xf).sum(1, keepdim=True) / n - mean * mean).clamp_min(0)
        else:
            s = xf[:, :1]
            d = xf - s
            s1, s2 = torch.zeros(B, 1, C), torch.zeros(B, 1, C)
            for r0 in range(0, H * W, 512):
                s1 = s1 + d[:, r0:r0 + 512].sum(1, keepdim=True)
                s2 = s2 + (d[:, r0:r0 + 512] ** 2).sum(1, keepdim=True)
            md = s1 / n
            var = s2 / n - md * md
            var = fmax0(var) if mistake == "nan_dropped_by_max" else torch.where(var < 0, torch.zeros_like(var), var)
            mean = s + md
        rstd = 1 / torch.sqrt(var + eps)
        y = ((xf - mean) * rstd).reshape(B, H, W, C)
        if P["relu"]:
            y = relu_of(y, mistake)
        if "res" in P:
            y = y + P["res"]
        return {"mean": mean.reshape(B, C), "rstd": rstd.reshape(B, C), "out": inorm.layout(P, y).to(hdt)}

    @staticmethod
    def specials(row, P, hdt):
        """sample 0: +inf in the plane of channel 3, -inf in channel 5 (first element of the plane), NaN in channel 9; sample 1: +inf and
        -inf in channel 2; the other planes, and all of sample 2, stay clean"""
        x = P["x"].clone()
        x[0, 4, 7, 3], x[0, 0, 0, 5], x[0, 12, 17, 9] = float("inf"), float("-inf"), float("nan")
        x[1, 3, 3, 2], x[1, 9, 1, 2] = float("inf"), float("-inf")
        return dict(P, x=x)

    @staticmethod
    def torch_eval(row, P, hdt):
        y = F.instance_norm(P["x"].to(hdt).float().permute(0, 3, 1, 2), eps=P["eps"]).permute(0, 2, 3, 1)
        return {"out": torch.relu(y) if P["relu"] else y}

    @staticmethod
    def clean(row, P, name, out):
        plane = torch.isfinite(P["x"]).all(1).all(1)                    # [B, C]
        return plane if name in ("mean", "rstd") else plane[:, None, None, :].expand(out.shape)


# ---- the live-channel LayerNorm ------------------------------------------------------------------------------------------------------------------
class ln_live:
    @staticmethod
    def _row(row):
        return dict(row, op="layernorm", end=row.get("end", "up"), seed=row.get("seed", row["shape"]["C"]))

    @staticmethod
    def base(row, hdt):
        x, gamma, beta = R.norm_inputs(ln_live._row(row), hdt)
        return dict(x=x, gamma=gamma, beta=beta, eps=R.eps_scaled(0))

    @staticmethod
    def derive(row, P, hdt):
        return R.norm_exps(ln_live._row(row), P["x"], hdt)

    @staticmethod
    def scaled(row, P, exps, hdt):
        return dict(P, x=P["x"] * 2.0 ** exps[0], eps=R.eps_scaled(exps[0]), k=exps[0])

    @staticmethod
    def outputs(row, P, hdt):
        ref, bound, tiny = N.ln_ref(P["x"], P["gamma"], P["beta"], P["eps"])
        tol = N.k_of(hdt) * U[hdt] * bound + U[hdt] * ref.abs() + tiny + FL[hdt]         # gpu_util.check_bound's tolerance
        pad = row["ld"] - row["shape"]["C"]
        return {"out": Out(F.pad(ref, (0, pad)), F.pad(tol, (0, pad)), hdt, 0, False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        x = P["x"].float()
        mean = x.mean(1, keepdim=True)
        d = x - mean
        rstd = 1 / torch.sqrt((d * d).mean(1, keepdim=True) + torch.tensor(P["eps"], dtype=F32))
        y = d * rstd * P["gamma"].float() + P["beta"].float()
        return {"out": F.pad(y, (0, row["ld"] - row["shape"]["C"])).to(hdt)}

    @staticmethod
    def specials(row, P, hdt):
        x = P["x"].clone()
        x[1, 7], x[5, 0], x[9, 59], x[20, 30], x[20, 31] = float("inf"), float("-inf"), float("nan"), float("inf"), float("-inf")
        return dict(P, x=x)

    @staticmethod
    def torch_eval(row, P, hdt):
        C = row["shape"]["C"]
        y = F.layer_norm(P["x"].to(hdt).float(), (C,), P["gamma"].float(), P["beta"].float(), P["eps"])
        return {"out": F.pad(y, (0, row["ld"] - C))}

    @staticmethod
    def clean(row, P, name, out):
        return torch.isfinite(P["x"]).all(1)[:, None].expand(out.shape)


# ---- channel attention ------------------------------------------------------------------------------------------------------------------------
def _cab(row, hdt, B=None):
    c = HT.CAB_CASES[row["cab"]]
    return HT.cab_case(hdt, *((B,) + c[1:] if B else c))


class chan_pool:
    UNIT = 2.0 ** -6

    @staticmethod
    def base(row, hdt):
        """every live element in [0.75, 1 - 2^-6], one sign per channel, on the quantum 2^-6: scaled to the top, no two of them
        have a sum inside fp16 while the fp32 mean is"""
        L = _cab(row, hdt)
        g = torch.Generator().manual_seed(11 + row["cab"])
        mag = 0.75 + (0.25 - chan_pool.UNIT) * torch.rand(L["c2"].shape, generator=g)
        sign = torch.where(torch.arange(L["ld"]) % 3 == 0, -1.0, 1.0)
        c2 = R.quantised(mag * sign, hdt, chan_pool.UNIT)
        c2[..., L["C"]:] = 0
        return dict(c2=c2, C=L["C"], ld=L["ld"])

    @staticmethod
    def derive(row, P, hdt):
        if hdt == torch.float16:
            return (R.k_top(float(P["c2"].abs().max()), TOP[hdt]),)
        return (R.k_top(float(P["c2"].double().abs().sum(1).max()), TOP[hdt]),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        return dict(P, c2=P["c2"] * 2.0 ** exps[0], k=exps[0])

    @staticmethod
    def outputs(row, P, hdt):
        ref, bd = HT.pool_ref(P["c2"].to(hdt), P["C"])
        return {"pool": Out(ref, bd + FL[F32], F32, P.get("k", 0), False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        x = _flush_in(P["c2"], hdt, mistake).float()[..., :P["C"]]
        acc = torch.zeros(x.shape[0], P["C"])
        for r0 in range(0, x.shape[1], 64):
            part = x[:, r0:r0 + 64].sum(1)
            acc = acc + (part.to(hdt).float() if mistake == "pool_16bit_partials" else part)
        return {"pool": acc / float(x.shape[1])}


class scale_add:
    UNIT = 2.0 ** -6

    @staticmethod
    def base(row, hdt):
        L = _cab(row, hdt)
        C, ld = L["C"], L["ld"]
        if row["prop"] == "sub_out":
            # y = n 2^-6 (|n| <= 100), c2 = m 2^-3 (|m| <= 27), gate 2^-3: y + c2 s = (n + m) 2^-6 with |n + m| <= 127, exact in both
            # storage types; times 2^-18 all three are fp16 subnormals (c2: 8 m 2^-24)
            g = torch.Generator().manual_seed(13 + row["cab"])
            y = torch.randint(-100, 101, L["y"].shape, generator=g).float() * scale_add.UNIT
            c2 = torch.randint(-27, 28, L["c2"].shape, generator=g).float() * 0.125
            s = torch.full((L["B"], ld), 0.125)
        else:
            # the gate the chain itself produces on the base data (at most conv_scale = 0.01), as the fp32 values the gate kernel would store
            y, c2 = R.quantised(L["y"].float(), hdt, scale_add.UNIT), R.quantised(L["c2"].float(), hdt, scale_add.UNIT)
            s = F.pad(HT.gate_ref(*HT.pool_ref(c2.to(hdt), C), L)[0].float(), (0, ld - C))
        y[..., C:], c2[..., C:], s[:, C:] = 0, 0, 0
        return dict(y=y, c2=c2, s=s, C=C, ld=ld)

    @staticmethod
    def value(P):
        return P["y"].double() + P["c2"].double() * P["s"].double().unsqueeze(1)

    @staticmethod
    def derive(row, P, hdt):
        if row["prop"] == "sub_out":
            return (-24 - R.floor_log2(scale_add.UNIT),)
        m = max(float(P["c2"].abs().max()), float(P["y"].abs().max()), float(scale_add.value(P).abs().max()))
        return (R.k_top(m, TOP[hdt]),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        return dict(P, y=P["y"] * 2.0 ** exps[0], c2=P["c2"] * 2.0 ** exps[0], k=exps[0])

    @staticmethod
    def outputs(row, P, hdt):
        v = scale_add.value(P)
        t = E * v.abs()                                     # hat_ref.cab_value64 with an exact gate (ds = 0): one fma
        return {"y": Out(v, stored_tol(v, t, hdt, floor_everywhere=False), hdt, P.get("k", 0), row["prop"] == "sub_out")}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        y, c2 = _flush_in(P["y"], hdt, mistake), _flush_in(P["c2"], hdt, mistake)
        v = (y.double() + c2.double() * P["s"].double().unsqueeze(1)).float()              # one fma: one rounding
        return {"y": _flush_out(v.to(hdt), mistake)}


class cab:
    """pool -> gate -> scale-add, the specials row only"""
    @staticmethod
    def base(row, hdt):
        return _cab(row, hdt, B=3)

    @staticmethod
    def specials(row, P, hdt):
        """sample 0: +inf in channel 3 and -inf in channel 5 (pool +-inf, hidden units +inf / 0 / NaN by the signs of w1); sample 1: a NaN
        in channel 7 (pool NaN -> both hidden units NaN -> every gate NaN); sample 2 clean"""
        c2 = P["c2"].clone()
        c2[0, 17, 3], c2[0, 400, 5], c2[1, 100, 7] = float("inf"), float("-inf"), float("nan")
        return dict(P, c2=c2)

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        C, ld = P["C"], P["ld"]
        c2 = P["c2"].float()
        pool = c2[..., :C].mean(1)
        h = relu_of(pool @ P["w1"].T + P["b1"], mistake)
        s = F.pad(torch.tensor(P["scale"], dtype=F32) * torch.sigmoid(h @ P["w2"].T + P["b2"]), (0, ld - C))
        return {"pool": pool, "gate": s, "y": (P["y"].float() + c2 * s.unsqueeze(1)).to(hdt)}

    @staticmethod
    def torch_eval(row, P, hdt):
        """CABlock's channel attention in torch's own layers: AdaptiveAvgPool2d(1), 1x1 conv, ReLU, 1x1 conv, Sigmoid, the scaled add"""
        C, ld, B = P["C"], P["ld"], P["B"]
        c2 = P["c2"].float()[..., :C].transpose(1, 2).reshape(B, C, P["H"], P["W"])
        pooled = F.adaptive_avg_pool2d(c2, 1)
        hid = F.relu(F.conv2d(pooled, P["w1"][:, :, None, None], P["b1"]))
        att = torch.sigmoid(F.conv2d(hid, P["w2"][:, :, None, None], P["b2"]))
        y = P["y"].float()[..., :C] + (c2 * att * P["scale"]).reshape(B, C, -1).transpose(1, 2)
        return {"pool": pooled.reshape(B, C), "gate": F.pad(att.reshape(B, C) * P["scale"], (0, ld - C)), "y": F.pad(y, (0, ld - C))}

    @staticmethod
    def clean(row, P, name, out):
        m = torch.zeros(out.shape, dtype=torch.bool)
        m[2] = True
        return m


# ---- activations -------------------------------------------------------------------------------------------------------------------------------
def act_inputs(prop, hdt):
    """top: 32 magnitudes from the largest storage value down to half of it, both signs; sub_out: subnormals n 2^-24 (fp16) or n 2^-133
    (bf16) across the whole subnormal range, both signs"""
    fi = torch.finfo(hdt)
    if prop == "top":
        mag = torch.tensor([fi.max * (1 - j / 64) for j in range(32)], dtype=F64)
    else:
        step = fi.smallest_normal * fi.eps
        nmax = round(1 / fi.eps) - 1                       # 1023 / 127
        mag = torch.tensor([round(1 + j * (nmax - 1) / 31) * step for j in range(32)], dtype=F64)
    return torch.cat([mag, -mag]).to(hdt)


class swin_act:
    @staticmethod
    def base(row, hdt):
        if row["prop"] == "specials":
            x = (torch.randn(64, generator=torch.Generator().manual_seed(3)) * 3).to(hdt)
        else:
            x = act_inputs(row["prop"], hdt)
        return dict(x=x.float(), mode=row["mode"], slope=row["slope"])

    @staticmethod
    def derive(row, P, hdt):
        return ()

    @staticmethod
    def outputs(row, P, hdt):
        ref, bd = SW.act_bound(P["x"].to(hdt), P["mode"], P["slope"])
        return {"x": Out(ref, bd, hdt, 0, False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        x = _flush_in(P["x"], hdt, mistake).float()
        if P["mode"] == 0:
            y = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))
        else:
            y = torch.where(x > 0, x, torch.tensor(P["slope"], dtype=F32) * x)
        return {"x": _flush_out(y.to(hdt), mistake)}

    @staticmethod
    def specials(row, P, hdt):
        x = P["x"].clone()
        x[3], x[10], x[20], x[41], x[42] = float("inf"), float("-inf"), float("nan"), float("-inf"), float("inf")
        return dict(P, x=x)

    @staticmethod
    def torch_eval(row, P, hdt):
        x = P["x"].to(hdt)
        if P["mode"] == 0:
            return {"x": F.gelu(x.double())}        # float64: torch's fp32 gelu(+inf) depends on the element count (range_image_cases)
        return {"x": F.leaky_relu(x.float(), P["slope"])}

    @staticmethod
    def clean(row, P, name, out):
        return torch.isfinite(P["x"])


class silu(swin_act):
    @staticmethod
    def base(row, hdt):
        return swin_act.base(dict(row, mode=-1, slope=0.0), hdt)

    @staticmethod
    def outputs(row, P, hdt):
        x = P["x"].to(hdt)
        return {"x": Out(CR.silu_exact(x), CR.silu_bound(x, hdt), hdt, 0, False)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        return {"x": _flush_out(CR.silu_host(_flush_in(P["x"], hdt, mistake).to(hdt)), mistake)}

    @staticmethod
    def torch_eval(row, P, hdt):
        return {"x": F.silu(P["x"].to(hdt).float())}


def act_exact_at_top(P, got, hdt):
    """elements of a `top` row that must be the input itself: f(x) = x in float64-then-rounded terms for the positive inputs (gelu, silu
    and the leaky ReLU are the identity there to far below the last bit) - f(65504) is 65504, not inf"""
    x = P["x"].to(hdt)
    pos = x > 0
    return int((got.to(hdt)[pos] != x[pos]).sum())


# ---- the RRDB epilogue, in place ---------------------------------------------------------------------------------------------------------------
EPI_FORMS = {"block": dict(live=32, c0=64, ldo=192, alpha=0.2, act=1, beta1=1.0, beta2=None),
             "rrdb": dict(live=64, c0=0, ldo=64, alpha=0.04, act=0, beta1=0.2, beta2=1.0)}
EPI_NPIX = 2 * 37 * 5


class rdb_epilogue:
    @staticmethod
    def base(row, hdt):
        f = dict(EPI_FORMS[row["form"]])
        live, ldo = f["live"], f["ldo"]
        g = torch.Generator().manual_seed(live + ldo)
        if row["prop"] == "epi_back":
            # lattice: acc = L in [256, 511], bias 768, alpha 1: step 1 = L + 768 >= 1024; the residuals (storage values themselves:
            # -384 and -256, beta1 = 2) take the 768 back in one step (block) or two (rrdb: -512, then -256)
            buf = torch.randint(256, 512, (EPI_NPIX, ldo), generator=g).float()
            f.update(alpha=1.0, beta1=2.0, beta2=None if f["beta2"] is None else 1.0)
            bias = torch.full((live,), 768.0)
            r1 = torch.full((EPI_NPIX, live), -384.0 if f["beta2"] is None else -256.0)
            r2 = None if f["beta2"] is None else torch.full((EPI_NPIX, live), -256.0)
        else:
            buf = torch.randn((EPI_NPIX, ldo), generator=g).to(hdt).float()
            r1 = torch.randn((EPI_NPIX, live), generator=g).to(hdt).float()
            r2 = None if f["beta2"] is None else torch.randn((EPI_NPIX, live), generator=g).to(hdt).float()
            bias = torch.randn(live, generator=g)
        return dict(f, buf=buf, r1=r1, r2=r2, bias=bias)

    @staticmethod
    def value(P):
        """(float64 value of the slice, G: the magnitude the epilogue's roundings are relative to - rrdb_ref.value64 with acc = the stored value)"""
        al, b1, b2 = RB.f32(P["alpha"]), RB.f32(P["beta1"]), RB.f32(P["beta2"] or 0.0)
        acc = P["buf"][:, P["c0"]:P["c0"] + P["live"]].double()
        bias = P["bias"].double()
        v = al * (acc + bias)
        if P["act"]:
            v = torch.where(v > 0, v, RB.f32(0.2) * v)
        G = abs(al) * (acc.abs() + bias.abs())
        for r, b in ((P["r1"], b1), (P["r2"], b2)):
            if r is not None:
                v = v + b * r.double()
                G = G + (b * r.double()).abs()
        return v, G

    @staticmethod
    def derive(row, P, hdt):
        v, G = rdb_epilogue.value(P)
        if hdt == torch.bfloat16:
            return (R.k_top(float(G.max()), TOP[hdt]),)
        m = max(float(t.abs().max()) for t in (P["buf"], P["r1"], P["r2"], v) if t is not None)
        if row["prop"] == "epi_back":
            m = float(v.abs().max())                       # the operands of the lattice are below the outputs' top by construction (asserted)
        return (R.k_top(m, TOP[hdt]),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        f = 2.0 ** exps[0]
        return dict(P, buf=P["buf"] * f, r1=P["r1"] * f, r2=None if P["r2"] is None else P["r2"] * f, bias=P["bias"] * f, k=exps[0])

    @staticmethod
    def outputs(row, P, hdt):
        v, G = rdb_epilogue.value(P)
        t = 8 * E * G + 2.0 ** -146                         # rrdb_ref.bound without the accumulation term
        return {"slice": Out(v, stored_tol(v, t, hdt), hdt, P.get("k", 0), row["prop"] == "epi_back")}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        s = slice(P["c0"], P["c0"] + P["live"])
        r1, r2 = P["r1"].to(hdt), None if P["r2"] is None else P["r2"].to(hdt)
        v = RB.steps32(P["buf"][:, s].to(hdt).float(), P["bias"], P["alpha"], P["act"], r1, P["beta1"], r2, P["beta2"] or 0.0,
                       "rounded_before_residual" if mistake == "rounded_before_residual" else None)
        return {"slice": v.to(hdt)}

    @staticmethod
    def specials(row, P, hdt):
        buf, r1 = P["buf"].clone(), P["r1"].clone()
        c0 = P["c0"]
        buf[3, c0 + 1], buf[5, c0 + 2], buf[7, c0 + 3], buf[9, c0 + 4] = float("inf"), float("-inf"), float("nan"), float("inf")
        r1[9, 4], r1[11, 5] = float("-inf"), float("nan")                  # inf + (-inf); a NaN residual on a finite accumulator
        return dict(P, buf=buf, r1=r1)

    @staticmethod
    def torch_eval(row, P, hdt):
        """the epilogue as the RRDB graph writes it: leaky_relu(alpha (acc + bias), 0.2) + beta1 r1 + beta2 r2"""
        v = P["alpha"] * (P["buf"][:, P["c0"]:P["c0"] + P["live"]].to(hdt).float() + P["bias"])
        if P["act"]:
            v = F.leaky_relu(v, 0.2)
        v = v + P["beta1"] * P["r1"].to(hdt).float()
        return {"slice": v if P["r2"] is None else v + P["beta2"] * P["r2"].to(hdt).float()}

    @staticmethod
    def clean(row, P, name, out):
        s = slice(P["c0"], P["c0"] + P["live"])
        m = torch.isfinite(P["buf"][:, s]) & torch.isfinite(P["r1"])
        return m if P["r2"] is None else m & torch.isfinite(P["r2"])


# ---- sigmoid outputs ----------------------------------------------------------------------------------------------------------------------------
def sure_sign(logit, t):
    """the elements whose fp32 logit has the sign of the float64 one whatever the summation order: |logit| > 2 t, t the bound of its
    fp32 evaluation.  The kernel's scaled logit is 2^k times ITS base logit, so only these are known to saturate."""
    return logit.abs() > 2 * t


def k_saturate(logit, t):
    """the smallest k with min |logit| 2^k >= SAT over the sure elements: the scaled minimum lies in [SAT, 2 SAT)"""
    return math.ceil(math.log2(SAT / float(logit[sure_sign(logit, t)].abs().min())))


def saturated(sign, sure, odt):
    v = sign.double()
    return Out(v, (~sure).double(), odt, None, True, sure)


class hed_fuse:
    @staticmethod
    def base(row, hdt):
        so, wf, bf = HD.fuse_case(row["geometry"])
        return dict(so=so, wf=wf, bf=bf, H=HD.MODEL_CASES[row["geometry"]][0], W=HD.MODEL_CASES[row["geometry"]][1])

    @staticmethod
    def logits(P):
        """(the six float64 logit maps [6, B, 1, H, W], the bound of their fp32 evaluation) from hed_ref.fuse_ref: its t is the bound
        after the sigmoid, t_logit / 4 + 4 E"""
        ref, t = HD.fuse_ref(P["so"], P["wf"], P["bf"], P["H"], P["W"])
        return torch.logit(ref), 4 * (t - 4 * E)

    @staticmethod
    def derive(row, P, hdt):
        return (k_saturate(*hed_fuse.logits(P)),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        f = 2.0 ** exps[0]
        l, t = hed_fuse.logits(P)
        return dict(P, so=[s * f for s in P["so"]], bf=P["bf"] * f, k=exps[0], sign=l > 0, sure=sure_sign(l, t))

    @staticmethod
    def outputs(row, P, hdt):
        odt = DT[row.get("out", "f32")]
        if "sign" in P:                                    # saturated: exactly 1 or 0, whatever the output type
            return {"out": saturated(P["sign"], P["sure"], odt)}
        ref, t = HD.fuse_ref(P["so"], P["wf"], P["bf"], P["H"], P["W"])
        return {"out": Out(ref, HD.stored_bound(ref, t, odt), odt, None, False)}

    @staticmethod
    def eval32(P):
        """hed_ref.fuse_ref's evaluation in fp32 torch calls: the six sigmoided maps"""
        H, W = P["H"], P["W"]
        oy, ox = HD.crop_offsets(H), HD.crop_offsets(W)
        ls = []
        for k in range(5):
            s = P["so"][k].float()[:, None]
            up = F.conv_transpose2d(s, HD.bilinear(2 ** k, F32), stride=2 ** k) if k else s
            ls.append(up[:, :, oy[k]:oy[k] + H, ox[k]:ox[k] + W])
        fuse = P["bf"].float() + sum(P["wf"][k].float() * ls[k] for k in range(5))
        return torch.sigmoid(torch.stack(ls + [fuse]))

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        return {"out": hed_fuse.eval32(P).to(DT[row.get("out", "f32")])}

    @staticmethod
    def specials(row, P, hdt):
        """sample 0: +inf in map 1 inside the crop, NaN in map 3, -inf in map 5 (whose one pixel spreads over 32 x 32 output pixels);
        sample 1 clean"""
        so = [s.clone() for s in P["so"]]
        so[0][0, 36, 37], so[2][0, 9, 10], so[4][0, 2, 2] = float("inf"), float("nan"), float("-inf")
        return dict(P, so=so)

    @staticmethod
    def torch_eval(row, P, hdt):
        return {"out": hed_fuse.eval32(P)}

    @staticmethod
    def clean(row, P, name, out):
        m = torch.zeros(out.shape, dtype=torch.bool)
        m[:, 1] = True
        return m


class conv7_out:
    @staticmethod
    def base(row, hdt):
        xp, w, b = LA.conv7_out_case(hdt, *row["shape"])
        if row["prop"] == "saturate":                      # logits around 1.5 +- 1: both signs occur, and few lie near zero
            b = torch.full((1,), 1.5)
        return dict(xp=xp.float(), w=w.float(), b=b, sigmoid=int(row["prop"] != "top"))

    @staticmethod
    def derive(row, P, hdt):
        ref, t = LA.conv7_out_ref(P["xp"], P["w"], P["b"], 0)
        k = R.k_top(float(ref.abs().max()), TOP[torch.float16]) if row["prop"] == "top" else k_saturate(ref, t)
        return (k // 2, k - k // 2)

    @staticmethod
    def scaled(row, P, exps, hdt):
        ka, kw = exps
        P1 = dict(P, xp=P["xp"] * 2.0 ** ka, w=P["w"] * 2.0 ** kw, b=P["b"] * 2.0 ** (ka + kw), k=ka + kw)
        if row["prop"] == "saturate":
            l, t = LA.conv7_out_ref(P["xp"], P["w"], P["b"], 0)
            P1["sign"], P1["sure"] = l > 0, sure_sign(l, t)
        return P1

    @staticmethod
    def outputs(row, P, hdt):
        odt = DT[row.get("out", "f32")]
        if "sign" in P:
            return {"out": saturated(P["sign"], P["sure"], odt)}
        ref, t = LA.conv7_out_ref(P["xp"], P["w"], P["b"], P["sigmoid"])
        return {"out": Out(ref, LA.stored_bound(ref, t, odt), odt, P.get("k", 0) if row["prop"] == "top" else None, False)}

    @staticmethod
    def eval32(P):
        """the 49 x 64 products of every output pixel formed one by one and summed (no library convolution: a zero-weight or
        transformed-domain product of an inf would be a NaN the kernel does not form), bias, sigmoid"""
        x = P["xp"].float().permute(0, 3, 1, 2)
        B, _, Hp, Wp = x.shape
        cols = F.unfold(x, 7)                                             # [B, 64 * 49, L]
        v = (cols * P["w"].float().reshape(1, -1, 1)).sum(1).reshape(B, 1, Hp - 6, Wp - 6) + P["b"].float()
        return torch.sigmoid(v) if P["sigmoid"] else v

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        return {"out": conv7_out.eval32(P).to(DT[row.get("out", "f32")])}

    @staticmethod
    def specials(row, P, hdt):
        """sample 0 of the 15 x 24 padded image: +inf under the outputs of columns 0 .. 2, NaN under columns 5 .. 11, -inf under columns
        15 .. 17; sample 1 clean"""
        xp = P["xp"].clone()
        xp[0, 7, 2, 5], xp[0, 7, 11, 40], xp[0, 7, 21, 63] = float("inf"), float("nan"), float("-inf")
        return dict(P, xp=xp)

    @staticmethod
    def torch_eval(row, P, hdt):
        return {"out": conv7_out.eval32(dict(P, xp=P["xp"].to(hdt), w=P["w"].to(hdt)))}

    @staticmethod
    def clean(row, P, name, out):
        m = torch.zeros(out.shape, dtype=torch.bool)
        m[1] = True
        return m


# ---- boundary kernels: bit-equal to torch's cast --------------------------------------------------------------------------------------------------
def cast_problem(row, hdt):
    """(inputs, expected stored output) of a `cast` row: range_ref.cast_image in the row's source dtype (the kernels whose input is a
    storage tensor take it in the storage type and the row's dtype is the OUTPUT's), the expectation from torch's own casts"""
    op, src = row["op"], row.get("src")
    sn = NAME[hdt]
    if op == "pixel_unshuffle":
        x = R.cast_image(src, (2, 3, 8, 12), seed=row["r"])
        return dict(x=x), RB.unshuffle(x, row["r"], hdt)
    if op == "tconv_compose":
        w = R.cast_image(src, (5, 3, 3, 3), seed=1)                      # [Cin, Cout, 3, 3]
        return dict(w=w), LA.compose_tconv(w.float().to(hdt))
    if op == "swin_entry":
        x = R.cast_image(src, (2, 3, 37), seed=2)
        want = torch.zeros((2, 37, 8), dtype=hdt)
        want[..., :3] = ((x.float() - 0.0) * 1.0).to(hdt).transpose(1, 2)
        return dict(x=x), want
    if op == "swin_exit":
        x = torch.randn((2, 37, 8), generator=torch.Generator().manual_seed(3)).to(hdt)
        x[..., :3] = R.cast_image(sn, (2, 37, 3), seed=3)                # (the kernel reads channels 0 .. 2 of a stride of 8)
        return dict(x=x), (x[..., :3].float() / 1.0 + 0.0).transpose(1, 2).contiguous().to(DT[src])
    if op == "hed_entry":
        x = R.cast_image(src, (2, 3, 5, 7), seed=4)
        want = torch.zeros((2, 5 + 68, 7 + 68, 8), dtype=hdt)
        want[:, 34:39, 34:41, :3] = x.float().to(hdt).permute(0, 2, 3, 1)
        return dict(x=x), want
    if op == "ctrl_emit":
        f = R.cast_image(sn, (2, 35, 24), seed=5)
        out = torch.full((4, 20, 35), float("nan"), dtype=DT[src])
        return dict(f=f, C=20, scale=1.0, accumulate=0, out=out, b0=2), CR.emit_host(f, 20, 1.0, False, out, 2)
    assert op == "ctrl_emit_acc"
    P = ctrl_emit_acc.base(row, hdt)
    return P, ctrl_emit_acc.emulate(row, P, hdt)["out"]


class ctrl_emit_acc:
    @staticmethod
    def base(row, hdt):
        """res_order: f = 32768 + 64 n, scale 2: every product is beyond 65504; out = -49152: the sums 16384 + 128 n are inside fp16.
        specials: randn with +-inf and NaN in both operands"""
        g = torch.Generator().manual_seed(17)
        B, HW, Cpad, C = 2, 35, 24, 20
        if row["prop"] == "res_order":
            f = (32768.0 + 64.0 * torch.randint(0, 256, (B, HW, Cpad), generator=g).float()).to(hdt)
            out = torch.full((B + 2, C, HW), -49152.0, dtype=hdt)
            return dict(f=f, C=C, scale=2.0, accumulate=1, out=out, b0=1)
        f = torch.randn((B, HW, Cpad), generator=g).to(hdt)
        out = torch.randn((B + 2, C, HW), generator=g).to(hdt)
        return dict(f=f, C=C, scale=-1.7, accumulate=1, out=out, b0=1)

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        return {"out": CR.emit_host(P["f"], P["C"], P["scale"], bool(P["accumulate"]), P["out"], P["b0"],
                                    "rounded_before_accumulate" if mistake == "rounded_before_accumulate" else None)}

    @staticmethod
    def specials(row, P, hdt):
        f, out = P["f"].clone(), P["out"].clone()
        f[0, 3, 1], f[0, 4, 2], f[0, 5, 3], f[0, 6, 4] = float("inf"), float("-inf"), float("nan"), float("inf")
        out[1, 4, 6], out[1, 7, 7] = float("inf"), float("nan")             # scale < 0: -inf + inf at [1][4][6]
        return dict(P, f=f, out=out)

    @staticmethod
    def torch_eval(row, P, hdt):
        """out[b0 + b] += scale * f[b] as torch.add with alpha, NCHW from NHWC"""
        out = P["out"].float().clone()
        b0, B = P["b0"], P["f"].shape[0]
        out[b0:b0 + B] = torch.add(out[b0:b0 + B], P["f"].float()[:, :, :P["C"]].permute(0, 2, 1), alpha=P["scale"])
        return {"out": out}

    @staticmethod
    def clean(row, P, name, out):
        m = torch.isfinite(P["out"])
        b0, B = P["b0"], P["f"].shape[0]
        m[b0:b0 + B] &= torch.isfinite(P["f"][:, :, :P["C"]].transpose(1, 2))
        return m


# ---- window attention: SwinIR 8 x 8 (win_attn) and HAT 16 x 16 / overlapping (hat_attn) -----------------------------------------------------------
ATTN_UNIT = 2.0 ** -6
LOGIT_LIMIT = 15                         # q, k = n 2^-6 with |n| <= 15: times 2^-18 they are fp16 subnormals n 2^-24, times 2^18 at most 61440


def _attn_ref(row):
    return SW if row["op"] == "win_attn" else HT


def _attn_case(row, hdt):
    return SW.case(hdt, *row["case"]) if row["op"] == "win_attn" else HT.case(hdt, *row["case"])


def _attn_operands(row, L, dt):
    """(q, k, v, bias, mask or None, unwindow) of a call as its reference computes them"""
    if row["op"] == "hat_attn":
        qq, kk, vv, bias, mask = HT._operands(L, dt)
        s = L["shift"] if L["mode"] == "sa" else 0
        return qq, kk, vv, bias, mask, (lambda ow: HT._unwindow(L, ow, s))
    qq, kk, vv = SW._windows(L, dt)
    return qq, kk, vv, SW.expanded_bias(L["table"].to(dt)).unsqueeze(0), SW._mask(L, dt), (lambda ow: SW._unwindow(L, ow))


def _qkv_view(L):
    """[rows, 3 (q, k, v), heads, 32] view of the live part of qkv (float32 copy)"""
    nh = L["heads"]
    return L["qkv"][:, :96 * nh].float().reshape(-1, 3, nh, 32)


def _with_qkv(L, t):
    nh = L["heads"]
    t = t.clone()
    t[..., 30:] = 0
    qkv = L["qkv"].clone()
    qkv[:, :96 * nh] = t.reshape(-1, 96 * nh).to(qkv.dtype)
    return dict(L, qkv=qkv)


class win_attn:
    @staticmethod
    def base(row, hdt):
        L = _attn_case(row, hdt)
        t = _qkv_view(L)
        nh = L["heads"]
        if row["prop"] == "logit_shift":
            t[:, :2] = R.quantised(t[:, :2] * 0.1, hdt, ATTN_UNIT, LOGIT_LIMIT)
        elif row["end"] == "up":
            # V = +-(1.5 + randn / 4), one sign per channel: every output, a convex combination, is away from zero (range_ref.attn_inputs)
            sign = torch.where(torch.arange(nh * 32) % 3 == 0, -1.0, 1.0).reshape(nh, 32)
            t[:, 2] = R.quantised((1.5 + 0.25 * t[:, 2]) * sign, hdt, ATTN_UNIT)
            if row.get("peaked"):
                # logits nine times as wide: one or two keys carry a row's softmax, so the output's error IS the rounding of their P -
                # a P narrowed through the other 16-bit type (bf16: 2^-9 of a p in [1/2, 1)) is four times what the bound allows it
                t[:, :2] = R.quantised(t[:, :2] * 3.0, hdt, ATTN_UNIT)
        else:
            # q = 0 and a zero table: the softmax is uniform over a window (over a region of a shifted one: 16 .. 256 keys, powers of
            # two); V = n keys / 64 with n in {-1, 0, 1} and keys the window's 64 or 256: times 2^-18 V and every output,
            # sum(n) keys / (64 size), are fp16 subnormals on the lattice
            g = torch.Generator().manual_seed(29)
            t[:, 0] = 0
            t[:, 2] = torch.randint(-1, 2, t[:, 2].shape, generator=g).float() * (1.0 if row["op"] == "win_attn" else 4.0)
            L = dict(L, table=torch.zeros_like(L["table"]))
        return dict(L=_with_qkv(L, t))

    @staticmethod
    def derive(row, P, hdt):
        t = _qkv_view(P["L"])
        if row["prop"] == "logit_shift":                   # the same numbers on both flavours: the operand that goes up reaches fp16's top
            return (R.k_top(float(t[:, 0 if row["dir"] == "q_up" else 1].abs().max()), TOP[torch.float16]),)
        if row["end"] == "down":
            # V is a multiple of keys / 64 and the largest uniform softmax runs over `keys` of them: the outputs are multiples of 1 / 64
            vq = float(t[:, 2][t[:, 2] != 0].abs().min())
            keys = 64 if row["op"] == "win_attn" else 256
            return (-24 - R.floor_log2(vq / keys),)
        return (R.k_top(float(t[:, 2].abs().max()), TOP[hdt]),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        t = _qkv_view(P["L"])
        k = exps[0]
        if row["prop"] == "logit_shift":
            up, down = (0, 1) if row["dir"] == "q_up" else (1, 0)
            t[:, up], t[:, down] = t[:, up] * 2.0 ** k, t[:, down] * 2.0 ** -k
            return dict(L=_with_qkv(P["L"], t), k=0)
        t[:, 2] = t[:, 2] * 2.0 ** k
        return dict(L=_with_qkv(P["L"], t), k=k)

    @staticmethod
    def lattice(row):
        """the down row is exact where every softmax is uniform over a power of two of keys: not the overlapping form, whose 576 keys give 1 / 576"""
        return row["prop"] == "convex" and row["end"] == "down" and not (row["op"] == "hat_attn" and row["case"][0] == "oca")

    @staticmethod
    def outputs(row, P, hdt):
        v, bd = _attn_ref(row).bound(P["L"])
        k = P.get("k", 0)
        if row["prop"] == "convex" and row["end"] == "down" and not win_attn.lattice(row):
            k = None                                       # every output is subnormal: rounding is absolute there, check 2 with its floor decides
        return {"o": Out(v, bd, hdt, k, win_attn.lattice(row))}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        L = P["L"]
        f = F32
        qq, kk, vv, bias, mask, unwindow = _attn_operands(row, L, f)
        if mistake == "flush_subnormal_operands":
            qq, kk, vv = (R.flush(t.double(), hdt).float() for t in (qq, kk, vv))
        c = torch.tensor(SW.SCALE, dtype=f)
        if mistake == "scale_folded_into_q":
            l = (qq * c).to(hdt).float() @ kk.transpose(-2, -1) + bias
        else:
            l = c * (qq @ kk.transpose(-2, -1)) + bias
        if mask is not None:
            l = l + mask
        p = torch.softmax(l, dim=-1)
        if mistake == "p_narrowed_twice":                  # through the other 16-bit type first, then to storage
            p = p.to(torch.bfloat16 if hdt == torch.float16 else torch.float16).float()
        p = p.to(hdt).float()
        o = (p @ vv).to(hdt)
        return {"o": _flush_out(unwindow(o.float()).to(hdt), mistake)}


class hat_attn(win_attn):
    pass


# ---- the dense-block convolution of the RRDBNet (MFMA, narrow N) with its epilogue -----------------------------------------------------------
# three cases of tests/test_gpu_rdb_kernels.CASES: (Cin, NT, live, ldo, c0, form, ups)
RDB_CASES = {"plain": (64, 32, 32, 192, 64, "plain", 0), "rrdb": (192, 64, 64, 192, 0, "rrdb", 0), "act-ups1": (64, 64, 64, 64, 0, "act", 1)}
EPI_BACK = dict(bias=147456.0, r1=-32768.0, r2=-32768.0, final=49152.0)      # bias + 2 r1 + r2 = final (the lattice rrdb form: beta1 2, beta2 1)


def rdb_image():
    """(th + 1, 2 tw + 1) of the kernel's output tile: a second tile row, a third tile column with one live pixel"""
    import ctypes as C
    from gyre_amd import _lib
    th, tw = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib(_lib.BF16).gyre_op_rdb_tile(C.byref(th), C.byref(tw)))
    return th.value + 1, 2 * tw.value + 1


class rdb_conv:
    @staticmethod
    def base(row, hdt):
        Cin, NT, live, ldo, c0, form, ups = RDB_CASES[row["case"]]
        H, W = rdb_image()
        L = RB.launch(hdt, 2, H, W, Cin, NT, live, 192, ldo, c0, form=form, ups=ups, lattice=row["prop"] != "top")
        if row["prop"] == "cancel":                          # the two channels the scaled problem injects into
            L["x"][..., 0], L["x"][..., Cin - 1] = 0, 0
        return dict(L=L)

    @staticmethod
    def derive(row, P, hdt):
        L, prop = P["L"], row["prop"]
        v, A, G = RB.value64(L)
        xmax, wmax = float(L["x"][..., :L["Cin"]].abs().max()), float(L["w"].abs().max())
        # the lattice is the integers: its quantum, the smallest non-zero magnitude, times 2^k is 2^-24
        down = lambda t: -24 - R.floor_log2(float(t[(t != 0) & ~torch.isnan(t)].abs().min()))
        if prop == "sub_act":
            return (down(L["x"][..., :L["Cin"]].float()), R.k_top(wmax, TOP[torch.float16]))
        if prop == "sub_w":
            return (R.k_top(xmax, TOP[torch.float16]), down(L["w"].float()))
        if prop == "sub_out":
            k = down(RB._sum(L, F64))
            return (k // 2, k - k // 2)
        if prop == "epi_back":
            k = R.k_top(float(v.abs().max()), TOP[hdt] - EPI_BACK["final"])
        elif hdt == torch.bfloat16:
            k = R.k_top(max(float(G.max()), abs(L["alpha"]) * float(A.max())), TOP[hdt])
        else:
            k = R.k_top(max(float(t.abs().max()) for t in (v, L["r1"], L["r2"]) if t is not None), TOP[hdt])
        return (k // 2, k - k // 2)

    @staticmethod
    def scaled(row, P, exps, hdt):
        L0, (ka, kw) = P["L"], exps
        k = ka + kw
        L = dict(L0, x=(L0["x"].float() * 2.0 ** ka).to(hdt), w=(L0["w"].float() * 2.0 ** kw).to(hdt), bias=L0["bias"] * 2.0 ** k)
        for n in ("r1", "r2"):
            if L0[n] is not None:
                L[n] = (L0[n].float() * 2.0 ** k).to(hdt)
        if row["prop"] == "cancel":
            # channel 0, walked first, adds 512 * 64 = 2^15 per valid tap (at least four: 2^17), the last channel takes every one back
            Cin, live = L["Cin"], L["live"]
            L["x"][..., 0], L["x"][..., Cin - 1] = 512.0, 512.0
            L["w"][:live, :, :, 0], L["w"][:live, :, :, Cin - 1] = 64.0, -64.0
        if row["prop"] == "epi_back":
            L["bias"] = L["bias"] + EPI_BACK["bias"]
            L["r1"], L["r2"] = (L["r1"].float() + EPI_BACK["r1"]).to(hdt), (L["r2"].float() + EPI_BACK["r2"]).to(hdt)
        return dict(L=L, k=k)

    @staticmethod
    def outputs(row, P, hdt):
        L, prop = P["L"], row["prop"]
        v, bd = RB.bound(L)
        lattice = prop != "top"
        k = P.get("k", 0)
        if prop == "sub_out" and L["act"]:
            k = None                # 0.2f n 2^-24 is rounded absolutely in the subnormals: one rounding of the exact value, no base run to compare
        value = RB.lattice_expected(L).double() if lattice else v
        return {"slice": Out(value, bd, hdt, k, lattice, None, EPI_BACK["final"] if prop == "epi_back" and "k" in P else 0.0)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        L = P["L"]
        if mistake == "flush_subnormal_operands":
            L = dict(L, x=R.flush(L["x"].double(), hdt).to(hdt), w=R.flush(L["w"].double(), hdt).to(hdt))
        out = RB.emulate(L, "rounded_before_residual" if mistake == "rounded_before_residual" else None)
        return {"slice": _flush_out(out[..., L["c0"]:L["c0"] + L["live"]].contiguous(), mistake)}


# ---- the line-art hinter's first 7 x 7 convolution (MFMA, reflection inside the gather) ------------------------------------------------------
class conv7_in:
    UNIT = 2.0 ** -4

    @staticmethod
    def base(row, hdt):
        """top: lineart_ref.conv7_in_case.  sub_act / sub_w: x = n / 16 (0 .. 15), w = m / 16 (|m| <= 15), bias a multiple of 1 / 4: every
        product is an integer over 256 and every partial sum exact in fp32, so a subnormal operand must give the exact value"""
        B, H, W = row["shape"]
        x, w, b = LA.conv7_in_case(hdt, B, H, W)
        if row["prop"] != "top":
            g = torch.Generator().manual_seed(41)
            x = torch.randint(0, 16, x.shape, generator=g).float() * conv7_in.UNIT
            w = torch.randint(-15, 16, w.shape, generator=g).float() * conv7_in.UNIT
            b = torch.randint(-8, 9, b.shape, generator=g).float() * 0.25
        return dict(x=x.float(), w=w.float(), b=b)

    @staticmethod
    def derive(row, P, hdt):
        down = -24 - R.floor_log2(conv7_in.UNIT)
        if row["prop"] == "sub_act":
            return (down, R.k_top(float(P["w"].abs().max()), TOP[torch.float16]))
        if row["prop"] == "sub_w":
            return (R.k_top(float(P["x"].abs().max()), TOP[torch.float16]), down)
        ref, t = LA.conv7_in_ref(P["x"], P["w"], P["b"])
        k = R.k_top(float(ref.abs().max()), TOP[hdt]) if hdt == torch.float16 else R.k_top(float(t.max()) / ((49 * 8 + 2) * E), TOP[hdt])
        return (k // 2, k - k // 2)

    @staticmethod
    def scaled(row, P, exps, hdt):
        ka, kw = exps
        return dict(x=P["x"] * 2.0 ** ka, w=P["w"] * 2.0 ** kw, b=P["b"] * 2.0 ** (ka + kw), k=ka + kw)

    @staticmethod
    def outputs(row, P, hdt):
        ref, t = LA.conv7_in_ref(P["x"], P["w"], P["b"])
        return {"out": Out(ref, LA.stored_bound(ref, t, hdt), hdt, P.get("k", 0), row["prop"] != "top")}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        x, w = _flush_in(P["x"], hdt, mistake), _flush_in(P["w"], hdt, mistake)
        y = F.conv2d(F.pad(x.double(), (3,) * 4, "reflect"), w.double(), P["b"].double()).float()      # fp32 of the exact sum (lattice rows: exact)
        return {"out": y.permute(0, 2, 3, 1).to(hdt)}


# ---- the plain-matrix delta merge (k_merge_delta): lattice data, base and every term's scale times 2^k -----------------------------------------
class merge_delta:
    @staticmethod
    def base(row, hdt):
        import merge_delta_ref as MD
        base, terms = MD.case_terms(MD.CASES[MD.IDS.index(row["case"])])
        return dict(base=base, terms=terms)

    @staticmethod
    def derive(row, P, hdt):
        """up: an fp16 output - the largest merged weight into (top / 2, top]; fp32 / bf16 outputs - the fp32 accumulator: the largest
        merged weight times 2^8 (the margin range_ref.lora_exps gives the LyCORIS forms, whose absolute sum is not exposed) <= 2^126.
        down: the smallest k that leaves every merged weight an integer times 2^-24 (fp16 subnormals)"""
        import numpy as np
        import merge_delta_ref as MD
        ref = MD.ref64(P["base"], P["terms"])
        if row["end"] == "down":
            k = -24
            while not np.array_equal(ref * 2.0 ** (k + 24), np.round(ref * 2.0 ** (k + 24))):
                k += 1
            return (k,)
        m = float(np.abs(ref).max())
        return (R.k_top(m, TOP[torch.float16]) if row["out"] == "f16" else R.k_top(m * 256.0, 2.0 ** 126),)

    @staticmethod
    def scaled(row, P, exps, hdt):
        import numpy as np
        k = exps[0]
        return dict(base=P["base"] * np.float32(2.0 ** k), terms=[(fields, user * 2.0 ** k) for fields, user in P["terms"]], k=k)

    @staticmethod
    def outputs(row, P, hdt):
        import merge_delta_ref as MD
        odt = DT[row["out"]]
        ref = torch.from_numpy(MD.ref64(P["base"], P["terms"]).copy())
        return {"out": Out(ref, torch.from_numpy(MD.bound(P["base"], P["terms"], odt).copy()) + FL[odt], odt, P.get("k", 0), True)}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        import merge_delta_ref as MD
        return {"out": _flush_out(MD.emulate(P["base"], P["terms"], DT[row["out"]]), mistake)}


# ---- the four-parity upsampler convolution (GemmParams::ups4, launch_compose_ups4, config 24) -----------------------------------------------
UPS4_ALL = 1 << 30                       # tuning bit 30 of gyre_debug_gemm_ablation: the form on config 24 whatever the tile count


class ups4:
    @staticmethod
    def shape(row):
        """(B, Hi, Wi, Cin, N): the smallest problem gyre_debug_ups4_plan accepts - one source pixel, one 64-channel chunk, 8 outputs; at
        a 1 x 1 image the one live 2 x 2 tap of every parity is a sum of FOUR nine-tap weights.  cancel needs a second chunk."""
        return (1, 1, 1, 128 if row["prop"] == "cancel" else 64, 8)

    @staticmethod
    def base(row, hdt):
        import math
        B, Hi, Wi, Cin, N = ups4.shape(row)
        g = torch.Generator().manual_seed(53)
        if row["prop"] == "top":
            x = torch.randn(B, Hi, Wi, Cin, generator=g).to(hdt).double()
            w = (torch.randn(N, 3, 3, Cin, generator=g) / math.sqrt(9 * Cin)).to(hdt).double()
            bias = torch.randn(N, generator=g).float().double()
        else:                                                # the exact lattice of tests/test_gpu_ups4_conv.py
            x = torch.randint(-2, 3, (B, Hi, Wi, Cin), generator=g).double()
            w = torch.randint(-4, 5, (N, 3, 3, Cin), generator=g).double()
            bias = torch.randint(-8, 9, (N,), generator=g).double()
        if row["prop"] == "cancel":
            x[..., 0], x[..., Cin - 1] = 0, 0
        return dict(x=x, w=w, bias=bias)

    @staticmethod
    def reference(P):
        """(float64 nine-tap value [M, N], absolute-value form) of the stored operands: gemm_ref.conv_gather / reference"""
        import gemm_ref as G
        A = G.conv_gather(P["x"], ups=1)
        M, _, Cc = A.shape
        return G.reference(A.reshape(M, 9 * Cc), P["w"].reshape(P["w"].shape[0], 9 * Cc), bias=P["bias"])

    @staticmethod
    def derive(row, P, hdt):
        import ups4_ref as U4
        prop = row["prop"]
        v, b = ups4.reference(P)
        wc = U4.compose(P["w"])
        down = lambda t: -24 - R.floor_log2(float(t[t != 0].abs().min()))
        if prop == "sub_act":                                # the composed weights, sums of up to four taps, must stay storage values
            return (down(P["x"]), R.k_top(float(wc.abs().max()), TOP[torch.float16]))
        if prop == "sub_w":
            return (R.k_top(float(P["x"].abs().max()), TOP[torch.float16]), down(P["w"]))
        k = R.k_top(float(v.abs().max()), TOP[hdt]) if hdt == torch.float16 else R.k_top(float(b.max()), TOP[hdt])
        return (k // 2, k - k // 2)

    @staticmethod
    def scaled(row, P, exps, hdt):
        ka, kw = exps
        P1 = dict(x=P["x"] * 2.0 ** ka, w=P["w"] * 2.0 ** kw, bias=P["bias"] * 2.0 ** (ka + kw), k=ka + kw)
        if row["prop"] == "cancel":
            # channel 0, in the first chunk, adds 512 * 64 = 2^15 per nine-tap weight (a composed tap: up to 2^17), the last channel of
            # the second chunk takes every one back
            Cin = P["x"].shape[-1]
            P1["x"][..., 0], P1["x"][..., Cin - 1] = 512.0, 512.0
            P1["w"][..., 0], P1["w"][..., Cin - 1] = 64.0, -64.0
        return P1

    @staticmethod
    def outputs(row, P, hdt):
        import gemm_ref as G
        import ups4_ref as U4
        v, b = ups4.reference(P)
        Cin = P["x"].shape[-1]
        # tests/test_gpu_ups4_conv.py: comp = sum |x| * (half a storage ulp of each composed weight), the form's one new rounding
        wc = U4.compose(P["w"])
        mant = 7 if hdt == torch.bfloat16 else 10
        e = torch.floor(torch.log2(wc.abs().clamp_min(2.0 ** -120)))
        comp = U4.forward(P["x"], torch.where(wc == 0, torch.zeros_like(wc), torch.exp2(e - mant - 1)), absolute=True)
        tol = G.gauss_k(4 * Cin, hdt) * U[hdt] * b + U[hdt] * v.abs() + comp + FL[hdt]          # gpu_util.check_bound's tolerance
        return {"out": Out(v, tol, hdt, P.get("k", 0), row["prop"] != "top")}

    @staticmethod
    def emulate(row, P, hdt, mistake=None):
        import ups4_ref as U4
        x, w = P["x"], P["w"]
        if mistake == "flush_subnormal_operands":
            x, w = R.flush(x, hdt), R.flush(w, hdt)
        y = U4.forward(x, U4.compose(w, hdt=hdt)) + P["bias"]                                  # composed weights rounded once to storage
        return {"out": y.float().to(hdt)}


OPS = {c.__name__: c for c in (hed_tail, inorm, ln_live, chan_pool, scale_add, cab, swin_act, silu, rdb_epilogue, hed_fuse, conv7_out,
                               ctrl_emit_acc, win_attn, hat_attn, rdb_conv, conv7_in, merge_delta, ups4)}
SCALING_FAMILIES = ("hed", "inorm", "norm", "cab", "epi", "sat", "attn", "rdb", "merge", "ups4")


def derive(row, hdt):
    """The exponents of any row (range_image_cases.IMAGE_EXPS records them)."""
    if row["family"] not in SCALING_FAMILIES:
        return ()
    op = OPS[row["op"]]
    return tuple(op.derive(row, op.base(row, hdt), hdt))


def problems(row, hdt, exps):
    op = OPS[row["op"]]
    P0 = op.base(row, hdt)
    return P0, op.scaled(row, P0, exps, hdt)


def worst_ratio(got, o):
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    err = (g - o.value).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / o.tol.clamp_min(1e-300)).max())


def excluded(o0, o1):
    """What check 1 leaves out of an output: range_ref.excluded_mask on the two float64 references - but nothing of an exact output,
    nothing of an invariant one (k = 0: both runs round the same number) and no element whose tolerance is zero (its value is known
    exactly: a score whose every term is zero)."""
    if o1.exact or o1.k == 0:
        return torch.zeros_like(o1.value, dtype=torch.bool)
    return R.excluded_mask(o0.value, o1.value, o1.odt) & (o1.tol != 0)


def judge(row, hdt, exps, P0, P1, got0, got1, enforce=True):
    """Check 1 and check 2 over every output of a scaling row; prints the `[range]` line; dict(excluded, bitdiff, ratio, failed).
    An output with k None (the saturating sigmoids) has no base run to compare with: its expectation is exact."""
    op = OPS[row["op"]]
    o0, o1 = op.outputs(row, P0, hdt), op.outputs(row, P1, hdt)
    n_ex = bitdiff = total = 0
    ratio, finite = 0.0, True
    for name, o in o1.items():
        g1 = got1[name].double().cpu()
        total += g1.numel()
        finite = finite and bool(torch.isfinite(g1).all())
        ratio = max(ratio, worst_ratio(g1, o))
        if o.exact:
            want = o.value.to(o.odt).double()
            sure = torch.ones_like(g1, dtype=torch.bool) if o.sure is None else o.sure
            bitdiff += int((~((g1 == want) | ((g1 == 0) & (want == 0))) & sure).sum())
            n_ex += int((~sure).sum())
        if o.k is None:
            continue
        g0 = got0[name].double().cpu()
        ex = excluded(o0[name], o)
        want = (g0 * 2.0 ** o.k + o.offset).to(o.odt).double()
        bitdiff += R.check1(g1, want, ex, o.odt)[0]
        n_ex += int(ex.sum())
    R.report(row["id"], hdt, exps, n_ex, bitdiff, ratio)
    failed = bitdiff > 0 or not ratio <= 1.0 or n_ex > R.EXCLUDE_CAP * total or not finite
    if enforce:
        rid = row["id"]
        assert finite, f"{rid}: NaN / inf in the scaled output"
        assert n_ex <= R.EXCLUDE_CAP * total, f"{rid}: {n_ex} of {total} elements excluded"
        assert ratio <= 1.0, f"{rid}: the scaled run leaves the float64 bound by {ratio:.3g}x"
        assert bitdiff == 0, f"{rid}: {bitdiff} elements of the scaled run are not 2^k times the base run (or not the exact value)"
    return dict(excluded=n_ex, bitdiff=bitdiff, ratio=ratio, failed=failed)


def judge_single(row, hdt, P, got, enforce=True):
    """The activation rows: one run at the edge itself, judged against float64 under the kernel's own bound; `top` rows: f(x) = x bit
    for bit for the positive inputs."""
    op = OPS[row["op"]]
    (name, o), = op.outputs(row, P, hdt).items()
    g = got[name].cpu()
    ratio = worst_ratio(g, o)
    bitdiff = act_exact_at_top(P, g, hdt) if row["prop"] == "top" else 0
    R.report(row["id"], hdt, (), 0, bitdiff, ratio)
    failed = bitdiff > 0 or not ratio <= 1.0
    if enforce:
        assert ratio <= 1.0, f"{row['id']}: outside the float64 bound by {ratio:.3g}x (inf: a NaN / inf output)"
        assert bitdiff == 0, f"{row['id']}: {bitdiff} positive inputs at the top of the range did not come back as themselves"
    return dict(excluded=0, bitdiff=bitdiff, ratio=ratio, failed=failed)


def judge_specials(row, hdt, P, Ps, got_clean, got, enforce=True):
    """Every output element in the class torch's CPU evaluation gives; the clean samples with the bits of the run without specials.
    The `[range]` line counts class differences as bit differences; dict(classdiff, cleandiff, failed)."""
    op = OPS[row["op"]]
    want = op.torch_eval(row, Ps, hdt)
    classdiff = cleandiff = 0
    where = ""
    for name, w in want.items():
        g = got[name].cpu()
        bad = classes(g) != classes(w)
        if bool(bad.any()) and not where:
            i = tuple(bad.nonzero()[0].tolist())
            where = f"{name}{list(i)}: got {float(g[i])!r}, torch gives {float(w[i])!r}"
        classdiff += int(bad.sum())
        m = op.clean(row, Ps, name, g)
        assert bool(m.any()) and not bool(m.all()), f"{row['id']}: {name} needs clean and unclean elements"
        assert bool(torch.isfinite(w.double()[m]).all()), f"{row['id']}: torch's own answer is not finite on a sample claimed clean"
        cleandiff += R.same_bits(g[m], got_clean[name].cpu()[m])
    R.report(row["id"], hdt, (), 0, classdiff + cleandiff, 0.0 if not classdiff else float("inf"))
    if enforce:
        assert classdiff == 0, f"{row['id']}: {classdiff} elements are not in the class torch gives, first {where}"
        assert cleandiff == 0, f"{row['id']}: {cleandiff} elements of clean samples changed their bits"
    return dict(classdiff=classdiff, cleandiff=cleandiff, failed=classdiff + cleandiff > 0)
