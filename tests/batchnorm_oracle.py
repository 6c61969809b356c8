"""What tests/test_batchnorm_kernels.py (GPU) and tests/test_batchnorm_oracle_cpu.py share (a plain
module, imported by them):

* plain statements of the operations of csrc/kernels/batchnorm.hip, written from the definitions
  in its header comment and not from the kernels: torch, whole tensors, no blocks, no lanes,
  float64 unless `dtype=` says otherwise (the float32 run is how the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.
  figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and check() are those of
  tests/transformer_oracle.py; BARS below is entered into its table so that they see it.

Definitions (rows r of M, channels c of C, everything per channel):

  forward   mean = sum_r x / M, var = sum_r (x - mean)^2 / M (two-pass), rstd = 1/sqrt(var + eps)
            scale = gamma*rstd, shift = beta - mean*scale          (gamma = 1, beta = 0 if absent)
            moving = moving*momentum + batch*(1 - momentum), the variance unbiased
            (var*M/(M-1)) when M > 1                               (the TF/Keras convention)
  apply     out = act(y*scale + shift + res), res = r or r*rscale + rshift; the mask bit of an
            element is [stored bf16 out > 0], bit j of byte i for element 8*i + j
  backward  g = dy*[out > 0]; dbeta = sum_r g; dgamma = sum_r g*(y - mean)*rstd
            dz = gamma*rstd*(g - dbeta/M - xhat*dgamma/M), xhat = (y - mean)*rstd
  split     from the sums sg = sum_r g, sgy = sum_r g*y: dgamma = rstd*(sgy - mean*sg),
            a = gamma*rstd, b = -gamma*rstd^2*dgamma/M, c = -a*sg/M - b*mean, dz = a*g + b*y + c
            (+ the old dgamma / dbeta: accumulate; a, b, c never see the old values)

The float32 run uses the same definitions with dtype=torch.float32, except that var and dgamma
take the kernel's one-pass forms, E[x^2] - mean^2 (clamped at 0) and rstd*(sgy - mean*sg): the
bars therefore measure the formula the project chose, at the scale that formula works at, and a
kernel that sums in another order has MARGIN to do it in.

Figures. Every comparison is element-wise: figure = max |got - want| / scale; for a bf16 output
half a bf16 ulp of `want` is taken off the error first. The scales are written out beside BARS.
Staging: the statistics are compared with the oracle first; the apply output is then compared
with apply() in float64 on the kernel's own scale / shift and dz with dz_from_coef() on the
kernel's own coef, so a cancellation error in a coefficient is charged to the statistics figure,
whose scale is honest about it, and never hidden in a loose bar on the output."""
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

F32 = torch.float32
EPS = 1e-5
MOMENTUM = 0.9


def f32r(v):
    """A Python float as the kernels receive it (a C float)."""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------ forward
def _affine(gamma, beta, like, dtype):
    g = gamma.to(dtype) if gamma is not None else torch.ones_like(like)
    b = beta.to(dtype) if beta is not None else torch.zeros_like(like)
    return g, b


def _finish(mean, var, gamma, beta, eps, dtype):
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = _affine(gamma, beta, mean, dtype)
    scale = g * rstd
    return {"mean": mean, "var": var, "rstd": rstd, "scale": scale, "shift": b - mean * scale}


def fwd_stats(x, gamma, beta, eps, dtype=F64, one_pass=None):
    """Statistics and affine coefficients of x [M, C]. one_pass (default: every dtype but
    float64): var = E[x^2] - mean^2 clamped at 0, the kernel's form."""
    x = x.to(dtype)
    M = x.shape[0]
    mean = x.sum(0) / M
    if dtype != F64 if one_pass is None else one_pass:
        var = ((x * x).sum(0) / M - mean * mean).clamp_min(0)
    else:
        var = ((x - mean) ** 2).sum(0) / M
    return _finish(mean, var, gamma, beta, eps, dtype)


def stats_from_sums(s, q, count, gamma, beta, eps, dtype=F64):
    """The same from per-channel totals (sum x, sum x^2) of `count` rows: all there is to go by
    when the partial sums come from a conv epilogue."""
    s, q = s.to(dtype), q.to(dtype)
    mean = s / count
    return _finish(mean, (q / count - mean * mean).clamp_min(0), gamma, beta, eps, dtype)


def running(rm0, rv0, mean, var, M, momentum, dtype=F64):
    unbiased = var * M / (M - 1) if M > 1 else var
    return (rm0.to(dtype) * momentum + mean.to(dtype) * (1 - momentum),
            rv0.to(dtype) * momentum + unbiased.to(dtype) * (1 - momentum))


def stats_scales(A1, Q, ref, gamma, beta, eps, M=None, momentum=None, rm0=None, rv0=None):
    """The scale of each statistics figure. A1 = sum|x| / M and Q = E[x^2] are the magnitudes the
    two sums work at. mean: A1. var: Q (both terms of E[x^2] - mean^2 are that large). rstd:
    rstd*(1 + Q/(var + eps)): its own rounding (rsqrtf) plus d rstd/d var = -rstd/(2(var + eps))
    times the error of var. scale: |gamma| times that. shift = beta - mean*scale: |beta| +
    A1*|gamma|*rstd (the product and the error of mean) + |mean| * the scale of `scale`. Running
    statistics: |old|*momentum + (1 - momentum) * the scale of the batch value."""
    A1, Q = A1.to(F64), Q.to(F64)
    mean, var, rstd = ref["mean"].to(F64), ref["var"].to(F64), ref["rstd"].to(F64)
    g, b = _affine(gamma, beta, mean, F64)
    s_rstd = rstd * (1 + Q / (var + eps))
    s_scale = g.abs() * s_rstd
    out = {"mean": A1, "var": Q, "rstd": s_rstd, "scale": s_scale,
           "shift": b.abs() + A1 * g.abs() * rstd + mean.abs() * s_scale}
    if rm0 is not None:
        ub = M / (M - 1) if M > 1 else 1.0
        out["run_mean"] = rm0.to(F64).abs() * momentum + A1 * (1 - momentum)
        out["run_var"] = rv0.to(F64).abs() * momentum + Q * ub * (1 - momentum)
    return out


def data_scales(x):
    """(A1, Q) of x [M, C]."""
    x = x.to(F64)
    return x.abs().sum(0) / x.shape[0], (x * x).sum(0) / x.shape[0]


def block_sums(x, T, other=None, dtype=F64):
    """partial [T, 2, C] of bn_stats_partial (sum x, sum x^2) or, with `other`, of the backward
    partial kernel (sum x, sum x*other): block b covers rows [b*rpb, min(M, (b+1)*rpb)),
    rpb = ceil(M / T); and the same sums of the magnitudes (the scales)."""
    x = x.to(dtype)
    M, C = x.shape
    prod = x * (x if other is None else other.to(dtype))
    rpb = (M + T - 1) // T
    out = torch.zeros((T, 2, C), dtype=dtype, device=x.device)
    mag = torch.zeros((T, 2, C), dtype=dtype, device=x.device)
    for b in range(T):
        lo, hi = b * rpb, min(M, (b + 1) * rpb)
        if lo < hi:
            out[b, 0], out[b, 1] = x[lo:hi].sum(0), prod[lo:hi].sum(0)
            mag[b, 0], mag[b, 1] = x[lo:hi].abs().sum(0), prod[lo:hi].abs().sum(0)
    return out, mag


# ------------------------------------------------------------------ apply
def apply(y, scale, shift, residual=None, rscale=None, rshift=None, relu=False, dtype=F64):
    f = y.to(dtype) * scale.to(dtype) + shift.to(dtype)
    if residual is not None:
        r = residual.to(dtype)
        f = f + (r * rscale.to(dtype) + rshift.to(dtype) if rscale is not None else r)
    return torch.where(f > 0, f, torch.zeros_like(f)) if relu else f


def apply_scale(y, scale, shift, residual=None, rscale=None, rshift=None):
    """|y*scale| + |shift| + |r*rscale| + |rshift|: what the fp32 sum works at before the store."""
    s = (y.to(F64) * scale.to(F64)).abs() + shift.to(F64).abs()
    if residual is not None:
        r = residual.to(F64).abs()
        s = s + (r * rscale.to(F64).abs() + rshift.to(F64).abs() if rscale is not None else r)
    return s


_BITS = (1, 2, 4, 8, 16, 32, 64, 128)


def mask_bits(out):
    """uint8 [numel/8]: bit j of byte i is [out.flatten()[8*i + j] > 0]."""
    b = (out.to(F64) > 0).reshape(-1, 8).to(torch.int32)
    w = torch.tensor(_BITS, dtype=torch.int32, device=out.device)
    return (b * w).sum(1).to(torch.uint8)


def mask_bools(mask, shape):
    w = torch.tensor(_BITS, dtype=torch.int32, device=mask.device)
    return ((mask.to(torch.int32)[:, None] & w) != 0).reshape(shape)


# ------------------------------------------------------------------ backward
def relu_grad(dy, keep, dtype=F64):
    """g = dy * [out > 0]; keep: bool like dy, or None (no ReLU)."""
    g = dy.to(dtype)
    return g if keep is None else torch.where(keep, g, torch.zeros_like(g))


def bwd_direct(g, y, mean, rstd, gamma, dg0=None, db0=None, dtype=F64):
    """(dz, dgamma, dbeta) by the definitions."""
    g, y, mean, rstd = g.to(dtype), y.to(dtype), mean.to(dtype), rstd.to(dtype)
    M = y.shape[0]
    gam, _ = _affine(gamma, None, mean, dtype)
    xhat = (y - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dz = gam * rstd * (g - dbeta / M - xhat * dgamma / M)
    if dg0 is not None:
        dgamma, dbeta = dgamma + dg0.to(dtype), dbeta + db0.to(dtype)
    return dz, dgamma, dbeta


def bwd_sums(g, y, dtype=F64):
    g, y = g.to(dtype), y.to(dtype)
    return g.sum(0), (g * y).sum(0)


def bwd_coef(sg, sgy, count, mean, rstd, gamma, dg0=None, db0=None, dtype=F64):
    """{"dgamma", "dbeta", "coef" [3, C]} from the sums: the kernel's split."""
    sg, sgy, mean, rstd = sg.to(dtype), sgy.to(dtype), mean.to(dtype), rstd.to(dtype)
    gam, _ = _affine(gamma, None, mean, dtype)
    dgam = rstd * (sgy - mean * sg)
    a = gam * rstd
    b = -gam * rstd * rstd * dgam / count
    c = -a * sg / count - b * mean
    dgamma, dbeta = (dgam, sg) if dg0 is None else (dgam + dg0.to(dtype), sg + db0.to(dtype))
    return {"dgamma": dgamma, "dbeta": dbeta, "coef": torch.stack([a, b, c])}


def bwd_scales(asg, asgy, count, mean, rstd, gamma, dg0=None, db0=None):
    """asg = sum|g|, asgy = sum|g*y| (or sum_t |partial_t| where only partial sums are known).
    dbeta: asg (+ |old|). dgamma = rstd*(sgy - mean*sg): rstd*(asgy + |mean|*asg) (+ |old|).
    coef a = gamma*rstd: itself. b = -gamma*rstd^2*dgamma/M: |gamma|*rstd^2/M * the scale of
    dgamma (without the old value). c = -a*sg/M - b*mean: |a|*asg/M + |mean| * the scale of b."""
    asg, asgy, mean, rstd = asg.to(F64), asgy.to(F64), mean.to(F64).abs(), rstd.to(F64)
    gam, _ = _affine(gamma, None, mean, F64)
    s_dg = rstd * (asgy + mean * asg)
    s_a = gam.abs() * rstd
    s_b = gam.abs() * rstd * rstd * s_dg / count
    out = {"dbeta": asg, "dgamma": s_dg, "coef": torch.stack([s_a, s_b, s_a * asg / count + mean * s_b])}
    if dg0 is not None:
        out["dgamma"], out["dbeta"] = s_dg + dg0.to(F64).abs(), asg + db0.to(F64).abs()
    return out


def dz_from_coef(coef, g, y, dtype=F64):
    c = coef.to(dtype)
    return c[0] * g.to(dtype) + c[1] * y.to(dtype) + c[2]


def dz_scale(coef, g, y):
    c = coef.to(F64).abs()
    return c[0] * g.to(F64).abs() + c[1] * y.to(F64).abs() + c[2]


def e2e_scales(y, g, ref, gamma, eps):
    """End to end (the backward from the kernels' own forward state against the float64 oracle
    of the whole) the errors of the state come on top. With R = the scale of rstd above and
    A1 = sum|y|/M, which bounds |mean| and is the scale of its error:
      dbeta   sum|g|
      dgamma  rstd*(sum|g*y| + A1*sum|g|)   the sums, and the error of mean
              + R*sum|g*(y - mean)|         the error of rstd
      dz      |gamma|*R*(|g| + sum|g|/M)    gamma*rstd*(g - dbeta/M)
              + |gamma|*R*(|y| + A1)*(the scale of dgamma)/M   gamma*rstd*xhat*dgamma/M, which
                                            the kernel evaluates as b*y + c with c holding -b*mean"""
    y, g = y.to(F64), g.to(F64)
    M = y.shape[0]
    A1, Q = data_scales(y)
    rstd, mean, var = ref["rstd"], ref["mean"], ref["var"]
    gam, _ = _affine(gamma, None, mean, F64)
    R = rstd * (1 + Q / (var + eps))
    asg = g.abs().sum(0)
    s_dg = rstd * ((g * y).abs().sum(0) + A1 * asg) + R * (g * (y - mean)).abs().sum(0)
    s_dz = gam.abs() * R * (g.abs() + asg / M) + gam.abs() * R * (y.abs() + A1) * s_dg / M
    return {"e2e_dbeta": asg, "e2e_dgamma": s_dg, "e2e_dz": s_dz}


# ------------------------------------------------------------------ fp8 copies
def fp8_half_step(v, e5m2=False):
    """Half a step of the fp8 format at each (already scaled and clamped) value: 2^-4 (e4m3) or
    2^-3 (e5m2) relative on normals, the absolute half step below the normal range."""
    rel, sub = (2.0 ** -3, 2.0 ** -17) if e5m2 else (2.0 ** -4, 2.0 ** -10)
    return (v.to(F64).abs() * rel).clamp_min(sub)


def fp8_decode(q8, e5m2=False):
    return q8.cpu().view(torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn).to(F64)


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_batchnorm_oracle_cpu.py prints them and asserts the relation).
BARS = {
    #                         scale of the figure                                      fp32
    "bn_partial": 4e-6,     # sum|x| and sum x^2 of the block's rows                   2.1e-7
    "bn_sums": 4e-6,        # sum_t |partial_t| (the atomic fold)                      2.4e-7
    "bn_mean": 5e-6,        # A1 = sum|x| / M                                          2.6e-7
    "bn_var": 9e-6,         # Q = E[x^2]                                               5.5e-7
    "bn_rstd": 5e-6,        # rstd*(1 + Q/(var + eps))                                 2.7e-7
    "bn_scale": 5e-6,       # |gamma| * the scale of rstd                              2.7e-7
    "bn_shift": 5e-6,       # |beta| + A1*|gamma|*rstd + |mean| * the scale of `scale` 2.7e-7
    "bn_run_mean": 4e-6,    # |old|*momentum + A1*(1 - momentum)                       2.4e-7
    "bn_run_var": 8e-6,     # |old|*momentum + Q*M/(M-1)*(1 - momentum)                4.7e-7
    "bn_out": 3e-6,         # |y*scale| + |shift| + |r*rscale| + |rshift|; bf16        1.3e-7
    "bn_dbeta": 5e-6,       # sum|g| (+ |old|)                                         2.7e-7
    "bn_dgamma": 5e-6,      # rstd*(sum|g*y| + |mean|*sum|g|) (+ |old|)                2.7e-7
    "bn_coef": 5e-6,        # bwd_scales(): each row's own propagation                 3.2e-7
    "bn_dz": 3e-6,          # |a*g| + |b*y| + |c|; bf16                                1.6e-7
    "bn_e2e_dbeta": 1e-6,   # e2e_scales()                                             1.3e-8
    "bn_e2e_dgamma": 1e-6,  # e2e_scales()                                             3.4e-8
    "bn_e2e_dz": 3e-6,      # e2e_scales(); bf16                                       1.4e-7
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
# fixed channel indices of every C (C >= 8)
CH_NORMAL, CH_MEAN64, CH_CONST, CH_ZERO, CH_OUTLIER, CH_GAMMA0, CH_GAMMA_NEG, CH_MASKED = range(8)

STATS_C = (8, 24, 40, 64, 96, 2048, 2056)


def rlanes(C):
    return 256 // min(C // 8, 256)


def stats_Ms(C):
    """1, 2, rlanes - 1, either side of the step of bn_num_partials from 1 to 2, and an M with three
    partial rows whose last block is shorter than the others (M = 3k + 1: blocks k+1, k+1, k-1)."""
    r = rlanes(C)
    m3 = next(m for m in range(32 * r + 1, 32 * r + 4) if m % 3 == 1)
    return sorted({1, 2, 16 * r, 16 * r + 1, m3} | ({r - 1} if r > 1 else set()))


STATS_CASES = [(M, C) for C in STATS_C for M in stats_Ms(C)]

FOLD_T = (1, 7, 8, 9, 255, 256, 257, 1000, 8192, 8193)
FOLD_C = (8, 40, 2048)
FOLD_COUNT = 50176.0

APPLY_C = (8, 24, 64, 96, 2048, 4096)
APPLY_OPTIONS = ("plain", "relu", "residual", "residual_bn")


def apply_Ms(C):
    """M*C/8 vectors below 256, 1024 (or the last M below it), the first M past it, and a few
    blocks of 1024 with a partial last one."""
    cg = C // 8
    return sorted({max(1, 255 // cg), max(1, 1024 // cg), 1024 // cg + 1, 3172 // cg + 1})


APPLY_CASES = [(M, C) for C in APPLY_C for M in apply_Ms(C)]
E2E_CASES = [(77, 64), (600, 96), (300, 2048)]
WRAP_M, WRAP_C = 1048576 + 8, 64


# ------------------------------------------------------------------ seeded inputs
def affine_inputs(C, gen):
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[CH_GAMMA0], gamma[CH_GAMMA_NEG] = 0.0, -0.75
    return gamma, torch.randn(C, generator=gen)


def stats_inputs(M, C):
    """x bf16 [M, C]: channel CH_NORMAL N(0,1), CH_MEAN64 64 + N(0,1), CH_CONST 3.0, CH_ZERO 0,
    CH_OUTLIER 0.1*N(0,1) with 200 in row M//2, the others N(mu, sd) with mu ~ 2*N(0,1) and
    sd ~ exp(N(0,1)); gamma (0 at CH_GAMMA0, -0.75 at CH_GAMMA_NEG), beta, old running stats."""
    gen = _gen(M, C, 1)
    mu, sd = torch.randn(C, generator=gen) * 2, torch.exp(torch.randn(C, generator=gen))
    x = torch.randn(M, C, generator=gen) * sd + mu
    x[:, CH_NORMAL] = torch.randn(M, generator=gen)
    x[:, CH_MEAN64] = 64 + torch.randn(M, generator=gen)
    x[:, CH_CONST] = 3.0
    x[:, CH_ZERO] = 0.0
    x[:, CH_OUTLIER] = 0.1 * torch.randn(M, generator=gen)
    x[M // 2, CH_OUTLIER] = 200.0
    gamma, beta = affine_inputs(C, gen)
    return {"x": x.bfloat16(), "gamma": gamma, "beta": beta,
            "rm0": torch.randn(C, generator=gen), "rv0": torch.rand(C, generator=gen) + 0.5}


def fold_inputs(T, C):
    """partial fp32 [T, 2, C]: a float64 split of known totals (sum x, sum x^2 of FOLD_COUNT rows
    with the special channels of stats_inputs) into T positive shares plus zero-sum noise, rounded
    to fp32. The truth is the float64 sum of the rounded shares. Also what the backward fold needs:
    a state (mean, rstd) to read the same rows as (sum g, sum g*y) with, and old dgamma / dbeta."""
    gen = _gen(T, C, 2)
    mean = torch.randn(C, generator=gen, dtype=F64) * 2
    var = torch.exp(torch.randn(C, generator=gen, dtype=F64))
    mean[CH_MEAN64], var[CH_MEAN64] = 64.0, 1.0
    mean[CH_CONST], var[CH_CONST] = 3.0, 0.0
    mean[CH_ZERO], var[CH_ZERO] = 0.0, 0.0
    tot = torch.stack([mean * FOLD_COUNT, (var + mean * mean) * FOLD_COUNT])
    w = torch.rand(T, 1, C, generator=gen, dtype=F64) + 0.1
    w /= w.sum(0, keepdim=True)
    part = w * tot
    if T > 1:
        noise = torch.randn(T, 2, C, generator=gen, dtype=F64)
        part += 0.25 * (noise - noise.mean(0, keepdim=True)) * tot.abs() / T
    gamma, beta = affine_inputs(C, gen)
    return {"partial": part.float(), "gamma": gamma, "beta": beta,
            "rm0": torch.randn(C, generator=gen), "rv0": torch.rand(C, generator=gen) + 0.5,
            "mean": torch.randn(C, generator=gen), "rstd": torch.rand(C, generator=gen) + 0.5,
            "dg0": torch.randn(C, generator=gen) * 100, "db0": torch.randn(C, generator=gen) * 100}


def fold_truth(partial):
    """(s, q, sum_t|s_t|, sum_t|q_t|) per channel, float64."""
    p = partial.to(F64)
    return p[:, 0].sum(0), p[:, 1].sum(0), p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)


def zero_rows(M):
    return sorted({0, M // 2, M - 1})


def apply_inputs(M, C):
    """y, res, dy, out bf16 [M, C]; scale, shift, rscale, rshift, gamma, mean, rstd fp32 [C].
    In rows zero_rows(M): channel 0 lands exactly on +0 (y = 0, scale 1, shift 0), channel 1 on
    -0 (y = -0, shift -0) and channel 2 on 2^-140, which rounds to 0 in bf16 (y = 2^-120,
    scale 2^-20); the residual is 0 (-0 in channel 1) there and rscale 1, rshift 0 (-0).
    `out` is a stand-in for a stored ReLU output for the backward: N(0,1) with the same zeros and
    channel CH_MASKED nowhere positive."""
    gen = _gen(M, C, 3)
    y, res = torch.randn(M, C, generator=gen) * 2, torch.randn(M, C, generator=gen)
    dy, out = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    scale, shift = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    rscale, rshift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.5
    rows = zero_rows(M)
    scale[0:3] = torch.tensor([1.0, 1.0, 2.0 ** -20])
    shift[0:3] = torch.tensor([0.0, -0.0, 0.0])
    rscale[0:3] = 1.0
    rshift[0:3] = torch.tensor([0.0, -0.0, 0.0])
    special = torch.tensor([0.0, -0.0, 2.0 ** -120])
    zeros = torch.tensor([0.0, -0.0, 0.0])
    for r in rows:
        y[r, 0:3], res[r, 0:3], out[r, 0:3] = special, zeros, zeros
    out[:, CH_MASKED] = -out[:, CH_MASKED].abs()
    y, res, dy, out = y.bfloat16(), res.bfloat16(), dy.bfloat16(), out.bfloat16()
    st = fwd_stats(y, None, None, EPS)
    gamma, _ = affine_inputs(C, gen)
    return {"y": y, "res": res, "dy": dy, "out": out, "scale": scale, "shift": shift, "rscale": rscale,
            "rshift": rshift, "gamma": gamma, "mean": st["mean"].float(), "rstd": st["rstd"].float(),
            "dg0": torch.randn(C, generator=gen) * 10, "db0": torch.randn(C, generator=gen) * 10}


def apply_kwargs(inp, option):
    """The oracle's arguments of an APPLY_OPTIONS entry: (residual, rscale, rshift, relu)."""
    if option == "plain":
        return None, None, None, False
    if option == "relu":
        return None, None, None, True
    if option == "residual":
        return inp["res"], None, None, True
    return inp["res"], inp["rscale"], inp["rshift"], True


def e2e_inputs(M, C):
    """A whole training-mode BN + residual + ReLU: y as stats_inputs' x, res and dy N(0,1)."""
    inp = stats_inputs(M, C)
    gen = _gen(M, C, 4)
    inp["y"] = inp.pop("x")
    inp["res"] = torch.randn(M, C, generator=gen).bfloat16()
    inp["dy"] = torch.randn(M, C, generator=gen).bfloat16()
    return inp


# ------------------------------------------------------------------ figures
def stats_figures(got, ref, scales):
    """{bar name: figure} for the entries of `got` (mean, var, rstd, scale, shift, run_*)."""
    return {"bn_" + k: figure(v, ref[k], scales[k]) for k, v in got.items() if v is not None}


def bwd_figures(got, ref, scales):
    return {"bn_" + k: figure(v, ref[k], scales[k]) for k, v in got.items() if v is not None}
