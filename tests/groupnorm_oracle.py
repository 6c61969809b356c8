"""What tests/test_groupnorm.py (GPU), tests/test_groupnorm_cpu.py and tests/test_groupnorm_oracle_cpu.py
share (a plain module, imported by them):

* plain statements of the six operations of csrc/kernels/groupnorm.hip, written from their
  definitions and not from the kernels: torch, whole tensors, no slabs, no lanes, float64 unless
  `dtype=` says otherwise (the float32 run is how the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.
  figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and check() are those of
  tests/transformer_oracle.py; BARS below is entered into its table so that they see it.

Definitions. x [N, M, C] channels last, G groups of Cg = C / G consecutive channels, m = M * Cg;
group (n, g) is x[n, :, g*Cg : (g+1)*Cg]:

  1 col_sums     p_c = x[n, 0, c] (the pivot), S1[n, c] = sum_r (x - p_c), S2[n, c] = sum_r (x - p_c)^2
  2 fold_stats   per channel: d = S1 / M, mean_c = p_c + d, M2_c = S2 - S1 * d (clamped at 0);
                 per group, its channels having equal counts: mean = first + sum_c (mean_c - first) / Cg
                 (first = mean_c of the group's first channel), M2 = sum_c (M2_c + M * (mean_c - mean)^2),
                 var = M2 / m (biased), rstd = 1 / sqrt(var + eps)
                 rows: mean_c[n, c] = mean[n, g(c)], scale[n, c] = rstd[n, g(c)] * gamma_c
  3 apply        y = (x - mean_c) * scale + beta_c                 (gamma = 1 / beta = 0 when absent)
  4 bwd_sums     sdy[n, c] = sum_r dy, sdyx[n, c] = sum_r dy * (x - mean) * rstd
  5 bwd_fold     A[n, g] = sum_{c in g} gamma_c * sdy, B[n, g] = sum_{c in g} gamma_c * sdyx
                 p = rstd * gamma_c, q = -rstd^2 * B / m, r = -rstd * A / m   per (n, c)
                 dbeta[c] = sum_n sdy, dgamma[c] = sum_n sdyx      (+ the old value: accumulate)
  6 bwd_apply    dx = p * dy + q * (x - mean_c) + r
  By the definitions (stats_def, backward_def): mean = sum / m, var = sum (x - mean)^2 / m in two
  passes, xh = (x - mean) * rstd, dx = rstd * (gamma * dy - A / m - xh * B / m).

The float64 run of the statistics uses the two-pass definition; the float32 run uses operations 1
and 2, the kernel's pivoted one-pass form: the bars therefore measure the formula the project
chose, and a kernel that sums in another order has MARGIN to do it in.

Figures. Every comparison is element-wise: figure = max |got - want| / scale; for a bf16 output
half a bf16 ulp of `want` is taken off the error first. The scales are written out beside BARS.
Staging: mean and rstd are compared with the oracle first; y is then compared with apply() and
dx, dgamma, dbeta with backward_def() in float64 on the kernel's own mean / rstd, so a
cancellation error in a statistic is charged to the statistics figure, whose scale is honest
about it, and never hidden in a loose bar on the output."""
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

from tensorflow_train_distributed_amd.ops import _plan

F32 = torch.float32
BF16 = torch.bfloat16
EPS = 1e-3


def f32r(v):
    """A Python float as the kernels receive it (a C float)."""
    return float(torch.tensor(v, dtype=F32))


def _affine(gamma, beta, C, dtype, device="cpu"):
    g = gamma.to(dtype) if gamma is not None else torch.ones(C, dtype=dtype, device=device)
    b = beta.to(dtype) if beta is not None else torch.zeros(C, dtype=dtype, device=device)
    return g, b


def _per_channel(stat, C):
    """[N, G] -> [N, 1, C]: the value of each channel's group."""
    return stat.repeat_interleave(C // stat.shape[1], dim=1)[:, None, :]


# ------------------------------------------------------------------ forward
def stats_def(x, G, eps, dtype=F64):
    """(mean, var, rstd) [N, G] by the two-pass definition."""
    x = x.to(dtype)
    N, M, C = x.shape
    xg = x.reshape(N, M, G, C // G)
    mean = xg.sum((1, 3)) / (M * (C // G))
    var = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3)) / (M * (C // G))
    return mean, var, 1.0 / torch.sqrt(var + eps)


def col_sums(x, dtype=F64):
    """Operation 1: (pivot, S1, S2) [N, C]."""
    x = x.to(dtype)
    p = x[:, 0, :]
    d = x - p[:, None, :]
    return p, d.sum(1), (d * d).sum(1)


def fold_stats(p, S1, S2, M, G, eps, dtype=F64):
    """Operation 2 without the rows: (mean, var, rstd) [N, G]."""
    p, S1, S2 = p.to(dtype), S1.to(dtype), S2.to(dtype)
    N, C = p.shape
    Cg = C // G
    d = S1 / M
    mean_c = (p + d).reshape(N, G, Cg)
    M2_c = (S2 - S1 * d).clamp_min(0).reshape(N, G, Cg)
    first = mean_c[:, :, :1]
    mean = first[:, :, 0] + (mean_c - first).sum(2) / Cg
    M2 = (M2_c + M * (mean_c - mean[:, :, None]) ** 2).sum(2)
    var = M2 / (M * Cg)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def stats(x, G, eps, dtype=F64):
    """(mean, var, rstd): the definition in float64, operations 1 and 2 in any other dtype."""
    if dtype == F64:
        return stats_def(x, G, eps, dtype)
    return fold_stats(*col_sums(x, dtype), x.shape[1], G, eps, dtype)


def coef_rows(mean, rstd, gamma, C, dtype=F64):
    """The rows of operation 2: (mean_c, scale) [N, 1, C]."""
    g, _ = _affine(gamma, None, C, dtype, mean.device)
    return _per_channel(mean.to(dtype), C), _per_channel(rstd.to(dtype), C) * g


def apply(x, mean, rstd, gamma, beta, dtype=F64):
    """Operation 3."""
    C = x.shape[2]
    mean_c, scale = coef_rows(mean, rstd, gamma, C, dtype)
    _, b = _affine(None, beta, C, dtype, x.device)
    return (x.to(dtype) - mean_c) * scale + b


def apply_scale(x, mean, rstd, gamma, beta):
    """|(x - mean_c) * scale| + |beta|: what the fp32 sum works at before the store."""
    C = x.shape[2]
    mean_c, scale = coef_rows(mean, rstd, gamma, C, F64)
    _, b = _affine(None, beta, C, F64, x.device)
    return ((x.to(F64) - mean_c) * scale).abs() + b.abs()


# ------------------------------------------------------------------ backward
def bwd_sums(dy, x, mean, rstd, dtype=F64):
    """Operation 4: (sdy, sdyx) [N, C]."""
    C = x.shape[2]
    dy = dy.to(dtype)
    xh = (x.to(dtype) - _per_channel(mean.to(dtype), C)) * _per_channel(rstd.to(dtype), C)
    return dy.sum(1), (dy * xh).sum(1)


def bwd_fold(sdy, sdyx, mean, rstd, gamma, M, dg0=None, db0=None, dtype=F64):
    """Operation 5: {"dgamma", "dbeta" [C], "A", "B" [N, G], "rows": (mean_c, p, q, r) [N, 1, C]}."""
    sdy, sdyx, mean, rstd = sdy.to(dtype), sdyx.to(dtype), mean.to(dtype), rstd.to(dtype)
    N, C = sdy.shape
    G = mean.shape[1]
    m = M * (C // G)
    g, _ = _affine(gamma, None, C, dtype, sdy.device)
    A = (g * sdy).reshape(N, G, C // G).sum(2)
    B = (g * sdyx).reshape(N, G, C // G).sum(2)
    rows = (_per_channel(mean, C), _per_channel(rstd, C) * g, _per_channel(-(rstd * rstd) * B / m, C),
            _per_channel(-rstd * A / m, C))
    dgamma, dbeta = sdyx.sum(0), sdy.sum(0)
    if dg0 is not None:
        dgamma = dgamma + dg0.to(dtype)
    if db0 is not None:
        dbeta = dbeta + db0.to(dtype)
    return {"dgamma": dgamma, "dbeta": dbeta, "A": A, "B": B, "rows": rows}


def bwd_apply(dy, x, rows, dtype=F64):
    """Operation 6."""
    mean_c, p, q, r = rows
    return p * dy.to(dtype) + q * (x.to(dtype) - mean_c) + r


def backward(dy, x, mean, rstd, gamma, dg0=None, db0=None, dtype=F64):
    """(dx, dgamma, dbeta) through operations 4, 5 and 6."""
    f = bwd_fold(*bwd_sums(dy, x, mean, rstd, dtype), mean, rstd, gamma, x.shape[1], dg0, db0, dtype)
    return bwd_apply(dy, x, f["rows"], dtype), f["dgamma"], f["dbeta"]


def backward_def(dy, x, mean, rstd, gamma, dg0=None, db0=None, dtype=F64):
    """(dx, dgamma, dbeta) by the definitions, from given mean / rstd [N, G]."""
    dy, x = dy.to(dtype), x.to(dtype)
    N, M, C = x.shape
    G = mean.shape[1]
    m = M * (C // G)
    g, _ = _affine(gamma, None, C, dtype, x.device)
    rs = _per_channel(rstd.to(dtype), C)
    xh = (x - _per_channel(mean.to(dtype), C)) * rs
    gd = g * dy
    A = gd.reshape(N, M, G, C // G).sum((1, 3))
    B = (gd * xh).reshape(N, M, G, C // G).sum((1, 3))
    dx = rs * (gd - _per_channel(A, C) / m - xh * _per_channel(B, C) / m)
    dgamma, dbeta = (dy * xh).sum((0, 1)), dy.sum((0, 1))
    if dg0 is not None:
        dgamma = dgamma + dg0.to(dtype)
    if db0 is not None:
        dbeta = dbeta + db0.to(dtype)
    return dx, dgamma, dbeta


# ------------------------------------------------------------------ scales
def stats_scales(x, G, eps):
    """mean: A1 = sum |x| / m of the group. rstd: rstd * (1 + V / (var + eps)), its own rounding
    plus d rstd / d var = -rstd / (2 (var + eps)) times the error of var, whose sums work at
    V = E[(x - p_c)^2] + |mean| * max_c |mean_c - mean|: the pivoted second moment, and the
    squares of differences of fp32 channel means that are each an ulp of |mean| off."""
    x = x.to(F64)
    N, M, C = x.shape
    Cg = C // G
    mean, var, rstd = stats_def(x, G, eps)
    xg = x.reshape(N, M, G, Cg)
    A1 = xg.abs().sum((1, 3)) / (M * Cg)
    p = x[:, :1, :]
    Qp = ((x - p) ** 2).reshape(N, M, G, Cg).sum((1, 3)) / (M * Cg)
    mean_c = x.sum(1).reshape(N, G, Cg) / M
    D = (mean_c - mean[:, :, None]).abs().max(2).values
    V = Qp + mean.abs() * D
    return {"mean": A1, "rstd": rstd * (1 + V / (var + eps))}


def bwd_scales(dy, x, mean, rstd, gamma, dg0=None, db0=None):
    """dbeta: sum |dy| (+ |old|). dgamma: sum |dy * xh| (+ |old|). dx: rstd * (|gamma dy| +
    sum |gamma dy| / m + |xh| * sum |gamma dy xh| / m), the three terms of the definition."""
    dy, x = dy.to(F64), x.to(F64)
    N, M, C = x.shape
    G = mean.shape[1]
    m = M * (C // G)
    g, _ = _affine(gamma, None, C, F64, x.device)
    rs = _per_channel(rstd.to(F64), C)
    xh = ((x - _per_channel(mean.to(F64), C)) * rs).abs()
    gd = (g * dy).abs()
    A = gd.reshape(N, M, G, C // G).sum((1, 3))
    B = (gd * xh).reshape(N, M, G, C // G).sum((1, 3))
    out = {"dx": rs * (gd + _per_channel(A, C) / m + xh * _per_channel(B, C) / m),
           "dgamma": (dy.abs() * xh).sum((0, 1)), "dbeta": dy.abs().sum((0, 1))}
    if dg0 is not None:
        out["dgamma"] = out["dgamma"] + dg0.to(F64).abs()
    if db0 is not None:
        out["dbeta"] = out["dbeta"] + db0.to(F64).abs()
    return out


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_groupnorm_oracle_cpu.py prints them and asserts the relation).
BARS = {
    #                       scale of the figure                                        fp32
    "gn_mean": 7e-6,      # A1 = sum |x| / m of the group                              3.9e-7
    "gn_rstd": 3e-6,      # rstd * (1 + V / (var + eps)), stats_scales()               1.4e-7
    "gn_y": 3e-6,         # |(x - mean_c) * scale| + |beta|; bf16                      1.9e-7
    "gn_dx": 3e-6,        # bwd_scales(); bf16                                         1.4e-7
    "gn_dgamma": 3e-6,    # sum |dy * xh| (+ |old|)                                    1.5e-7
    "gn_dbeta": 2e-6,     # sum |dy| (+ |old|)                                         7.4e-8
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
# (C, G) of the fast form (bf16, C % 8 == 0): one group; two; one channel per group; two channels
# per group; four; a wide group; Cg = 10 (a lane's 8 channels straddle two groups); more lanes per
# row than one block holds, with many groups and with one.
FAST_CG = [(8, 1), (16, 2), (16, 16), (16, 8), (32, 8), (64, 2), (40, 4), (2056, 257), (2056, 1)]
# (C, G) of the generic form: (65, 5) has a group across a 64-wide column boundary
GENERIC_CG = [(1, 1), (3, 3), (6, 2), (12, 1), (65, 5), (130, 2)]
FAST_AS_FP32 = [(16, 8), (40, 4)]
CASE_N = (1, 3)
CAP = _plan.gn_max_slabs()


def case_Ms(C, fast):
    """1, 2 and either side of the rows a block has in flight."""
    r = _plan.gn_rows_per_block(C, fast)
    return sorted({1, 2, r + 1} | ({r - 1} if r > 1 else set()))


# (N, M, C, G): N * T one below the slab cap, at it, and past it (two rows per slab, the last slab
# one row; three rows per slab, the last slab shorter), for one image and for three
SLAB_CASES = ([(1, M, 8, 2) for M in (CAP - 1, CAP, CAP + 1, 2 * CAP + 1)]
              + [(3, M, 16, 2) for M in (CAP // 3 - 1, CAP // 3, CAP // 3 + 1)])
# kinds of special values, see inputs()
VALUE_KINDS = ("mean_far", "const_group", "zero_image", "gamma0", "eps0")
VALUE_SHAPES = [(2, 37, 16, 4, BF16), (2, 37, 16, 4, F32), (2, 11, 6, 2, F32)]
RANK_SHAPES = [(5, 12), (3, 7, 12), (2, 3, 5, 12), (2, 2, 3, 2, 12)]


def all_cases():
    """Every (N, M, C, G, dtype, kind) the GPU tests run and the float32 run sets the bars over."""
    out = []
    for C, G in FAST_CG:
        out += [(N, M, C, G, BF16, "plain") for N in CASE_N for M in case_Ms(C, True)]
    for C, G in GENERIC_CG:
        out += [(N, M, C, G, dt, "plain") for dt in (F32, BF16) for N in CASE_N for M in case_Ms(C, False)]
    for C, G in FAST_AS_FP32:
        out += [(N, M, C, G, F32, "plain") for N in CASE_N for M in case_Ms(C, True)]
    out += [(N, M, C, G, BF16, "plain") for N, M, C, G in SLAB_CASES]
    out += [(N, M, C, G, dt, kind) for kind in VALUE_KINDS for N, M, C, G, dt in VALUE_SHAPES]
    return out


def case_eps(kind):
    return 0.0 if kind == "eps0" else EPS


# ------------------------------------------------------------------ seeded inputs
def inputs(N, M, C, G, dt, kind="plain"):
    """CPU tensors of a case: x, dy [N, M, C] of dtype dt (values rounded to it, which is what
    the oracle sees); gamma, beta, dg0, db0 fp32 [C]. x is N(mu_c, sd_c) per channel with
    mu ~ 2 N(0,1), sd ~ exp(N(0,1)/2), plus a per-image shift. Kinds:
      mean_far     group 0 of every image: 1000 (fp32) or 100 (bf16) times its spread away from 0
      const_group  group 0 of image 0 is the constant 3.0
      zero_image   image 0 is all zero
      gamma0       gamma[0] = 0
      eps0         plain data, eps = 0 (case_eps)"""
    gen = _gen(N, M, C, G, VALUE_KINDS.index(kind) + 1 if kind in VALUE_KINDS else 0, int(dt == BF16))
    Cg = C // G
    mu, sd = torch.randn(C, generator=gen) * 2, torch.exp(torch.randn(C, generator=gen) * 0.5)
    x = torch.randn(N, M, C, generator=gen) * sd + mu + torch.randn(N, 1, 1, generator=gen)
    dy = torch.randn(N, M, C, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen)
    if kind == "mean_far":
        x[:, :, :Cg] = (1000.0 if dt == F32 else 100.0) + torch.randn(N, M, Cg, generator=gen)
    elif kind == "const_group":
        x[0, :, :Cg] = 3.0
    elif kind == "zero_image":
        x[0] = 0.0
    elif kind == "gamma0":
        gamma[0] = 0.0
    return {"x": x.to(dt), "dy": dy.to(dt), "gamma": gamma, "beta": beta,
            "dg0": torch.randn(C, generator=gen) * 10, "db0": torch.randn(C, generator=gen) * 10}


# ------------------------------------------------------------------ figures
def stats_figures(mean, rstd, x, G, eps):
    """gn_mean, gn_rstd of a result against the float64 definition."""
    m64, _, r64 = stats_def(x, G, eps)
    sc = stats_scales(x, G, eps)
    return {"gn_mean": figure(mean, m64, sc["mean"]), "gn_rstd": figure(rstd, r64, sc["rstd"])}


def y_figure(y, x, mean, rstd, gamma, beta):
    """gn_y against apply() in float64 on the given (the kernel's own) mean / rstd."""
    return {"gn_y": figure(y, apply(x, mean, rstd, gamma, beta), apply_scale(x, mean, rstd, gamma, beta),
                           bf16_store=y.dtype == BF16)}


def bwd_figures(dx, dgamma, dbeta, dy, x, mean, rstd, gamma, dg0=None, db0=None):
    """gn_dx, gn_dgamma, gn_dbeta (each where given) against backward_def() in float64 on the given
    (the kernel's own) mean / rstd."""
    want = backward_def(dy, x, mean, rstd, gamma, dg0, db0)
    sc = bwd_scales(dy, x, mean, rstd, gamma, dg0, db0)
    out = {}
    if dx is not None:
        out["gn_dx"] = figure(dx, want[0], sc["dx"], bf16_store=dx.dtype == BF16)
    if dgamma is not None:
        out["gn_dgamma"] = figure(dgamma, want[1], sc["dgamma"])
    if dbeta is not None:
        out["gn_dbeta"] = figure(dbeta, want[2], sc["dbeta"])
    return out


def fp32_figures(N, M, C, G, dt, kind):
    """Every figure of a case with this module's float32 run in the kernel's place."""
    inp = inputs(N, M, C, G, dt, kind)
    eps = case_eps(kind)
    x, dy, gamma, beta = inp["x"], inp["dy"], inp["gamma"], inp["beta"]
    mean, _, rstd = stats(x, G, f32r(eps), F32)
    figs = stats_figures(mean, rstd, x, G, eps)
    figs.update(y_figure(apply(x, mean, rstd, gamma, beta, F32), x, mean, rstd, gamma, beta))
    dx, dg, db = backward(dy, x, mean, rstd, gamma, inp["dg0"], inp["db0"], F32)
    figs.update(bwd_figures(dx, dg, db, dy, x, mean, rstd, gamma, inp["dg0"], inp["db0"]))
    return figs
