"""What tests/test_nn_generic_kernels.py (GPU) and tests/test_nn_generic_oracle_cpu.py share (a
plain module, imported by them):

* plain statements of the operations of csrc/kernels/nn_generic.hip (the pooling and in_top_k
  kernels apart, which tests/pooling_oracle.py and tests/xent_oracle.py state) and of
  csrc/kernels/gemm_f32.hip, written from the definitions in the comments of those files and not
  from the kernel bodies: torch, whole tensors, no blocks, no lanes, float64 unless `dtype=` says
  otherwise (the float32 run is how the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.
  figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and check() are those of
  tests/transformer_oracle.py; BARS below is entered into its table so that they see it.

Definitions (rows r of M, columns c of C or H):

  col_stats    part[t][0][c] = sum_r a, part[t][1][c] = sum_r a*a (mode 0), sum_r a*b (mode 1),
               sum_r a*(b - mu[r])*rs[r] (mode 2), over the rows [t*rpb, (t+1)*rpb) below M,
               rpb = ceil(M/T); a block without rows holds zeros
  col_reduce2  o0[c] = sum_t part[t][0][c] (+ the old o0 with acc), o1 likewise from part[t][1]
  col_affine   out = a*c0[c] + b*c1[c] + c2[c] over the flat index, c = i % C (absent terms 0)
  bn_infer     rstd = 1/sqrt(mv + eps), scale = gamma*rstd, shift = beta - mm*scale (gamma = 1,
               beta = 0 if absent); dgamma = rstd*(sum g*x - mm*sum g), dbeta = sum g
  layer norm   mean = sum_c x / H, var = sum_c (x - mean)^2 / H (two-pass), rstd = 1/sqrt(var+eps)
               xh = (x - mean)*rstd, y = xh*gamma + beta
               g = dy*gamma, dx = rstd*(g - mean_c(g) - xh*mean_c(g*xh))
               dgamma = sum_r dy*xh, dbeta = sum_r dy
  gather       out[r] = table[ids[r]], a row of zeros where ids[r] is outside [0, V)
  scatter_add  table[ids[r]] += dy[r] row by row, rows with ids[r] outside [0, V) dropped
  unary        tanh(x), sigmoid(x) = 1/(1 + exp(-x)); from the output y: dy*(1 - y^2), dy*y*(1 - y)
  sum_all      scale * sum(x);  fill_scaled: g*scale everywhere;  row_scale: a[r][c]*g[r]
  gemm         C = op(A).op(B) + bias[n] + beta*C, op the optional transpose

Figures. Every comparison is element-wise: figure = max |got - want| / scale; for a bf16 output
half a bf16 ulp of `want` is taken off the error first. The scales are written out beside BARS.
Staging: statistics are compared with the oracle first; LayerNorm's y and dx are then compared
with the float64 statement on the kernel's own mean and rstd, and the unary backward on the
stored y it is handed, so a cancellation error is charged to the figure whose scale is honest
about it."""
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)


def f32r(v):
    """A Python float as the kernels receive it (a C float)."""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------ column statistics
def col_stats_parts(M, C):
    """Row blocks that the wrapper splits M rows into: one per 256 rows, at most 2048 blocks in
    all over the ceil(C/64) column groups, at least one."""
    cb = -(-C // 64)
    return max(1, min(-(-M // 256), max(1, 2048 // cb)))


def col_terms(a, b=None, mode=0, mu=None, rs=None, dtype=F64):
    """The two per-element terms [M, C] whose column sums col_stats takes."""
    a = a.to(dtype)
    if mode == 0:
        return a, a * a
    if mode == 1:
        return a, a * b.to(dtype)
    return a, a * (b.to(dtype) - mu.to(dtype)[:, None]) * rs.to(dtype)[:, None]


def col_stats(a, T, b=None, mode=0, mu=None, rs=None, dtype=F64):
    """(part [T, 2, C], the same sums of the magnitudes of the terms)."""
    s, q = col_terms(a, b, mode, mu, rs, dtype)
    M, C = s.shape
    rpb = -(-M // T)
    part = torch.zeros((T, 2, C), dtype=dtype, device=a.device)
    mag = torch.zeros((T, 2, C), dtype=dtype, device=a.device)
    for t in range(T):
        lo, hi = t * rpb, min(M, (t + 1) * rpb)
        if lo < hi:
            part[t, 0], part[t, 1] = s[lo:hi].sum(0), q[lo:hi].sum(0)
            mag[t, 0], mag[t, 1] = s[lo:hi].abs().sum(0), q[lo:hi].abs().sum(0)
    return part, mag


def col_reduce2(part, old=None, dtype=F64):
    """(o [2, C], scale [2, C]); old: [2, C] that acc = 1 adds onto."""
    p = part.to(dtype)
    o, mag = p.sum(0), part.to(F64).abs().sum(0)
    if old is not None:
        o, mag = o + old.to(dtype), mag + old.to(F64).abs()
    return o, mag


def col_affine(a, c0, b=None, c1=None, c2=None, dtype=F64):
    """a, b [..., C]; c0, c1, c2 [C]."""
    v = a.to(dtype) * c0.to(dtype)
    if b is not None:
        v = v + b.to(dtype) * c1.to(dtype)
    return v if c2 is None else v + c2.to(dtype)


def col_affine_scale(a, c0, b=None, c1=None, c2=None):
    """|a*c0| + |b*c1| + |c2|."""
    v = (a.to(F64) * c0.to(F64)).abs()
    if b is not None:
        v = v + (b.to(F64) * c1.to(F64)).abs()
    return v if c2 is None else v + c2.to(F64).abs()


# ------------------------------------------------------------------ inference-mode BN
def _affine(gamma, beta, like, dtype):
    g = gamma.to(dtype) if gamma is not None else torch.ones_like(like)
    b = beta.to(dtype) if beta is not None else torch.zeros_like(like)
    return g, b


def bn_infer_coef(mm, mv, gamma, beta, eps, dtype=F64):
    mm, mv = mm.to(dtype), mv.to(dtype)
    rstd = 1.0 / torch.sqrt(mv + eps)
    g, b = _affine(gamma, beta, mm, dtype)
    scale = g * rstd
    return {"rstd": rstd, "scale": scale, "shift": b - mm * scale}


def bn_infer_coef_scales(mm, mv, gamma, beta, eps):
    """stats_scales() of tests/batchnorm_oracle.py with the moving statistics, which are inputs
    here, in the place of the sums: A1 -> |mm|, Q -> |mv| (the one rounding of mv + eps is what
    reaches rstd through d rstd / d var)."""
    mm, mv = mm.to(F64), mv.to(F64)
    rstd = 1.0 / torch.sqrt(mv + eps)
    g, b = _affine(gamma, beta, mm, F64)
    s_rstd = rstd * (1 + mv.abs() / (mv + eps))
    s_scale = g.abs() * s_rstd
    return {"rstd": s_rstd, "scale": s_scale, "shift": b.abs() + mm.abs() * g.abs() * rstd + mm.abs() * s_scale}


def bn_infer_bwd(part, mm, rstd, dtype=F64):
    """part [T, 2, C] of (sum g, sum g*x) -> {"dgamma", "dbeta"}."""
    p = part.to(dtype)
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    return {"dgamma": rstd.to(dtype) * (q - mm.to(dtype) * s), "dbeta": s}


def bn_infer_bwd_scales(part, mm, rstd):
    """dbeta: sum_t |part|; dgamma: rstd*(sum_t |sum g*x| + |mm| * sum_t |sum g|), as bwd_scales()
    of tests/batchnorm_oracle.py."""
    p = part.to(F64).abs()
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    return {"dgamma": rstd.to(F64) * (q + mm.to(F64).abs() * s), "dbeta": s}


# ------------------------------------------------------------------ LayerNorm
def ln_stats(x, eps, dtype=F64):
    x = x.to(dtype)
    H = x.shape[1]
    mean = x.sum(1) / H
    var = ((x - mean[:, None]) ** 2).sum(1) / H
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_y(x, mean, rstd, gamma, beta, dtype=F64):
    xh = (x.to(dtype) - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    return xh * gamma.to(dtype) + beta.to(dtype)


def ln_dx(dy, x, mean, rstd, gamma, dtype=F64):
    H = x.shape[1]
    r = rstd.to(dtype)[:, None]
    xh = (x.to(dtype) - mean.to(dtype)[:, None]) * r
    g = dy.to(dtype) * gamma.to(dtype)
    return r * (g - g.sum(1, keepdim=True) / H - xh * ((g * xh).sum(1, keepdim=True) / H))


def ln_dparams(dy, x, mean, rstd, dtype=F64):
    """(dgamma, dbeta)."""
    d = dy.to(dtype)
    xh = (x.to(dtype) - mean.to(dtype)[:, None]) * rstd.to(dtype)[:, None]
    return (d * xh).sum(0), d.sum(0)


def ln_scales(x, dy, mean, rstd, gamma, beta):
    """mean: max_c |x| of the row. rstd: itself. y: |xh*gamma| + |beta|. dx: rstd * max_c
    |dy*gamma| of the row. dgamma, dbeta: sum_r |term|. mean / rstd: the ones y and dx are taken on."""
    x, d, m, r = x.to(F64), dy.to(F64), mean.to(F64), rstd.to(F64)
    g, b = gamma.to(F64), beta.to(F64)
    xh = (x - m[:, None]) * r[:, None]
    return {"mean": x.abs().max(1).values, "rstd": r, "y": (xh * g).abs() + b.abs(),
            "dx": (r * (d * g).abs().max(1).values)[:, None].expand_as(x),
            "dgamma": (d * xh).abs().sum(0), "dbeta": d.abs().sum(0)}


# ------------------------------------------------------------------ embedding
def gather(table, ids):
    """Rows of table [V, H] for ids of any shape; zeros where the id is outside [0, V)."""
    V, H = table.shape
    flat = ids.reshape(-1).to(torch.int64)
    ok = (flat >= 0) & (flat < V)
    out = table[torch.where(ok, flat, torch.zeros_like(flat))].clone()
    out[~ok] = 0
    return out.reshape(tuple(ids.shape) + (H,))


def scatter_add(dy, ids, table0, dtype=F64):
    """(table after the scatter, sum |terms| + |old|): row by row, in row order."""
    V, H = table0.shape
    d = dy.reshape(-1, H).to(dtype)
    out, mag = table0.to(dtype).clone(), table0.to(F64).abs().clone()
    for r, i in enumerate(ids.reshape(-1).tolist()):
        if 0 <= i < V:
            out[i] = out[i] + d[r]
            mag[i] = mag[i] + d[r].to(F64).abs()
    return out, mag


# ------------------------------------------------------------------ unary, reductions, scaling
TANH, SIGMOID = 0, 1


def unary(x, op, dtype=F64):
    x = x.to(dtype)
    return torch.tanh(x) if op == TANH else 1.0 / (1.0 + torch.exp(-x))


def unary_bwd(dy, y, op, dtype=F64):
    d, y = dy.to(dtype), y.to(dtype)
    return d * (1 - y * y) if op == TANH else d * (y * (1 - y))


def unary_bwd_scale(dy, y, op):
    """|dy|*(1 + y^2), or |dy|*|y|*(1 + |y|)."""
    d, y = dy.to(F64).abs(), y.to(F64).abs()
    return d * (1 + y * y) if op == TANH else d * y * (1 + y)


def sum_all(x, scale, dtype=F64):
    """(scale * sum x, |scale| * sum |x|)."""
    return x.to(dtype).sum() * scale, x.to(F64).abs().sum() * abs(scale)


def scaled_fp32(a, g):
    """a * g as one fp32 multiply, then the store's rounding to a's dtype: what fill_scaled and
    row_scale must give by bits."""
    return (a.to(F32) * g.to(F32)).to(a.dtype)


# ------------------------------------------------------------------ GEMM
def gemm(A, B, ta=False, tb=False, bias=None, C0=None, dtype=F64):
    """op(A).op(B) + bias + C0 (C0: the old C that beta = 1 adds; None with beta = 0)."""
    a, b = A.to(dtype), B.to(dtype)
    a = a.transpose(-1, -2) if ta else a
    b = b.transpose(-1, -2) if tb else b
    c = a @ b
    if bias is not None:
        c = c + bias.to(dtype)
    return c if C0 is None else c + C0.to(dtype)


def gemm_scale(A, B, ta=False, tb=False, bias=None, C0=None):
    """sum_k |a||b| + |bias| + |old C|."""
    return gemm(A.to(F64).abs(), B.to(F64).abs(), ta, tb, None if bias is None else bias.abs(),
                None if C0 is None else C0.abs())


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_nn_generic_oracle_cpu.py prints them and asserts the relation).
BARS = {
    #                         scale of the figure                                        fp32
    "cs_part": 4e-6,        # sum_r |term| of the block's rows                           2.0e-7
    "cs_reduce": 2e-6,      # sum_t |part_t| (+ |old| with acc)                          9.6e-8
    "cs_affine": 3e-6,      # |a*c0| + |b*c1| + |c2|; bf16                               1.5e-7
    "bni_rstd": 1e-6,       # rstd*(1 + |mv|/(mv + eps))                                 5.5e-8
    "bni_scale": 2e-6,      # |gamma| * the scale of rstd                                1.1e-7
    "bni_shift": 2e-6,      # |beta| + |mm*gamma|*rstd + |mm| * the scale of `scale`     6.4e-8
    "bni_dgamma": 2e-6,     # rstd*(sum_t |sum g*x| + |mm| * sum_t |sum g|)              1.2e-7
    "bni_dbeta": 2e-6,      # sum_t |sum g|                                              1.1e-7
    "gln_mean": 2e-6,       # max_c |x| of the row                                       9.7e-8
    "gln_rstd": 4e-6,       # rstd                                                       2.3e-7
    "gln_y": 4e-6,          # |xh*gamma| + |beta|; bf16                                  2.0e-7
    "gln_dx": 3e-6,         # rstd * max_c |dy*gamma| of the row; bf16                   1.6e-7
    "gln_dgamma": 3e-6,     # sum_r |dy*xh|                                              1.8e-7
    "gln_dbeta": 2e-6,      # sum_r |dy|                                                 9.9e-8
    "g_scatter": 3e-6,      # sum |terms| + |old|                                        1.4e-7
    "g_tanh": 1e-6,         # |want|; bf16                                               5.6e-8
    "g_sigmoid": 2e-6,      # |want|; bf16                                               1.2e-7
    "g_dtanh": 2e-6,        # |dy|*(1 + y^2); bf16                                       7.3e-8
    "g_dsigmoid": 5e-6,     # |dy|*|y|*(1 + |y|); bf16                                   3.1e-7
    "g_sum": 1e-6,          # |scale| * sum |x|; bf16                                    3.4e-8
    "f32_gemm": 5e-6,       # sum_k |a||b| + |bias| + |old C|                            2.9e-7
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
EPS_BN = 1e-3
CH_MEAN64 = 1  # of every C > 1: 64 + N(0,1). The offset holds its bar at the scale sum x^2 in the
#                float32 oracle (tests/test_nn_generic_oracle_cpu.py checks it), so it is not shrunk.

# (M, C, T): T = None stands for col_stats_parts(M, C), what the wrapper uses
COL_STATS_CASES = [(1, 1, None), (3, 63, None), (5, 64, None), (257, 65, None), (1030, 130, None),
                   (1030, 130, 1),   # one block of 1030 rows
                   (3, 63, 7)]       # blocks 3..6 have no rows
PARTS_VALUES = [((1, 1), 1), ((256, 64), 1), ((257, 64), 2), ((10 ** 6, 64), 2048), ((10 ** 6, 65), 1024),
                ((10 ** 6, 131073), 1)]

REDUCE_T, REDUCE_C = (1, 2, 300), (1, 255, 256, 257)

AFFINE_FORMS = ("c0", "c0_c2", "b_c1", "b_c1_c2")
AFFINE_C = (1, 3, 64, 130)
AFFINE_ROWS = 37                      # n = 37*C: 37, 111, 2368 and 4810, none a multiple of 256
AFFINE_WRAP = (2 ** 24 + 3 * 5, 3)    # n, C (bf16): a second grid-stride trip; n % C = 1, 2^24 % C = 1

BNI_C, BNI_T = (1, 257), (1, 5)

LN_EPS = (1e-12, 1e-5)
LN_CASES = [(1, 1), (1, 5), (2, 3), (63, 4), (64, 5), (65, 77), (100, 77), (1000, 77), (4097, 3), (4097, 77)]  # (H, rows)
ROW_CONST, ROW_OFFSET = 3, 5          # special rows of a case with 77 rows
LN_OFFSET = 100.0                     # ROW_OFFSET is LN_OFFSET + 0.1*N(0,1): holds its bars in float32, not shrunk

EMBED_TABLES = [(1, 1), (50, 24), (7, 130)]  # (V, H)
EMBED_IDS = (torch.int32, torch.int64)
GATHER_WRAP = (7, 130, (331, 390))    # V, H, ids shape: n*H = 129090*130 > 2^24 (bf16)

UNARY_OPS = (TANH, SIGMOID)
UNARY_WRAP = 2 ** 24 + 257

SUM_N = (1, 255, 257, 4096, 4097, 4096 * 1024 + 1)
SUM_BLOCKS = [(1, 1), (4096, 1), (4097, 2), (4096 * 1024, 1024), (10 ** 9, 1024)]
ROW_SCALE_CASES = [(1, 1), (33, 10), (5, 130)]

GEMM_SHAPES = [(1, 1, 1), (1, 1, 0), (33, 31, 1), (64, 64, 16), (65, 63, 17), (31, 130, 2), (133, 77, 201)]
GEMM_ALL_TRANS = [(65, 63, 17), (133, 77, 201)]
GEMM_PAD = 5                          # columns either side of a column slice of a wider tensor
BATCHED_CASES = [(Bt, shape) for Bt in (1, 3) for shape in ((20, 17, 33), (65, 63, 17))]


def gemm_cases():
    """(M, N, K, ta, tb, bias, beta, sliced)."""
    out = []
    for shape in GEMM_SHAPES:
        trans = [(a, b) for a in (False, True) for b in (False, True)] if shape in GEMM_ALL_TRANS else [(False, False)]
        for ta, tb in trans:
            for bias in (False, True):
                for beta in (0, 1):
                    out.append(shape + (ta, tb, bias, beta, False))
            out.append(shape + (ta, tb, True, 1, True))
            out.append(shape + (ta, tb, False, 0, True))
    return out


# ------------------------------------------------------------------ seeded inputs
def col_stats_inputs(M, C, dtype):
    """a, b [M, C] in dtype, mu, rs fp32 [M] (the row statistics of b, as LayerNorm's dgamma uses
    them). Column CH_MEAN64 of a is 64 + N(0,1)."""
    gen = _gen(M, C, 11)
    a = torch.randn(M, C, generator=gen) * 2 + torch.randn(C, generator=gen)
    if C > 1:
        a[:, CH_MEAN64] = 64 + torch.randn(M, generator=gen)
    b = torch.randn(M, C, generator=gen) * 1.5 + 0.5
    a, b = a.to(dtype), b.to(dtype)
    mu, rs = ln_stats(b, f32r(1e-5))
    return {"a": a, "b": b, "mu": mu.float(), "rs": rs.float()}


def reduce_inputs(T, C):
    gen = _gen(T, C, 12)
    return {"part": torch.randn(T, 2, C, generator=gen) * 3 + 1, "old": torch.randn(2, C, generator=gen) * 10}


def affine_inputs(rows, C, dtype):
    gen = _gen(rows, C, 13)
    return {"a": torch.randn(rows, C, generator=gen).to(dtype), "b": torch.randn(rows, C, generator=gen).to(dtype),
            "c0": torch.randn(C, generator=gen), "c1": torch.randn(C, generator=gen),
            "c2": torch.randn(C, generator=gen)}


def affine_wrap_inputs():
    """(inputs with ceil(n/C) rows, n): the kernel takes the first n elements of the flat a and b,
    the last row cut short, and the oracle's result is cut the same way."""
    n, C = AFFINE_WRAP
    return affine_inputs(-(-n // C), C, BF16), n


def affine_args(inp, form):
    """(b, c1, c2) of an AFFINE_FORMS entry."""
    return (inp["b"] if "b" in form else None, inp["c1"] if "b" in form else None,
            inp["c2"] if "c2" in form else None)


def bni_inputs(C, T):
    """Moving statistics (mv = 0 in channel 0: only eps under the root), gamma, beta, and
    partial sums [T, 2, C] for the backward with an rstd to read them with."""
    gen = _gen(C, T, 14)
    mm, mv = torch.randn(C, generator=gen) * 2, torch.rand(C, generator=gen) + 0.1
    mv[0] = 0.0
    return {"mm": mm, "mv": mv, "gamma": torch.rand(C, generator=gen) + 0.5, "beta": torch.randn(C, generator=gen),
            "part": torch.randn(T, 2, C, generator=gen) * 4, "rstd": torch.rand(C, generator=gen) + 0.5}


def ln_inputs(H, rows, dtype):
    """x, dy [rows, H] in dtype; gamma, beta fp32 [H]. With 77 rows, row ROW_CONST is the constant
    0.75 and row ROW_OFFSET is LN_OFFSET + 0.1*N(0,1)."""
    gen = _gen(H, rows, 15)
    x = torch.randn(rows, H, generator=gen) * 1.5 + 0.25
    dy = torch.randn(rows, H, generator=gen)
    gamma = torch.randn(H, generator=gen) * 0.5 + 1
    beta = torch.randn(H, generator=gen) * 0.1
    if rows >= 77:
        x[ROW_CONST] = 0.75
        x[ROW_OFFSET] = LN_OFFSET + 0.1 * torch.randn(H, generator=gen)
    return {"x": x.to(dtype), "dy": dy.to(dtype), "gamma": gamma, "beta": beta}


def out_of_range(V, idtype):
    return [-1, V] + ([2 ** 31 - 1] if idtype == torch.int32 else [2 ** 40])


def embed_inputs(V, H, idtype, dtype, same=False):
    """table [V, H] and dy [3, 7, H] in dtype, ids [3, 7] (the out-of-range values at fixed places
    in the last row; with `same` every other id is V // 2), an old fp32 gradient table."""
    gen = _gen(V, H, 16, int(same), int(idtype == torch.int64))
    shape = (3, 7)
    ids = torch.full(shape, V // 2, dtype=torch.int64) if same else torch.randint(0, V, shape, generator=gen)
    bad = out_of_range(V, idtype)
    ids[2, 1:1 + len(bad)] = torch.tensor(bad)
    return {"table": torch.randn(V, H, generator=gen).to(dtype), "ids": ids.to(idtype),
            "dy": torch.randn(shape + (H,), generator=gen).to(dtype), "old": torch.randn(V, H, generator=gen) * 5}


def unary_inputs(dtype):
    """[-87, 87] in 4096 steps, 2049 points of [-1e-3, 1e-3], the 32 smallest normal bf16 numbers of
    either sign and the bf16 grid from 7 to 10 of either sign (32 steps below 8 and 32 above)."""
    k = torch.arange(32, dtype=F64)
    tiny = 2.0 ** -126 * (1 + k / 128)
    eight = torch.cat([8 - (k + 1) / 32, 8 + k / 16])
    x = torch.cat([torch.linspace(-87, 87, 4096, dtype=F64), torch.linspace(-1e-3, 1e-3, 2049, dtype=F64),
                   tiny, -tiny, eight, -eight])
    return x.to(dtype)


def unary_bwd_inputs(op, dtype):
    """(dy, y): y a grid over the open range of the op's values."""
    gen = _gen(op, 17)
    y = torch.linspace(-0.99, 0.99, 1001) if op == TANH else torch.linspace(0.01, 0.99, 1001)  # open in bf16 too
    return torch.randn(1001, generator=gen).to(dtype), y.to(dtype)


def sum_inputs(n, dtype):
    return (torch.randn(n, generator=_gen(n, 18)) + 0.25).to(dtype)


def row_scale_inputs(rows, C, dtype):
    gen = _gen(rows, C, 19)
    return torch.randn(rows, C, generator=gen).to(dtype), torch.randn(rows, generator=gen)


def _wide(rows, cols, gen, sliced):
    """fp32 [rows, cols]: contiguous, or columns GEMM_PAD.. of a tensor 2*GEMM_PAD wider."""
    if not sliced:
        return torch.randn(rows, cols, generator=gen)
    return torch.randn(rows, cols + 2 * GEMM_PAD, generator=gen)[:, GEMM_PAD:GEMM_PAD + cols]


def gemm_inputs(M, N, K, ta, tb, sliced=False, batch=None):
    """A ([M, K], [K, M] with ta), B ([K, N], [N, K] with tb), bias [N], old C [M, N]; with
    `batch` a leading dimension of that size on A, B and C."""
    gen = _gen(M, N, K, int(ta), int(tb), int(sliced), batch or 0)
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if batch:
        return {"A": torch.randn(batch, *sa, generator=gen), "B": torch.randn(batch, *sb, generator=gen)}
    return {"A": _wide(*sa, gen, sliced), "B": _wide(*sb, gen, sliced), "bias": torch.randn(N, generator=gen),
            "C0": torch.randn(M, N, generator=gen) * 3}
