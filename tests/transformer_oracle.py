"""What tests/test_transformer_rows.py (GPU) and tests/test_transformer_oracle_cpu.py share (a
plain module, imported by them):

* plain statements of the operations of csrc/kernels/transformer.hip, written from their
  definitions and not from the kernels: torch, whole tensors, no tiles, no waves, float64 unless
  `dtype=` says otherwise (the float32 run is how the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.

Definitions (rows r, columns c, H columns; keep_* are the dropout keep masks of
ops.transformer.keep_mask over the flat index r*H + c, all ones when p = 0):

  LayerNorm    s = res + keep_in*x/(1-p_in)                      (res = 0 without a residual)
               mean = sum_c s / H, var = sum_c (s-mean)^2 / H, rstd = 1/sqrt(var+eps)
               xh = (s-mean)*rstd,  y = keep_out*(xh*gamma+beta)/(1-p_out)
  backward     d = keep_out*dy/(1-p_out), g = d*gamma, m1 = sum_c g / H, m2 = sum_c g*xh / H
               ds = rstd*(g - m1 - xh*m2), dx = keep_in*ds/(1-p_in)
               dgamma = sum_r d*xh, dbeta = sum_r d              (+ the old value: accumulate)
  embedding    s[r] = word[ids[r]] + pos[r % S] + type[tt[r]]    (tt = 0 without token types)
               dword[i] += sum_{ids[r]=i} ds[r]; dpos[p] = pos_beta*dpos[p] + sum_b ds[b*S+p];
               dtype[t] = sum_{tt[r]=t} ds[r]
  gather       out[r] = src[idx[r] + (r // per)*gs]              (idx = 0 without an index)
  scatter      dst[idx[r] + (r // per)*gs] (+)= src[r]
  count        n = max(1, #labels >= 0): scale/n, or (1/n, scale/n)
  xent         over the first V of ld columns, rows with label < 0 ignored:
               loss_r = max_r + log(sum_c exp(z-max_r)) - z[label]
               grad = gsc*(softmax(z) - onehot(label)), 0 in ignored rows and columns >= V
               correct_r = no z_c > z[label];  sums += msc * (sum_r loss_r, sum_r correct_r)
  dact         0: dy * d/dx [x/2 * (1 + tanh(k0*(x + k1*x^3)))], k0 = sqrt(2/pi), k1 = 0.044715
               1: dy * (1 - a^2), a the tanh output

The kernels round s to bf16 before they take its statistics, so the comparisons take mean, rstd,
y and the backward from the bf16 s (the kernel's own on the GPU, the rounded reference on the
CPU), after s itself is checked: within one bf16 ulp of the reference, plus the `ln_s` bar times
|res| + |x|/(1-p_in) for the fp32 product and sum before the store (where the two terms cancel,
their fp32 rounding is more than an ulp of the small result).

Figures. Every comparison is element-wise: figure = max |got - want| / scale, where for a bf16
output half a bf16 ulp of `want` (the store's rounding; between 2^-9 and 2^-8 of |want|) is taken
off the error first, and the scale is the magnitude the fp32 arithmetic before the store works
at (listed beside BARS, which holds the bar of every figure)."""
import math

import numpy as np
import torch

from tensorflow_train_distributed_amd.ops import transformer as T

F64 = torch.float64
K0, K1 = 0.7978845608028654, 0.044715


# ------------------------------------------------------------------ helpers
def bf16_half_ulp(want):
    """Half a bf16 ulp (8 significant bits) at each float64 value."""
    _, e = torch.frexp(want.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(want), e - 9)


def figure(got, want, scale, bf16_store=False, ulps=0.5):
    """max |got - want| / scale over the elements; bf16_store takes the store's half ulp (`ulps`
    bf16 ulps) off the error first."""
    want = want.to(F64)
    err = (got.to(F64) - want).abs()
    if bf16_store:
        err = (err - 2 * ulps * bf16_half_ulp(want)).clamp_min(0)
    if not torch.is_tensor(scale):
        scale = torch.tensor(float(scale), dtype=F64, device=err.device)
    fig = err / scale.to(F64).clamp_min(1e-300)
    return float(fig.max()) if fig.numel() else 0.0


def keep(seed, step, site, p, rows, H, device="cpu"):
    """The keep mask [rows, H] of a dropout site as a bool tensor (all True when p = 0)."""
    if p <= 0:
        return torch.ones((rows, H), dtype=torch.bool, device=device)
    idx = np.arange(rows * H, dtype=np.int64)
    return torch.from_numpy(T.keep_mask(seed, step, site, p, idx).reshape(rows, H)).to(device)


# ------------------------------------------------------------------ LayerNorm
def ln_s(x, res, keep_in, p_in, dtype=F64):
    s = keep_in.to(dtype) * x.to(dtype) / (1.0 - p_in)
    return s if res is None else res.to(dtype) + s


def ln_s_scale(x, res, p_in):
    a = x.to(F64).abs() / (1.0 - p_in)
    return a if res is None else a + res.to(F64).abs()


def ln_stats(s, eps, dtype=F64):
    s = s.to(dtype)
    H = s.shape[1]
    mean = s.sum(1) / H
    var = ((s - mean[:, None]) ** 2).sum(1) / H
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_y(s, mean, rstd, gamma, beta, keep_out, p_out, dtype=F64):
    xh = (s.to(dtype) - mean[:, None]) * rstd[:, None]
    return keep_out.to(dtype) * (xh * gamma.to(dtype) + beta.to(dtype)) / (1.0 - p_out)


def ln_bwd(dy, s, mean, rstd, gamma, keep_in, p_in, keep_out, p_out, dtype=F64):
    """(ds, dx, dgamma, dbeta) by the formulas above (no autograd)."""
    H = s.shape[1]
    d = keep_out.to(dtype) * dy.to(dtype) / (1.0 - p_out)
    xh = (s.to(dtype) - mean[:, None]) * rstd[:, None]
    g = d * gamma.to(dtype)
    m1 = g.sum(1) / H
    m2 = (g * xh).sum(1) / H
    ds = rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    dx = keep_in.to(dtype) * ds / (1.0 - p_in)
    return ds, dx, (d * xh).sum(0), d.sum(0)


# ------------------------------------------------------------------ embeddings
def embed_fwd(ids, tt, word, pos, typ, S, dtype=F64):
    rows = ids.numel()
    p = torch.arange(rows, device=ids.device) % S
    t = tt.long() if tt is not None else torch.zeros(rows, dtype=torch.long, device=ids.device)
    return word.to(dtype)[ids.long()] + pos.to(dtype)[p] + typ.to(dtype)[t]


def embed_bwd(ds, ids, tt, dword0, dpos0, T_, B, S, pos_beta, dtype=F64):
    """(dword, dpos, dtype-table gradient [T_, H]); dword0 / dpos0: the buffers' old contents.
    Row by row, in row order (no index_add_, no view tricks)."""
    ds = ds.to(dtype)
    H = ds.shape[1]
    dword = dword0.to(dtype).clone()
    dpos = dpos0.to(dtype).clone() if pos_beta else torch.zeros((S, H), dtype=dtype, device=ds.device)
    dtyp = torch.zeros((T_, H), dtype=dtype, device=ds.device)
    idl = ids.tolist()
    ttl = tt.tolist() if tt is not None else [0] * len(idl)
    for r in range(B * S):
        dword[idl[r]] += ds[r]
        dpos[r % S] += ds[r]
        dtyp[ttl[r]] += ds[r]
    return dword, dpos, dtyp


def embed_bwd_abs(ds, ids, tt, dword0, dpos0, T_, B, S, pos_beta):
    """sum |terms| of each embed_bwd output: the scale of its figure."""
    return embed_bwd(ds.to(F64).abs(), ids, tt, dword0.to(F64).abs(), dpos0.to(F64).abs(), T_, B, S, pos_beta)


# ------------------------------------------------------------------ gather / scatter
def _targets(idx, n, group, device):
    per, gs = group
    base = idx.long() if idx is not None else torch.zeros(n, dtype=torch.long, device=device)
    return base + (torch.arange(n, device=device) // per) * gs


def gather_rows(src, idx, group=(1, 0), n=None):
    n = idx.numel() if idx is not None else n
    return src[_targets(idx, n, group, src.device)].clone()


def scatter_rows(src, idx, dst0, accumulate=False, group=(1, 0), dtype=F64):
    """dst after the scatter, in `dtype` (targets distinct)."""
    to = _targets(idx, src.shape[0], group, src.device)
    assert to.unique().numel() == to.numel()
    dst = dst0.to(dtype).clone()
    for r, t in enumerate(to.tolist()):
        dst[t] = dst[t] + src[r].to(dtype) if accumulate else src[r].to(dtype)
    return dst


# ------------------------------------------------------------------ count, xent, activations
def count_valid(labels, scale, both=False):
    n = max(1, int((labels >= 0).sum()))
    return (1.0 / n, scale / n) if both else (scale / n,)


def xent(logits, V, labels, gsc, msc=1.0, dtype=F64):
    """(loss [rows], correct [rows], grad [rows, ld], sums-increment (2,)): loss / correct 0 in
    ignored rows."""
    rows, ld = logits.shape
    z = logits[:, :V].to(dtype)
    lab = labels.long()
    valid = lab >= 0
    safe = lab.clamp_min(0)
    mx = z.max(1).values
    e = torch.exp(z - mx[:, None])
    se = e.sum(1)
    zt = z.gather(1, safe[:, None])[:, 0]
    loss = torch.where(valid, mx + torch.log(se) - zt, torch.zeros_like(mx))
    correct = torch.where(valid & ((z > zt[:, None]).sum(1) == 0), torch.ones_like(mx), torch.zeros_like(mx))
    grad = torch.zeros((rows, ld), dtype=dtype, device=logits.device)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(rows, device=logits.device), safe] = 1
    grad[:, :V] = torch.where(valid[:, None], gsc * (e / se[:, None] - onehot), torch.zeros_like(z))
    return loss, correct, grad, (float(loss.to(F64).sum()) * msc, float(correct.sum()) * msc)


def dgelu(x, dtype=F64):
    x = x.to(dtype)
    t = torch.tanh(K0 * (x + K1 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * K0 * (1 + 3 * K1 * x * x)


def dact(dy, aux, kind, dtype=F64):
    a = aux.to(dtype)
    return dy.to(dtype) * (dgelu(a, dtype) if kind == 0 else 1 - a * a)


def tanh(x, dtype=F64):
    return torch.tanh(x.to(dtype))


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_transformer_oracle_cpu.py prints them and asserts the relation); 2^-24,
# one fp32 rounding, is the floor because torch's pairwise sums of a few hundred terms land below
# what any single fp32 operation may lose. MARGIN = 16 is the order of magnitude the optimizer
# tests allow: a wave tree, a fixed-order block reduce or atomics sum in another order than torch
# does, and __expf / __logf / rsqrtf / tanhf are not correctly rounded.
MARGIN = 16.0
FLOOR = 2.0 ** -24
BARS = {
    #                      scale of the figure                                   fp32
    "ln_s": 3e-6,        # |res| + |x|/(1-p_in); bf16, one whole ulp taken off   1.3e-7
    "ln_mean": 1e-6,     # max_c |s| of the row                                  2.5e-8
    "ln_rstd": 3e-6,     # rstd                                                  1.7e-7
    "ln_y": 5e-6,        # (|xh*gamma| + |beta|)/(1-p_out); bf16                 2.7e-7
    "ln_ds": 4e-6,       # rstd * max_c |d*gamma| of the row; bf16               2.4e-7
    "ln_dx": 4e-6,       # the same / (1-p_in); bf16                             2.4e-7
    "ln_dgamma": 3e-6,   # sum_r |d*xh| (+ |old|)                                1.6e-7
    "ln_dbeta": 1e-6,    # sum_r |d| (+ |old|)                                   6.2e-8
    "emb_s": 2e-6,       # |word| + |pos| + |type|; bf16                         7.9e-8
    "emb_dword": 2e-6,   # sum |terms| + |old|                                   8.8e-8
    "emb_dpos": 2e-6,    # sum |terms| (+ |old|)                                 7.8e-8
    "emb_dtype": 1e-6,   # sum |terms|                                           1.7e-8
    "scatter": 1e-6,     # |dst| + |src|; bf16 (accumulate)                      0
    "count": 1e-6,       # the value                                             5.0e-8
    "xent_grad": 2e-6,   # |gsc|; bf16                                           1.0e-7
    "xent_loss": 1e-6,   # msc * sum_r (|max| + |log se| + |z_label|)            4.8e-8
    "xent_correct": 1e-6,  # msc * valid rows                                    0
    "dact": 9e-6,        # |dy|; bf16                                            5.0e-7
    "tanh": 1e-6,        # 1; bf16                                               3.0e-8
}


def bar_holds(name, fp32_max):
    """The relation between a measured float32 maximum and the bar of its figure."""
    return MARGIN * max(fp32_max, FLOOR) <= BARS[name]


SEED, STEP = 7, 0          # RngState(SEED) before any advance()
SITE_IN, SITE_OUT = 11, 12
GUARD = 16                 # guard rows / elements on either side of an output
ROW_CONST, ROW_OFFSET = 3, 5   # special rows of a LayerNorm case with at least 77 rows

# mode -> (residual, p_in, p_out, eps)
LN_MODES = {
    "plain": (False, 0.0, 0.0, 1e-12),
    "both": (True, 0.1, 0.2, 1e-5),
    "embed": (False, 0.0, 0.1, 1e-12),      # the embedding LayerNorm of the engine
    "layer": (True, 0.1, 0.0, 1e-5),        # its two per-layer sites
    "res_nodrop": (True, 0.0, 0.0, 1e-12),  # s = x + res exactly
}
LN_GRID = [(m, H, rows) for m in ("plain", "both") for H in (512, 1024, 1536, 2048, 4096) for rows in (1, 77, 4097)]
LN_ENGINE = [(m, H, rows) for m in ("embed", "layer") for H in (512, 1024) for rows in (77, 4097)]
LN_EXTRA = [("res_nodrop", 1024, 77)]
LN_PREFETCH0 = [("both", 1024, rows) for rows in (9, 77, 4097)]

XENT_CASES = [(5, 8), (1000, 1024), (2048, 2048), (2049, 2056), (30522, 30528)]
XENT_ROWS = 7
COUNT_N = (1, 255, 256, 257, 5000)

EMBED_H = (128, 512, 768, 1024, 1536, 2048)
EMBED_B, EMBED_S, EMBED_V = 9, 129, 300

GATHER_H = (8, 128, 520, 1024)
GATHER_N = (1, 5, 13)

DACT_N8 = (1, 255, 257)
TANH_N = (1, 1001)


def _gen(*key):
    return torch.Generator().manual_seed(1234 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


# ------------------------------------------------------------------ LayerNorm inputs and figures
def ln_inputs(mode, H, rows):
    """CPU tensors of a LayerNorm case: x, res (or None), dy bf16 [rows, H]; gamma, beta fp32 [H].
    With at least 77 rows, row ROW_CONST of s is the constant 0.75 and row ROW_OFFSET is
    100 + 0.1*N(0,1) (through the residual where there is one, x = 0 there, so that an input
    dropout leaves them alone)."""
    residual = LN_MODES[mode][0]
    gen = _gen(list(LN_MODES).index(mode), H, rows)
    x = torch.randn(rows, H, generator=gen).bfloat16()
    res = torch.randn(rows, H, generator=gen).bfloat16() if residual else None
    dy = torch.randn(rows, H, generator=gen).bfloat16()
    gamma = torch.randn(H, generator=gen) * 0.5 + 1
    beta = torch.randn(H, generator=gen) * 0.1
    if rows >= 77:
        special = res if residual else x
        special[ROW_CONST] = 0.75
        special[ROW_OFFSET] = (100 + 0.1 * torch.randn(H, generator=gen)).bfloat16()
        if residual:
            x[ROW_CONST] = 0
            x[ROW_OFFSET] = 0
    return {"x": x, "res": res, "dy": dy, "gamma": gamma, "beta": beta}


def ln_masks(mode, H, rows, device="cpu"):
    _, p_in, p_out, _ = LN_MODES[mode]
    return (keep(SEED, STEP, SITE_IN, p_in, rows, H, device), keep(SEED, STEP, SITE_OUT, p_out, rows, H, device))


def ln_reference(mode, inp, kin, kout, s, stats=None, dg0=None, db0=None, dtype=F64):
    """Everything after s, in `dtype`: mean and rstd from the bf16 `s`; y and the backward from `s`
    and the fp32 statistics `stats` = (mean, rstd) that the backward kernel is handed (the forward
    kernel's own on the GPU, which are checked first; None: the ones computed here). dg0 / db0: old
    dgamma / dbeta that the backward accumulates onto."""
    _, p_in, p_out, eps = LN_MODES[mode]
    mean, rstd = ln_stats(s, eps, dtype)
    m, r = (mean, rstd) if stats is None else (stats[0].to(dtype), stats[1].to(dtype))
    y = ln_y(s, m, r, inp["gamma"], inp["beta"], kout, p_out, dtype)
    ds, dx, dg, db = ln_bwd(inp["dy"], s, m, r, inp["gamma"], kin, p_in, kout, p_out, dtype)
    if dg0 is not None:
        dg, db = dg + dg0.to(dtype), db + db0.to(dtype)
    return {"mean": mean, "rstd": rstd, "y": y, "ds": ds, "dx": dx, "dgamma": dg, "dbeta": db}


def ln_scales(mode, inp, kout, s, ref, stats=None, dg0=None, db0=None):
    """The scale of each LayerNorm figure, from the float64 reference `ref`."""
    _, p_in, p_out, _ = LN_MODES[mode]
    s = s.to(F64)
    m, r = (ref["mean"], ref["rstd"]) if stats is None else (stats[0].to(F64), stats[1].to(F64))
    gamma, beta = inp["gamma"].to(F64), inp["beta"].to(F64)
    d = kout.to(F64) * inp["dy"].to(F64) / (1.0 - p_out)
    xh = (s - m[:, None]) * r[:, None]
    row = r * (d * gamma).abs().max(1).values
    sg, sb = (d * xh).abs().sum(0), d.abs().sum(0)
    if dg0 is not None:
        sg, sb = sg + dg0.to(F64).abs(), sb + db0.to(F64).abs()
    return {"mean": s.abs().max(1).values, "rstd": ref["rstd"],
            "y": ((xh * gamma).abs() + beta.abs()) / (1.0 - p_out),
            "ds": row[:, None], "dx": row[:, None] / (1.0 - p_in), "dgamma": sg, "dbeta": sb}


LN_BF16 = ("y", "ds", "dx")


def ln_figures(got, ref, scales):
    """{figure name: value} of LayerNorm results `got` (a dict like ln_reference's, any subset)."""
    return {"ln_" + k: figure(v, ref[k], scales[k], bf16_store=k in LN_BF16 and v.dtype == torch.bfloat16)
            for k, v in got.items() if v is not None}


def check(figs, label=""):
    bad = {k: v for k, v in figs.items() if not v <= BARS[k]}
    assert not bad, (label, bad, {k: BARS[k] for k in bad})
    return figs


# ------------------------------------------------------------------ the other inputs
def xent_inputs(V, ld):
    """bf16 logits [7, ld] (columns >= V hold noise the kernel must not read into the loss) and
    int32 labels: row 0 label 0, row 1 label V-1, row 2 ignored, row 3 a tie on the maximum at the
    label, row 4 logits spread to +-80."""
    gen = _gen(V, ld)
    z = (torch.randn(XENT_ROWS, ld, generator=gen) * 3)
    z[:, V:] = 50 + 10 * torch.randn(XENT_ROWS, ld - V, generator=gen)
    z[4, :V] = torch.linspace(-80, 80, V)[torch.randperm(V, generator=gen)]
    z = z.bfloat16()
    labels = torch.randint(0, V, (XENT_ROWS,), generator=gen, dtype=torch.int32)
    labels[0], labels[1], labels[2] = 0, V - 1, -1
    top = float(z[3, :V].float().max()) + 1
    z[3, int(labels[3])] = top
    z[3, (int(labels[3]) + V // 2) % V if V > 1 else 0] = top  # the same value elsewhere: a tie
    return z, labels


def xent_scales(logits, V, labels, msc):
    z = logits[:, :V].to(F64)
    lab = labels.long()
    valid = lab >= 0
    mx = z.max(1).values
    se = torch.exp(z - mx[:, None]).sum(1)
    zt = z.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    return float(((mx.abs() + torch.log(se).abs() + zt.abs()) * valid).sum()) * msc, float(valid.sum()) * msc


def embed_inputs(H, T_, same_ids=False, with_tt=True):
    gen = _gen(H, T_, int(same_ids), int(with_tt))
    B, S, V = EMBED_B, EMBED_S, EMBED_V
    rows = B * S
    return {
        "word": torch.randn(V, H, generator=gen).bfloat16(), "pos": torch.randn(S, H, generator=gen).bfloat16(),
        "typ": torch.randn(T_, H, generator=gen).bfloat16(),
        # ids 0..V-3 only: rows V-2 and V-1 of dword are never named
        "ids": (torch.full((rows,), 17, dtype=torch.int32) if same_ids
                else torch.randint(0, V - 2, (rows,), generator=gen, dtype=torch.int32)),
        "tt": torch.randint(0, T_, (rows,), generator=gen, dtype=torch.int32) if with_tt else None,
        "ds": torch.randn(rows, H, generator=gen).bfloat16(),
        "dword0": torch.randn(V, H, generator=gen), "dpos0": torch.randn(S, H, generator=gen),
    }


def act_inputs(n):
    """bf16 [n] values that include 0, +-10 and the bf16 grid around +-1, and a bf16 dy."""
    gen = _gen(n, 3)
    grid = torch.tensor([0.0, 10.0, -10.0, 1.0, -1.0, 1 - 2.0 ** -8, 1 + 2.0 ** -7, -1 + 2.0 ** -8, -1 - 2.0 ** -7,
                         1 - 2.0 ** -7, 1 + 2.0 ** -6, -1 + 2.0 ** -7, -1 - 2.0 ** -6, 3.0, -3.0, 0.5])
    x = torch.randn(n, generator=gen) * 2
    k = min(n, grid.numel())
    x[:k] = grid[:k]
    return x.bfloat16(), torch.randn(n, generator=gen).bfloat16()


def tanh_outputs(n):
    """bf16 tanh outputs (the aux of dact kind 1): in [-1, 1], the grid values included."""
    x, dy = act_inputs(n)
    return torch.tanh(x.float()).bfloat16(), dy


assert math.isclose(K0, math.sqrt(2 / math.pi), rel_tol=1e-15)
