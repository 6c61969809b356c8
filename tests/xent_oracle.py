"""What tests/test_xent_kernels.py (GPU) and tests/test_xent_oracle_cpu.py share (a plain module,
imported by them):

* plain statements of ttdk_sparse_xent (csrc/kernels/xent.hip) and ttdk_in_top_k
  (csrc/kernels/nn_generic.hip), written from the definitions below and not from the kernels:
  torch, whole tensors, no blocks, no lanes, float64 unless `dtype=` says otherwise (the float32
  run is how the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.
  figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and check() are those of
  tests/transformer_oracle.py; BARS below is entered into its table so that they see it.

Definitions (rows of V logits z, label l):

  loss     max + log(sum exp(z - max)) - z[l]
  grad     grad_scale * (softmax(z) - onehot(l))
  correct  [0 <= l < V and z[l] finite and no z_c > z[l]]
  sums     (mean loss, mean correct) over all rows
  a label outside [0, V): the row's loss is NaN, correct 0, sums[0] NaN; the row's gradient is not
  compared (only that nothing outside the row was written)
  in_top_k correct iff the target is valid, its logit finite and fewer than k logits are strictly
           greater than it

correct and in_top_k are integer results: compared exactly, no bar. sums[1] is a count over
`rows`: it is held to one fp32 rounding, |got - count/rows| <= 2^-24.

Figures. Every comparison is element-wise: figure = max |got - want| / scale over the elements
whose `want` is finite; where `want` is +-inf or NaN, got must be the same (finite_figure()). For a
bf16 gradient half a bf16 ulp of `want` is taken off the error first. The scales are written out
beside BARS. The float32 run uses the same definitions with dtype=torch.float32; no formula had to
be changed for it."""
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
NEG_INF = float("-inf")


# ------------------------------------------------------------------ the operations
def xent(z, labels, grad_scale, dtype=F64):
    """{"loss" [rows], "grad" [rows, V], "correct" bool [rows], "sums" (mean loss, mean correct),
    "valid" bool [rows], "loss_scale" [rows]: |max| + |log se| + |z_l|, "sum_scale": its mean}."""
    rows, V = z.shape
    z = z.to(dtype)
    lab = labels.long()
    ok = (lab >= 0) & (lab < V)
    safe = lab.clamp(0, V - 1)
    mx = z.max(1).values
    e = torch.exp(z - mx[:, None])
    se = e.sum(1)
    zt = z.gather(1, safe[:, None])[:, 0]
    nan = torch.full_like(mx, float("nan"))
    loss = torch.where(ok, mx + torch.log(se) - zt, nan)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(rows, device=z.device), safe] = 1
    grad = grad_scale * (e / se[:, None] - onehot)
    correct = ok & torch.isfinite(zt) & ((z > zt[:, None]).sum(1) == 0)
    lscale = (mx.abs() + torch.log(se).abs() + zt.abs()).to(F64)
    return {"loss": loss, "grad": grad, "correct": correct, "valid": ok, "loss_scale": lscale,
            "sums": (loss.sum() / rows, correct.to(dtype).sum() / rows),
            "sum_scale": torch.where(torch.isfinite(lscale), lscale, torch.zeros_like(lscale)).sum() / rows}


def in_top_k(z, targets, k):
    """bool [rows]."""
    V = z.shape[1]
    z = z.to(F64)
    t = targets.long()
    ok = (t >= 0) & (t < V)
    zt = z.gather(1, t.clamp(0, V - 1)[:, None])[:, 0]
    return ok & torch.isfinite(zt) & ((z > zt[:, None]).sum(1) < k)


def finite_figure(got, want, scale, bf16_store=False):
    """figure() over the elements whose `want` is finite; the others must agree as they are
    (+inf with +inf, NaN with NaN). Returns (figure, whether they do)."""
    want = want.to(F64)
    got = got.to(F64)
    fin = torch.isfinite(want)
    same = bool((torch.isnan(want[~fin]) == torch.isnan(got[~fin])).all()) and \
        bool((torch.isnan(want[~fin]) | (want[~fin] == got[~fin])).all())
    if not torch.is_tensor(scale):
        scale = torch.full_like(want, float(scale))
    scale = scale.to(F64).expand_as(want)
    return figure(got[fin], want[fin], scale[fin], bf16_store=bf16_store), same


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_xent_oracle_cpu.py prints them and asserts the relation).
BARS = {
    #                        scale of the figure                                         fp32
    "sx_grad": 6e-6,       # |grad_scale|; bf16                                          3.4e-7
    "sx_loss": 3e-6,       # |max| + |log se| + |z_l| of the row                         1.8e-7
    "sx_mean_loss": 2e-6,  # the mean of that over the rows                              7.0e-8
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
XENT_V = (1, 2, 10, 63, 64, 65, 255, 256, 257, 1000, 1001, 4099)
XENT_ROWS = (1, 7, 300)   # 300: the sums kernel takes a second trip of its 256-thread loop
XENT_DTYPES = (F32, BF16)
XENT_LABELS = (torch.int32, torch.int64)


def grad_scales(rows):
    return (1.0, 1.0 / rows, 128.0 / rows)


# the planted rows: row i of a case with at least 7 rows holds PLANTS[i]; a case of one row holds
# PLANTS[V % 7]
PLANTS = ("label_first", "label_last", "tie_at_label", "tie_elsewhere", "spread", "neginf_target", "large_equal")
ROW_NEGINF = PLANTS.index("neginf_target")

TOPK_V = (1, 63, 64, 65, 1000)
TOPK_ROWS = (1, 4, 5, 9)   # the kernel takes four rows per block
TOPK_K = (1, 2, 5)


# ------------------------------------------------------------------ seeded inputs
def _plant(z, row, kind, V, gen):
    """Writes the plant into z[row] (float32, before the rounding to the logits' dtype) and returns
    the row's label."""
    lab = int(torch.randint(0, V, (1,), generator=gen))
    top = float(z[row].max()) + 1
    if kind == "label_first":
        return 0
    if kind == "label_last":
        return V - 1
    if kind == "tie_at_label":          # correct: nothing is strictly greater
        z[row, lab] = top
        z[row, (lab + V // 2) % V] = top
    elif kind == "tie_elsewhere":       # not correct (V > 1): the label lies below a tied maximum
        if V >= 3:
            z[row, 0], z[row, V - 1], lab = top, top, V // 2
            z[row, lab] = top - 1
        elif V == 2:
            z[row, 0], lab = top, 1
    elif kind == "spread":
        z[row] = torch.linspace(-80, 80, V)[torch.randperm(V, generator=gen)]
    elif kind == "neginf_target":       # loss +inf, not correct (V = 1: left alone, no finite logit would remain)
        if V > 1:
            z[row, lab] = NEG_INF
    elif kind == "large_equal":         # softmax 1/V everywhere, loss log V, correct
        z[row] = 32768.0
    return lab


def xent_inputs(V, rows, dtype):
    """(logits [rows, V] in `dtype`, labels int64 [rows]) on the CPU: 3*N(0,1) with the planted
    rows."""
    gen = _gen(V, rows, 11)
    z = torch.randn(rows, V, generator=gen) * 3
    labels = torch.randint(0, V, (rows,), generator=gen)
    if rows >= len(PLANTS):
        for i, kind in enumerate(PLANTS):
            labels[i] = _plant(z, i, kind, V, gen)
    else:
        labels[0] = _plant(z, 0, PLANTS[V % len(PLANTS)], V, gen)
    return z.to(dtype), labels


def finite_labels(z, labels):
    """The labels with every one that names a -inf logit moved to the row's largest logit: the
    variant of a case whose mean loss is finite."""
    zt = z.float().gather(1, labels[:, None])[:, 0]
    return torch.where(torch.isinf(zt), z.float().argmax(1), labels)


def bad_label_inputs(V, dtype):
    """A case of its own: 7 rows, row 2 labelled -1 and row 5 labelled V."""
    gen = _gen(V, 13)
    z = (torch.randn(7, V, generator=gen) * 3).to(dtype)
    labels = torch.randint(0, V, (7,), generator=gen)
    labels[2], labels[5] = -1, V
    return z, labels


def topk_inputs(V, rows, dtype):
    """(z [rows, V] in `dtype`, targets int64 [rows]): values in steps of 1/2 (ties everywhere);
    by row % 5: 1 the target's logit -inf, 2 +inf, 3 NaN (all where V > 1), 4 the row's largest."""
    gen = _gen(V, rows, 12)
    z = (torch.randn(rows, V, generator=gen) * 2).round() / 2
    t = torch.randint(0, V, (rows,), generator=gen)
    for r in range(rows):
        kind = r % 5
        if V > 1 and kind in (1, 2, 3):
            z[r, t[r]] = (NEG_INF, float("inf"), float("nan"))[kind - 1]
        elif kind == 4:
            t[r] = int(z[r].argmax())
    return z.to(dtype), t
