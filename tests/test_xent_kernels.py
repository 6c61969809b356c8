"""ttdk_sparse_xent (csrc/kernels/xent.hip: per-row loss, gradient, top-1 correctness and the
fixed-order batch means) and ttdk_in_top_k (csrc/kernels/nn_generic.hip) against the float64
statements of tests/xent_oracle.py: fp32 and bf16 logits, int32 and int64 labels, V from 1 to 4099
on either side of the wave and block sizes, 1, 7 and 300 rows, three gradient scales, every
combination of outputs the entry point allows, and planted rows (labels at both ends, ties at and
beside the label, logits over +-80, a -inf target logit, large equal logits, labels out of range).

correct and in_top_k are compared exactly. The gradient, the per-row loss and the mean loss are
compared element-wise, |got - want| <= half a bf16 ulp of want (a bf16 gradient only: the store)
+ bar * scale; where the oracle is +inf or NaN the kernel must be too. A bar is 16 x the largest
value the same figure takes when the oracle itself runs in float32 (tests/test_xent_oracle_cpu.py),
never less than 16 x 2^-24. The mean of `correct` is a count: held to 2^-24. Outputs sit between
guard rows of a fixed byte pattern that must survive, and start out as the pattern.

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure          MI355X     fp32      bar
  sx_grad         2.3e-7     3.4e-7    6e-6
  sx_loss         2.7e-7     1.8e-7    3e-6
  sx_mean_loss    7.1e-8     7.0e-8    2e-6
  mean correct    6.0e-8     -         2^-24 (not a bar: the count divided by rows, one fp32 rounding)
"""
import functools

import numpy as np
import pytest
import torch

import xent_oracle as O
import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd.ops import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
PATTERN = 0x5A
DT = {F32: 0, BF16: 1}
LT = {torch.int32: 0, torch.int64: 1}
ONE_ROUNDING = 2.0 ** -24

_seen = {}


def _check(figs, label):
    for k, v in figs.items():
        _seen[k] = max(_seen.get(k, 0.0), v)
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    return O.check(figs, label)


class Guarded:
    """A tensor `t` of `shape` with O.GUARD rows (elements of a 1-D shape) of the byte PATTERN on
    either side in one allocation; `t` starts out as the pattern too, so what a kernel leaves
    unwritten shows."""

    def __init__(self, shape, dtype):
        shape = tuple(shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.n = int(np.prod(shape)) * item
        self.g = O.GUARD * (int(np.prod(shape[1:])) if len(shape) > 1 else 1) * item
        self.g = (self.g + 15) // 16 * 16  # keep `t` 16-byte aligned
        self.raw = torch.full((2 * self.g + self.n,), PATTERN, dtype=U8, device=DEV)
        self.t = self.raw[self.g:self.g + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())


def _bits(t):
    t = t.contiguous()
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def f32r(v):
    """A Python float as the kernel receives it (a C float)."""
    return float(torch.tensor(v, dtype=F32))


OUTPUTS = ("loss_rows", "dlogits", "correct", "sums", "part")


def _run(z, labels, gs, absent=()):
    """One call of ttdk_sparse_xent with every output guarded; `absent` outputs are passed as null
    (their buffers must then stay untouched)."""
    rows, V = z.shape
    bufs = {"loss_rows": Guarded((rows,), F32), "dlogits": Guarded((rows, V), z.dtype), "correct": Guarded((rows,), U8),
            "sums": Guarded((2,), F32), "part": Guarded((2 * rows,), F32)}
    ptr = {k: (None if k in absent else b.t.data_ptr()) for k, b in bufs.items()}
    _lib.call("ttdk_sparse_xent", z.data_ptr(), DT[z.dtype], labels.data_ptr(), LT[labels.dtype], rows, V, float(gs),
              ptr["loss_rows"], ptr["dlogits"], ptr["correct"], ptr["sums"], ptr["part"], _lib.stream())
    for k, b in bufs.items():
        assert b.intact(), k
        if k in absent or (k == "part" and "sums" in absent):  # the row terms are only written for the sums
            assert b.untouched(), k
    return {k: b.t for k, b in bufs.items()}


@functools.lru_cache(maxsize=4)
def _case(V, rows, dtype):
    """The inputs and the float64 reference at grad_scale 1 (the gradient is linear in it), computed
    once on the CPU and shared; also the variant whose labels avoid the -inf logit."""
    z, labels = O.xent_inputs(V, rows, dtype)
    fin = O.finite_labels(z, labels)

    def dev(d):  # tensors to the GPU, the pair of means as Python floats
        return {k: (v.to(DEV) if torch.is_tensor(v) else tuple(float(s) for s in v)) for k, v in d.items()}

    return z.to(DEV), labels.to(DEV), fin.to(DEV), dev(O.xent(z, labels, 1.0)), dev(O.xent(z, fin, 1.0))


def _row_figures(out, ref, gs, bf16, rows_mask=None):
    """sx_grad and sx_loss of one call against the reference at scale 1; correct exactly."""
    gs = f32r(gs)
    sel = slice(None) if rows_mask is None else rows_mask
    g, _ = O.finite_figure(out["dlogits"][sel], gs * ref["grad"][sel], abs(gs), bf16_store=bf16)
    loss, same = O.finite_figure(out["loss_rows"], ref["loss"], ref["loss_scale"])
    assert same, (out["loss_rows"], ref["loss"])
    assert torch.equal(out["correct"], ref["correct"].to(U8))
    return {"sx_grad": g, "sx_loss": loss}


def _mean_correct_ok(got, ref):
    return abs(float(got) - ref["sums"][1]) <= ONE_ROUNDING


@pytest.mark.parametrize("V", O.XENT_V)
@pytest.mark.parametrize("dtype", O.XENT_DTYPES, ids=("fp32", "bf16"))
def test_sparse_xent(dtype, V):
    bf16 = dtype == BF16
    figs = {}

    def note(f):
        for k, v in f.items():
            figs[k] = max(figs.get(k, 0.0), v)

    for rows in O.XENT_ROWS:
        z, lab64, fin64, ref, ref_fin = _case(V, rows, dtype)
        for lt in O.XENT_LABELS:
            labels, fin = lab64.to(lt), fin64.to(lt)
            for gs in O.grad_scales(rows):
                out = _run(z, labels, gs)
                note(_row_figures(out, ref, gs, bf16))
                want0 = ref["sums"][0]
                if np.isfinite(want0):
                    note({"sx_mean_loss": O.figure(out["sums"][0], torch.tensor(want0, dtype=F64, device=DEV),
                                                   ref["sum_scale"])})
                else:
                    assert float(out["sums"][0]) == want0, (float(out["sums"][0]), want0)
                assert _mean_correct_ok(out["sums"][1], ref), (float(out["sums"][1]), ref["sums"][1])
                # the labels moved off the -inf logit: the mean loss is finite; and two calls give the same bits
                a, b = _run(z, fin, gs), _run(z, fin, gs)
                note(_row_figures(a, ref_fin, gs, bf16))
                note({"sx_mean_loss": O.figure(a["sums"][0], torch.tensor(ref_fin["sums"][0], dtype=F64, device=DEV),
                                               ref_fin["sum_scale"])})
                assert _mean_correct_ok(a["sums"][1], ref_fin)
                assert all(_same_bits(a[k], b[k]) for k in OUTPUTS)
    _check(figs, ("xent", dtype, V))


@pytest.mark.parametrize("V", O.XENT_V)
@pytest.mark.parametrize("dtype", O.XENT_DTYPES, ids=("fp32", "bf16"))
def test_every_output_combination(dtype, V):
    """Each of loss_rows, dlogits, correct and sums absent in turn, and sums and part both: what is
    written is the same bits as with all of them, what is absent stays untouched."""
    rows = 7
    z, lab64, _, _, _ = _case(V, rows, dtype)
    labels = lab64.to(torch.int32)
    gs = 128.0 / rows
    full = _run(z, labels, gs)
    for absent in (("loss_rows",), ("dlogits",), ("correct",), ("sums",), ("sums", "part"),
                   ("loss_rows", "dlogits", "correct")):
        out = _run(z, labels, gs, absent)
        for k in OUTPUTS:
            if k not in absent and not (k == "part" and "sums" in absent):
                assert _same_bits(out[k], full[k]), (absent, k)


@pytest.mark.parametrize("V", (1, 2, 65, 1000))
@pytest.mark.parametrize("dtype", O.XENT_DTYPES, ids=("fp32", "bf16"))
def test_labels_out_of_range(dtype, V):
    """Labels -1 and V. xent_kernel reads the target logit only under lab_ok (zt is NaN otherwise)
    and the one-hot term compares the column index with the label, so no access depends on the bad
    label: the row's loss is NaN, correct 0, the mean loss NaN, and the rows around it are right."""
    zc, lc = O.bad_label_inputs(V, dtype)
    ref = O.xent(zc, lc, 1.0)
    ref = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ref.items()}
    z = zc.to(DEV)
    bad = ~ref["valid"]
    assert bad.tolist() == [False, False, True, False, False, True, False]
    assert bool(torch.isnan(ref["loss"][bad]).all()) and not bool(ref["correct"][bad].any())
    figs = {}
    for lt in O.XENT_LABELS:
        out = _run(z, lc.to(DEV).to(lt), 0.5)
        for k, v in _row_figures(out, ref, 0.5, dtype == BF16, rows_mask=ref["valid"]).items():
            figs[k] = max(figs.get(k, 0.0), v)
        assert bool(torch.isnan(out["sums"][0]))
        assert abs(float(out["sums"][1]) - float(ref["sums"][1])) <= ONE_ROUNDING
    _check(figs, ("bad labels", dtype, V))


# ------------------------------------------------------------------ in_top_k
@pytest.mark.parametrize("V", O.TOPK_V)
@pytest.mark.parametrize("dtype", O.XENT_DTYPES, ids=("fp32", "bf16"))
def test_in_top_k(dtype, V):
    """Exactly, with ties, -inf, +inf and NaN target logits, and targets -1 and V: in_top_k_kernel
    reads the target's logit only when `valid` (0 <= t < V) holds."""
    for rows in O.TOPK_ROWS:
        zc, tc = O.topk_inputs(V, rows, dtype)
        outside = tc.clone()
        outside[0] = -1
        outside[rows - 1] = V if rows > 1 else -1
        z = zc.to(DEV)
        for targets in (tc, outside):
            for k in O.TOPK_K:
                want = O.in_top_k(zc, targets, k)
                for lt in O.XENT_LABELS:
                    t = targets.to(DEV).to(lt)
                    out = Guarded((rows,), U8)
                    _lib.call("ttdk_in_top_k", z.data_ptr(), t.data_ptr(), LT[lt], out.t.data_ptr(), DT[dtype], rows, V,
                              k, _lib.stream())
                    assert out.intact()
                    assert out.t.tolist() == want.to(U8).tolist(), (rows, V, k, lt, targets.tolist())
        assert not bool(O.in_top_k(zc, outside, 5)[0])


# ------------------------------------------------------------------ refusals
def test_refusals_make_no_launch():
    """sums without part, an unknown dtype code, no rows, no columns: an error and nothing written.
    The logits are fp32 and the labels int64, so a kernel of either type would stay inside them."""
    rows, V = 7, 16
    z = torch.randn(rows, V, device=DEV)
    labels = torch.zeros(rows, dtype=torch.int64, device=DEV)
    loss, dl, corr = Guarded((rows,), F32), Guarded((rows, V), F32), Guarded((rows,), U8)
    sums, part = Guarded((2,), F32), Guarded((2 * rows,), F32)
    p = lambda b: b.t.data_ptr()  # noqa: E731

    def refused(name, *args):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args, _lib.stream())

    refused("ttdk_sparse_xent", z.data_ptr(), 0, labels.data_ptr(), 1, rows, V, 1.0, p(loss), p(dl), p(corr), p(sums),
            None)
    for zdt, ldt in ((2, 1), (-1, 1), (0, 2), (0, -1)):
        refused("ttdk_sparse_xent", z.data_ptr(), zdt, labels.data_ptr(), ldt, rows, V, 1.0, p(loss), p(dl), p(corr),
                p(sums), p(part))
    for r, v in ((0, V), (rows, 0)):
        refused("ttdk_sparse_xent", z.data_ptr(), 0, labels.data_ptr(), 1, r, v, 1.0, p(loss), p(dl), p(corr), p(sums),
                p(part))
    for dt in (2, -1):
        refused("ttdk_in_top_k", z.data_ptr(), labels.data_ptr(), 1, p(corr), dt, rows, V, 1)
    refused("ttdk_in_top_k", z.data_ptr(), labels.data_ptr(), 1, p(corr), 0, 0, V, 1)
    refused("ttdk_in_top_k", z.data_ptr(), labels.data_ptr(), 1, p(corr), 0, rows, 0, 1)
    torch.cuda.synchronize()
    for buf in (loss, dl, corr, sums, part):
        assert buf.untouched()


# ------------------------------------------------------------------ ttd.nn
def test_nn_sparse_softmax_cross_entropy_with_upstream_gradient():
    """fp32 logits [9, 65], a different upstream gradient g in every row (one of them 0, one
    negative): the loss against the oracle, and d loss / d logits against grad(scale 1) * g[:, None]
    at the scale |g| of the row (the gradient is stored at scale 1 and row_scale multiplies it)."""
    rows, V = 9, 65
    zc, lc = O.xent_inputs(V, rows, F32)
    lc = O.finite_labels(zc, lc)
    gen = torch.Generator().manual_seed(21)
    g = torch.randn(rows, generator=gen)
    g[0], g[1] = 0.0, -2.5
    ref = O.xent(zc, lc, 1.0)
    z = zc.to(DEV).requires_grad_(True)
    loss = ttd.nn.sparse_softmax_cross_entropy_with_logits(labels=lc.to(DEV), logits=z)
    loss.backward(g.to(DEV))
    want = ref["grad"] * g.double()[:, None]
    scale = g.double().abs()[:, None].expand_as(want)
    assert bool((z.grad[0] == 0).all())
    _check({"sx_loss": O.figure(loss.detach().cpu(), ref["loss"], ref["loss_scale"]),
            "sx_grad": O.figure(z.grad.cpu()[1:], want[1:], scale[1:])}, "nn")


def test_zz_report_gpu_maxima():
    """Runs last in this file: the largest figure of the tests above beside its bar."""
    for k in sorted(_seen):
        print("%-14s gpu max %.3e   bar %.1e" % (k, _seen[k], O.BARS[k]))
    assert set(_seen) == set(O.BARS)
