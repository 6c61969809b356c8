"""Fused LM-head cross-entropy (linear_xent.hip) on the GPU: `ops.transformer.linear_xent_fwd` /
`linear_xent_bwd` and `ttd.nn.linear_cross_entropy` against the float64 formula on the same bf16
inputs. The kernels' tile is 128 x 128 with BK = 64: T, V and H sit at and around those sizes.

x is a column slice of a wider buffer where the case says so; dh, dw and dbias are slices of larger
allocations with 256 guard rows on each side (dh with a wider row stride) that hold a sentinel which
must be unchanged afterwards. Bars (derived from the reference alone, u = 2^-24; E = 2 H u (|h| @ |w|^T)
bounds a logit's fp32 accumulation error, Em its row maximum):
  loss, lse  Em + 16 max(e32, u (1 + |ref|)), e32 the largest error of the float32 CPU formula in the case
  g (not an output)  dg = |dloss| E: the logit error through |g| <= |dloss|
  dw, dbias  (2^-8 + 2 T u) (|g|^T @ |h|) + dg^T @ |h|, the same with sums over rows: g is rounded to
             bf16 once (half an ulp is 2^-9, doubled), then accumulated in fp32
  dh         (2^-8 + 2 V u) (|g| @ |w|) + dg @ |w| + 2^-7 |ref| for its own bf16 store
Rows planted in every case with T >= 127: labels 0, V - 1, 127, 128; a negative label and one >= V
(ignored); the maximum in the last column tile; logits of +80 (last tile) and -80 (first tile), so
that the running maximum is rescaled; a tie of the label with another column (correct = 1); a column
strictly above the label (correct = 0).

Largest |err| / bar of any case on an MI355X (the |err| there, the case):
  loss   0.010  (5.9e-06, t300_v392_s2)      dh     0.386  (9.3e-03, t1_v8_h8)
  lse    0.010  (6.6e-06, all_ignored)       dw     0.561  (4.6e-03, t1_v8_h8)
                                             dbias  0.561  (2.7e-03, t1_v8_h8)
T = 1 shows the bf16 rounding of g alone (nothing averages it); the cases with T >= 127 stay below 0.25."""
import functools

import pytest
import torch

import tensorflow_train_distributed_amd.nn as ttd_nn
from tensorflow_train_distributed_amd.ops import transformer as X
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

pytestmark = pytest.mark.gpu

GUARD, PAD, SENT = 256, 8, 7.0
U = 2.0 ** -24
CASES = {  # T, V, H, splits, chunk_rows, bias, x strided, every row ignored
    "t1_v8_h8": (1, 8, 8, None, None, False, False, False),
    "t127_v120_h64": (127, 120, 64, None, None, True, False, False),
    "t128_v128_h72": (128, 128, 72, None, None, False, True, False),
    "t129_v136_h200": (129, 136, 200, None, None, True, True, False),
    "t300_v392_s1": (300, 392, 72, 1, 128, True, False, False),
    "t300_v392_s2": (300, 392, 72, 2, 128, False, True, False),
    "t300_v392_s3": (300, 392, 200, 3, 128, True, False, False),
    "all_ignored": (129, 136, 64, None, None, True, False, True),
}


def _reference(h, w, b, lab, dloss):
    """float64 loss, lse, correct, g, dh, dw, dbias of bf16 h, w and fp32 b (ignored rows are zero), and
    the bars of the module docstring."""
    hd, wd = h.double(), w.double()
    (T, H), V = h.shape, w.shape[0]
    z = hd @ wd.T + (b.double() if b is not None else 0)
    valid = (lab >= 0) & (lab < V)
    at = lab.clamp(0, V - 1).long()[:, None]
    zt, lse = z.gather(1, at)[:, 0], torch.logsumexp(z, 1)
    g = (torch.softmax(z, 1) - torch.zeros_like(z).scatter_(1, at, 1.0)) * dloss.double()[:, None] * valid[:, None]
    ref = {"loss": (lse - zt) * valid, "lse": lse, "correct": valid & (zt >= z.max(1).values),
           "dh": g @ wd, "dw": g.T @ hd, "dbias": g.sum(0)}
    z32 = h.float() @ w.float().T + (b if b is not None else 0)
    lse32 = torch.logsumexp(z32, 1)
    e32 = max(float((lse32 - lse).abs().max()), float(((lse32 - z32.gather(1, at)[:, 0]) * valid - ref["loss"]).abs().max()))
    ha, wa, ga = hd.abs(), wd.abs(), g.abs()
    E = 2 * H * U * (ha @ wa.T)
    Em = E.max(1).values
    dg = dloss.double().abs()[:, None] * E
    bars = {k: Em + 16 * torch.clamp(U * (1 + ref[k].abs()), min=e32) for k in ("loss", "lse")}
    bars["dw"] = (2.0 ** -8 + 2 * T * U) * (ga.T @ ha) + dg.T @ ha
    bars["dbias"] = (2.0 ** -8 + 2 * T * U) * ga.sum(0) + dg.sum(0)
    bars["dh"] = (2.0 ** -8 + 2 * V * U) * (ga @ wa) + dg @ wa + 2.0 ** -7 * ref["dh"].abs()
    return ref, bars


@functools.lru_cache(maxsize=None)
def _case(name):
    """CPU inputs, float64 references and bars of a case, made once and shared (never modified)."""
    T, V, H, _, _, bias, _, ignored = CASES[name]
    gen = torch.Generator().manual_seed(7)
    h, w, b, dloss = (torch.randn(s, generator=gen) for s in ((T, H), (V, H), (V,), (T,)))
    lab = torch.randint(0, V, (T,), generator=gen, dtype=torch.int32)
    if T >= 127:
        w[11], b[11], w[2] = w[10], b[10], -w[V - 3]
        lab[:6] = torch.tensor([0, V - 1, min(127, V - 1), min(128, V - 1), -1, V + 5])
        for row, col, label, z in ((6, V - 2, 0, 30.0), (7, V - 3, V - 3, 80.0), (8, 10, 10, 30.0), (9, 20, 21, 30.0)):
            h[row], lab[row] = w[col] * (z / float(w[col] @ w[col])), label
    if ignored:
        lab = torch.where(torch.arange(T) % 2 == 0, -1, V + 3).int()
    h, w, b = h.bfloat16(), w.bfloat16(), (b if bias else None)
    ref, bars = _reference(h, w, b, lab, dloss)
    if T >= 127 and not ignored:
        assert not ref["correct"][9] and float(ref["lse"][7]) > 70
        ref["correct"][8] = True  # the tie: equal columns give equal logits
    return (h, w, b, lab, dloss), ref, bars


def _guarded(rows, width, dtype, pad):
    whole = torch.full((rows + 2 * GUARD, width + pad), SENT, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + rows, :width]


def _run(name):
    """Forward and backward of a case on guarded buffers -> outputs by name, the guards checked."""
    T, V, H, splits, chunk, _, strided, _ = CASES[name]
    (h, w, b, lab, dloss), _, _ = _case(name)
    hg = torch.zeros(T, H + 16, dtype=torch.bfloat16, device="cuda")[:, 8:8 + H] if strided else h.cuda()
    hg.copy_(h)
    wg, bg, lg, dg = w.cuda(), (b.cuda() if b is not None else None), lab.cuda(), dloss.cuda()
    bufs = {"dh": _guarded(T, H, torch.bfloat16, PAD), "dw": _guarded(V, H, torch.float32, 0),
            "dbias": _guarded(1, V, torch.float32, 0)}
    out = dict(zip(("loss", "lse", "correct"), X.linear_xent_fwd(hg, wg, lg, bg, splits=splits)))
    X.linear_xent_bwd(hg, wg, lg, out["lse"], dg, bg, chunk_rows=chunk, dh=bufs["dh"][1], dw=bufs["dw"][1],
                      dbias=bufs["dbias"][1][0])
    torch.cuda.synchronize()
    for what, (whole, view) in bufs.items():
        out[what] = view.reshape(-1) if what == "dbias" else view
        guard = whole.clone()
        guard[GUARD:GUARD + view.shape[0], :view.shape[1]] = SENT
        assert bool((guard == SENT).all()), "%s: written outside its slice" % what
    return out


def _within_bars(name, got, ref, bars, kinds):
    for k in kinds:
        err = (got[k].detach().cpu().double() - ref[k]).abs()
        ratio = float((err / bars[k].clamp_min(1e-300)).max())
        print("%s %s: largest |err| %.3e, worst |err| / bar = %.3f" % (name, k, float(err.max()), ratio))
        assert bool((err <= bars[k]).all()), "%s %s: worst |err| / bar = %.3f" % (name, k, ratio)


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(name):
    (_, _, _, lab, _), ref, bars = _case(name)
    got = _run(name)
    assert torch.equal(got["correct"].cpu().bool(), ref["correct"])
    _within_bars(name, got, ref, bars, ("loss", "lse", "dh", "dw", "dbias"))
    off = ((lab < 0) | (lab >= CASES[name][1])).cuda()
    assert not got["loss"][off].any() and not got["dh"][off].any(), "ignored rows must be exactly 0"
    if CASES[name][7]:
        assert not got["dw"].any() and not got["dbias"].any(), "ignored rows must add exactly 0"


def test_bitwise_repeatable():
    a, b = _run("t300_v392_s2"), _run("t300_v392_s2")  # splits = 2 in the forward, three chunks back
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind", ["H=12", "V=100", "splits=0", "splits>col_tiles", "misaligned"])
def test_refusals(kind):
    H, V = (12 if kind == "H=12" else 16), (100 if kind == "V=100" else 136)
    h = torch.zeros(16, H + 8, dtype=torch.bfloat16, device="cuda")[:, 4:4 + H] if kind == "misaligned" else \
        torch.zeros(16, H, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(V, H, dtype=torch.bfloat16, device="cuda")
    lab = torch.zeros(16, dtype=torch.int32, device="cuda")
    splits = {"splits=0": 0, "splits>col_tiles": 3}.get(kind)
    with pytest.raises(InvalidArgumentError):
        X.linear_xent_fwd(h, w, lab, splits=splits)
    if splits is None:
        f = torch.zeros(16, device="cuda")
        with pytest.raises(InvalidArgumentError):
            X.linear_xent_bwd(h, w, lab, f, f)


@pytest.mark.parametrize("kind", ["fwd null workspace", "fwd odd workspace", "grad rows > T - r0", "grad null g"])
def test_native_refusals(kind):
    """The library's own checks (hipErrorInvalidValue before any launch), past the Python ones."""
    from tensorflow_train_distributed_amd.ops import _lib
    T, V, H = 16, 136, 16
    h, w = (torch.zeros(n, H, dtype=torch.bfloat16, device="cuda") for n in (T, V))
    lab = torch.zeros(T, dtype=torch.int32, device="cuda")
    f = [torch.zeros(2 * T + 4, device="cuda") for _ in range(5)]
    ws = {"fwd null workspace": None, "fwd odd workspace": f[0].data_ptr() + 4}.get(kind, f[0].data_ptr())
    with pytest.raises(_lib.HipKernelError):
        if kind.startswith("fwd"):
            _lib.call("ttdk_linear_xent_fwd", h.data_ptr(), H, w.data_ptr(), H, None, lab.data_ptr(), ws,
                      *(t.data_ptr() for t in f[1:]), T, V, H, 1, _lib.stream())
        else:
            g = None if kind == "grad null g" else torch.zeros(T, V, dtype=torch.bfloat16, device="cuda").data_ptr()
            _lib.call("ttdk_linear_xent_grad", h.data_ptr(), H, w.data_ptr(), H, None, lab.data_ptr(), f[1].data_ptr(),
                      f[2].data_ptr(), g, T, 8, (9 if "rows" in kind else 8), V, H, _lib.stream())


def test_nn_end_to_end():
    h, w, b, lab, _ = _case("t129_v136_h200")[0]
    ref, bars = _reference(h, w, b, lab, torch.ones(h.shape[0]))  # .sum(): dloss = 1
    bars["dw"] = bars["dw"] + 2.0 ** -7 * ref["dw"].abs()         # the gradient of bf16 weights is stored as bf16
    x, wt, bias = (t.cuda().requires_grad_() for t in (h.reshape(3, 43, -1), w, b))
    labels = lab.reshape(3, 43).cuda().long()
    labels[labels < 0] = 2 ** 32 + 5  # ignored, and must not wrap into class 5 on its way to int32
    loss = ttd_nn.linear_cross_entropy(x, wt, labels, bias)
    loss.sum().backward()
    got = {"loss": loss.reshape(-1), "dh": x.grad.reshape(h.shape), "dw": wt.grad, "dbias": bias.grad}
    _within_bars("nn", got, ref, bars, ("loss", "dh", "dw", "dbias"))
    with pytest.raises(InvalidArgumentError):
        ttd_nn.linear_cross_entropy(x.float(), wt.float(), labels, bias)
