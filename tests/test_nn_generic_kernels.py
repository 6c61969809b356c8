"""The shape-general kernels of csrc/kernels/nn_generic.hip (column statistics, their fold, the
column affine pass, inference-mode BN, any-width LayerNorm, the embedding gather and scatter,
tanh / sigmoid, the full reduction and its glue) and the fp32 MFMA GEMM of csrc/kernels/gemm_f32.hip
against the float64 statements of tests/nn_generic_oracle.py, at the smallest shapes that reach
each path: a column tail, fewer rows than row groups, a second and an empty row block, widths
below and off the wave, a second grid-stride trip, out-of-range and int32 ids, the null-pointer
forms, K odd and K = 0, leading dimensions wider than the row.

Every figure is element-wise, max |got - want| / scale, after half a bf16 ulp of want for a bf16
output. A bar is 16 x the largest value the same figure takes when the oracle itself runs in
float32 (tests/test_nn_generic_oracle_cpu.py), never less than 16 x 2^-24. LayerNorm's y and dx are
taken on the kernel's own mean and rstd once those are checked, the unary backward on the y it
is handed. What is exact (the gather, fill_scaled, row_scale, K = 0, special values, repeats, the
batched GEMM against the 2-D one) is compared by bits. Outputs sit between guard rows of a fixed
byte pattern that must survive, and start out as the pattern.

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure          MI355X     fp32      bar
  cs_part         6.5e-7     2.0e-7    4e-6   (four row groups of serial sums, where torch sums pairwise)
  cs_reduce       4.3e-7     9.6e-8    2e-6   (300 partial rows folded serially)
  cs_affine       1.1e-7     1.5e-7    3e-6
  bni_rstd        3.4e-8     5.5e-8    1e-6
  bni_scale       5.1e-8     1.1e-7    2e-6
  bni_shift       5.1e-8     6.4e-8    2e-6
  bni_dgamma      1.1e-7     1.2e-7    2e-6
  bni_dbeta       1.1e-7     1.1e-7    2e-6
  gln_mean        3.3e-8     9.7e-8    2e-6
  gln_rstd        5.4e-7     2.3e-7    4e-6
  gln_y           1.5e-7     2.0e-7    4e-6
  gln_dx          1.5e-7     1.6e-7    3e-6
  gln_dgamma      1.7e-7     1.8e-7    3e-6
  gln_dbeta       9.8e-8     9.9e-8    2e-6
  g_scatter       1.7e-7     1.4e-7    3e-6
  g_tanh          7.0e-8     5.6e-8    1e-6
  g_sigmoid       1.2e-7     1.2e-7    2e-6   (3.8e-6 with __expf, at x near -87: the kernel now calls expf)
  g_dtanh         8.7e-8     7.3e-8    2e-6
  g_dsigmoid      5.5e-7     3.1e-7    5e-6
  g_sum           2.5e-8     3.4e-8    1e-6
  f32_gemm        2.9e-7     2.9e-7    5e-6

No figure comes within 4 x of its bar. The constant rows and H = 1 of LayerNorm, where only eps is
under the root, hold gln_rstd and gln_y, and row blocks without rows write zeros.
"""
import os

import numpy as np
import pytest
import torch

import nn_generic_oracle as O
import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import gemm as G
from tensorflow_train_distributed_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
PATTERN = 0x5A
DT = {F32: 0, BF16: 1}
INF, NAN = float("inf"), float("nan")

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
        self.g = (self.g + 15) // 16 * 16
        self.raw = torch.full((2 * self.g + self.n,), PATTERN, dtype=U8, device=DEV)
        self.t = self.raw[self.g:self.g + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())

    def written(self):
        """Guards intact and no element of `t` still the pattern."""
        word = {2: 0x5A5A, 4: 0x5A5A5A5A}[self.t.element_size()]
        return self.intact() and bool((_bits(self.t) != word).all())


def _bits(t):
    t = t.contiguous()
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return _lib.stream()


def _dev(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


def _upd(figs, k, v):
    figs[k] = max(figs.get(k, 0.0), v)


# ------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("M,C,T", O.COL_STATS_CASES)
def test_col_stats(M, C, T, dtype):
    wrapper = T is None
    T = T or _lib.query("ttdk_col_stats_parts", M, C)
    assert T == (O.col_stats_parts(M, C) if wrapper else T)
    inp = _dev(O.col_stats_inputs(M, C, dtype))
    a, b, mu, rs = inp["a"], inp["b"], inp["mu"], inp["rs"]
    figs = {}
    for mode in (0, 1, 2):
        runs = []
        for _ in range(2):
            part = Guarded((T, 2, C), F32)
            _lib.call("ttdk_col_stats", _p(a), _p(b) if mode else None, _p(mu) if mode == 2 else None,
                      _p(rs) if mode == 2 else None, DT[dtype], mode, M, C, _p(part.t), T, _s())
            assert part.written(), (mode, "a block left the pattern or a guard was written")
            runs.append(part.t)
        assert _same_bits(runs[0], runs[1])
        want, mag = O.col_stats(a, T, b, mode, mu, rs)
        _upd(figs, "cs_part", O.figure(runs[0], want, mag))
        rpb = -(-M // T)
        for t in range(T):
            if t * rpb >= M:  # a block without rows: zeros, not the pattern
                assert bool((_bits(runs[0][t]) == 0).all()), (mode, t)
        if mode == 0 and C > 1:
            c = O.CH_MEAN64
            O.check({"cs_part": O.figure(runs[0][:, 1, c], want[:, 1, c], mag[:, 1, c])}, "mean 64")
        if wrapper:
            w_part, w_T = K.col_stats(a, b if mode else None, mode, mu if mode == 2 else None, rs if mode == 2 else None)
            assert w_T == T and _same_bits(w_part, runs[0])
    _check(figs, ("col_stats", M, C, T, dtype))


def test_col_stats_parts_values():
    for (M, C), want in O.PARTS_VALUES:
        assert _lib.query("ttdk_col_stats_parts", M, C) == want, (M, C)


@pytest.mark.parametrize("T", O.REDUCE_T)
def test_col_reduce2(T):
    figs = {}
    for C in O.REDUCE_C:
        inp = _dev(O.reduce_inputs(T, C))
        part, old = inp["part"].contiguous(), inp["old"]
        for use0, use1 in ((True, True), (False, True), (True, False)):
            for acc in (0, 1):
                o = [Guarded((C,), F32), Guarded((C,), F32)]
                for i in (0, 1):
                    if (use0, use1)[i]:
                        o[i].t.copy_(old[i]) if acc else o[i].t.fill_(NAN)  # acc = 0 must not read the old contents
                _lib.call("ttdk_col_reduce2", _p(part), T, C, _p(o[0].t) if use0 else None,
                          _p(o[1].t) if use1 else None, acc, _s())
                want, mag = O.col_reduce2(part, old if acc else None)
                for i in (0, 1):
                    if (use0, use1)[i]:
                        assert o[i].intact() and bool(torch.isfinite(o[i].t).all()), (C, use0, use1, acc)
                        _upd(figs, "cs_reduce", O.figure(o[i].t, want[i], mag[i]))
                    else:
                        assert o[i].untouched()
        w0, w1 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        K.col_reduce2(part, T, w0, w1)
        want, mag = O.col_reduce2(part)
        _upd(figs, "cs_reduce", O.figure(torch.stack([w0, w1]), want, mag))
    _check(figs, ("col_reduce2", T))


def _affine_call(a, b, c0, c1, c2, out, n, C):
    _lib.call("ttdk_col_affine", _p(a), _p(b), DT[a.dtype], _p(c0), _p(c1), _p(c2), _p(out), n, C, _s())


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_col_affine(dtype):
    figs = {}
    for C in O.AFFINE_C:
        inp = _dev(O.affine_inputs(O.AFFINE_ROWS, C, dtype))
        a, c0 = inp["a"], inp["c0"]
        n = a.numel()
        assert n % 256
        for form in O.AFFINE_FORMS:
            b, c1, c2 = O.affine_args(inp, form)
            out = Guarded(a.shape, dtype)
            _affine_call(a, b, c0, c1, c2, out.t, n, C)
            assert out.written(), (C, form)
            _upd(figs, "cs_affine", O.figure(out.t, O.col_affine(a, c0, b, c1, c2),
                                             O.col_affine_scale(a, c0, b, c1, c2), bf16_store=dtype == BF16))
            assert _same_bits(K.col_affine(a, c0, b, c1, c2), out.t)
        out = Guarded(a.shape, dtype)
        _affine_call(a, inp["b"], c0, inp["c1"], inp["c2"], out.t, 0, C)  # n = 0: succeeds, writes nothing
        torch.cuda.synchronize()
        assert out.untouched()
    _check(figs, ("col_affine", dtype))


def test_col_affine_second_grid_stride_trip():
    """bf16, C = 3, n = 2^24 + 15: 65536 blocks of 256 cover 2^24 elements, and 2^24 % 3 = 1, so
    the channel of an element changes from the first trip to the second."""
    inp, n = O.affine_wrap_inputs()
    inp = _dev(inp)
    C = O.AFFINE_WRAP[1]
    a, b = inp["a"].reshape(-1), inp["b"].reshape(-1)
    assert a.numel() >= n
    out = Guarded((n,), BF16)
    _affine_call(a, b, inp["c0"], inp["c1"], inp["c2"], out.t, n, C)
    assert out.written()
    args = (inp["a"], inp["c0"], inp["b"], inp["c1"], inp["c2"])
    want, mag = O.col_affine(*args).reshape(-1)[:n], O.col_affine_scale(*args).reshape(-1)[:n]
    _check({"cs_affine": O.figure(out.t, want, mag, bf16_store=True)}, "col_affine wrap")


@pytest.mark.parametrize("C", O.BNI_C)
def test_bn_infer(C):
    figs = {}
    eps = O.f32r(O.EPS_BN)
    for T in O.BNI_T:
        inp = _dev(O.bni_inputs(C, T))
        mm, mv = inp["mm"], inp["mv"]
        assert float(mv[0]) == 0
        for gamma in (inp["gamma"], None):
            for beta in (inp["beta"], None):
                outs = {k: Guarded((C,), F32) for k in ("scale", "shift", "rstd")}
                _lib.call("ttdk_bn_infer_coef", _p(mm), _p(mv), _p(gamma), _p(beta), eps, C, _p(outs["scale"].t),
                          _p(outs["shift"].t), _p(outs["rstd"].t), _s())
                want, sc = O.bn_infer_coef(mm, mv, gamma, beta, eps), O.bn_infer_coef_scales(mm, mv, gamma, beta, eps)
                for k, o in outs.items():
                    assert o.written(), k
                    _upd(figs, "bni_" + k, O.figure(o.t, want[k], sc[k]))
                w = K.bn_infer_coef(mm, mv, gamma, beta, eps)
                assert all(_same_bits(x.contiguous(), outs[k].t) for x, k in zip(w, ("scale", "shift", "rstd")))
        part, rstd = inp["part"].contiguous(), inp["rstd"]
        want, sc = O.bn_infer_bwd(part, mm, rstd), O.bn_infer_bwd_scales(part, mm, rstd)
        for use_g, use_b in ((True, True), (False, True), (True, False)):
            outs = {"dgamma": Guarded((C,), F32), "dbeta": Guarded((C,), F32)}
            _lib.call("ttdk_bn_infer_bwd", _p(part), T, C, _p(mm), _p(rstd), _p(outs["dgamma"].t) if use_g else None,
                      _p(outs["dbeta"].t) if use_b else None, _s())
            for k, used in (("dgamma", use_g), ("dbeta", use_b)):
                if used:
                    assert outs[k].written()
                    _upd(figs, "bni_" + k, O.figure(outs[k].t, want[k], sc[k]))
                else:
                    assert outs[k].untouched()
    _check(figs, ("bn_infer", C))


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("H,rows", O.LN_CASES)
def test_ln_generic(H, rows, dtype):
    inp = _dev(O.ln_inputs(H, rows, dtype))
    x, dy, gamma, beta = inp["x"], inp["dy"], inp["gamma"], inp["beta"]
    bf = dtype == BF16
    for eps in O.LN_EPS:
        eps = O.f32r(eps)
        y, mean, rstd = Guarded((rows, H), dtype), Guarded((rows,), F32), Guarded((rows,), F32)
        _lib.call("ttdk_ln_generic_fwd", _p(x), _p(gamma), _p(beta), _p(y.t), _p(mean.t), _p(rstd.t), DT[dtype], rows, H,
                  eps, _s())
        assert y.written() and mean.written() and rstd.written()
        m64, r64 = O.ln_stats(x, eps)
        sc = O.ln_scales(x, dy, m64, r64, gamma, beta)
        figs = {"gln_mean": O.figure(mean.t, m64, sc["mean"]), "gln_rstd": O.figure(rstd.t, r64, sc["rstd"])}
        if rows >= 77:
            r = O.ROW_OFFSET
            O.check({"gln_mean": O.figure(mean.t[r], m64[r], sc["mean"][r]),
                     "gln_rstd": O.figure(rstd.t[r], r64[r], r64[r])}, "offset row")
        # y and dx on the kernel's own statistics
        sc = O.ln_scales(x, dy, mean.t, rstd.t, gamma, beta)
        figs["gln_y"] = O.figure(y.t, O.ln_y(x, mean.t, rstd.t, gamma, beta), sc["y"], bf16_store=bf)
        dx = Guarded((rows, H), dtype)
        _lib.call("ttdk_ln_generic_bwd_dx", _p(dy), _p(x), _p(gamma), _p(mean.t), _p(rstd.t), _p(dx.t), DT[dtype], rows,
                  H, _s())
        assert dx.written()
        figs["gln_dx"] = O.figure(dx.t, O.ln_dx(dy, x, mean.t, rstd.t, gamma), sc["dx"], bf16_store=bf)
        # the wrappers: the same forward, dgamma and dbeta by mode 2 and col_reduce2, with and without dx
        w_y, w_mean, w_rstd = K.ln_generic_fwd(x, gamma, beta, eps)
        assert _same_bits(w_y, y.t) and _same_bits(w_mean.contiguous(), mean.t) and _same_bits(w_rstd.contiguous(), rstd.t)
        dg, db = Guarded((H,), F32), Guarded((H,), F32)
        w_dx = K.ln_generic_bwd(dy, x, gamma, w_mean, w_rstd, dg.t, db.t)
        assert dg.written() and db.written() and _same_bits(w_dx, dx.t)
        want_dg, want_db = O.ln_dparams(dy, x, mean.t, rstd.t)
        figs["gln_dgamma"] = O.figure(dg.t, want_dg, sc["dgamma"])
        figs["gln_dbeta"] = O.figure(db.t, want_db, sc["dbeta"])
        dg2, db2 = Guarded((H,), F32), Guarded((H,), F32)
        assert K.ln_generic_bwd(dy, x, gamma, w_mean, w_rstd, dg2.t, db2.t, want_dx=False) is None
        assert dg2.intact() and db2.intact() and _same_bits(dg2.t, dg.t) and _same_bits(db2.t, db.t)
        _check(figs, ("ln", H, rows, dtype, eps))


# ------------------------------------------------------------------ embedding
def _gather(table, ids, V=None):
    Vt, H = table.shape
    out = Guarded(tuple(ids.shape) + (H,), table.dtype)
    _lib.call("ttdk_gather_generic", _p(table), _p(ids), int(ids.dtype == torch.int64), _p(out.t), DT[table.dtype],
              ids.numel(), H, Vt if V is None else V, _s())
    assert out.written()
    return out.t


@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("idtype", O.EMBED_IDS)
@pytest.mark.parametrize("V,H", O.EMBED_TABLES)
def test_gather_and_scatter(V, H, idtype, dtype):
    figs = {}
    for same in (False, True):
        inp = _dev(O.embed_inputs(V, H, idtype, dtype, same))
        table, ids, dy = inp["table"], inp["ids"], inp["dy"]
        assert ids.dim() == 2 and ids.dtype == idtype
        got = _gather(table, ids)
        assert _same_bits(got, O.gather(table, ids))
        assert _same_bits(K.gather_generic(table, ids), got)
        bad = len(O.out_of_range(V, idtype))
        assert bool((got[2, 1:1 + bad] == 0).all())
        for old in (torch.zeros_like(inp["old"]), inp["old"]):
            dtable = Guarded((V, H), F32)
            dtable.t.copy_(old)
            _lib.call("ttdk_scatter_add_generic", _p(dy), _p(ids), int(idtype == torch.int64), _p(dtable.t), DT[dtype],
                      ids.numel(), H, V, _s())
            assert dtable.intact()  # an out-of-range id writes nowhere
            want, mag = O.scatter_add(dy.cpu(), ids.cpu(), old.cpu())
            _upd(figs, "g_scatter", O.figure(dtable.t.cpu(), want, mag))
    _check(figs, ("embedding", V, H, idtype, dtype))


def test_gather_second_grid_stride_trip():
    V, H, shape = O.GATHER_WRAP
    gen = O._gen(V, H, 21)
    table = torch.randn(V, H, generator=gen).bfloat16().to(DEV)
    ids = torch.randint(-1, V + 1, shape, generator=gen, dtype=torch.int32).to(DEV)  # -1 and V among them
    assert ids.numel() * H > 65536 * 256
    got = _gather(table, ids)
    assert _same_bits(got, O.gather(table, ids))


# ------------------------------------------------------------------ tanh and sigmoid
def _unary(x, op, n=None):
    n = x.numel() if n is None else n
    y = Guarded((n,), x.dtype)
    _lib.call("ttdk_unary", _p(x), _p(y.t), DT[x.dtype], n, op, _s())
    assert y.written() if n else y.untouched()
    return y.t


def _unary_bwd(dy, y, op):
    dx = Guarded((y.numel(),), y.dtype)
    _lib.call("ttdk_unary_bwd", _p(dy), _p(y), _p(dx.t), DT[y.dtype], y.numel(), op, _s())
    assert dx.written() if y.numel() else dx.untouched()
    return dx.t


_UNARY = ((O.TANH, "g_tanh", "g_dtanh"), (O.SIGMOID, "g_sigmoid", "g_dsigmoid"))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_unary(dtype):
    x = O.unary_inputs(dtype).to(DEV)
    bf = dtype == BF16
    figs = {}
    for op, fwd, bwd in _UNARY:
        y = _unary(x, op)
        want = O.unary(x, op)
        figs[fwd] = O.figure(y, want, want.abs(), bf16_store=bf)
        assert _same_bits(K.unary(x, op), y)
        assert _same_bits(_unary(x, op, 257), y[:257])  # n = 257: one block and one element
        _unary(x, op, 0)
        _unary_bwd(x[:0], x[:0], op)
        dy_grid, y_grid = (t.to(DEV) for t in O.unary_bwd_inputs(op, dtype))
        gen = O._gen(op, 22)
        dy_own = torch.randn(y.numel(), generator=gen).to(dtype).to(DEV)
        for d, yy in ((dy_grid, y_grid), (dy_own, y)):  # a grid over the open range, and the kernel's own y
            dx = _unary_bwd(d, yy, op)
            _upd(figs, bwd, O.figure(dx, O.unary_bwd(d, yy, op), O.unary_bwd_scale(d, yy, op), bf16_store=bf))
            assert _same_bits(K.unary_bwd(d, yy, op), dx)
        assert _same_bits(_unary_bwd(dy_grid[:257].contiguous(), y_grid[:257].contiguous(), op),
                          _unary_bwd(dy_grid, y_grid, op)[:257])
    _check(figs, ("unary", dtype))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_unary_special_values(dtype):
    z = torch.tensor([0.0, -0.0, INF, -INF, NAN], dtype=dtype, device=DEV)
    t, s = _unary(z, O.TANH), _unary(z, O.SIGMOID)
    assert _same_bits(t[:4], torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=dtype, device=DEV)), t.tolist()
    assert _same_bits(s[:4], torch.tensor([0.5, 0.5, 1.0, 0.0], dtype=dtype, device=DEV)), s.tolist()
    assert bool(torch.isnan(t[4])) and bool(torch.isnan(s[4]))
    # finite |x| in (87, 1e4]: the sigmoid saturates and is never NaN
    big = torch.cat([torch.linspace(87, 104, 1001)[1:], torch.tensor([88.0, 88.5, 88.75, 89.0, 1e3, 1e4])]).to(dtype)
    big = big[big.float() > 87].to(DEV)
    lo, hi = _unary(-big, O.SIGMOID).double(), _unary(big, O.SIGMOID).double()
    assert bool(((lo >= 0) & (lo <= 2.0 ** -125)).all()), lo.max()
    assert bool(((hi >= 1 - 2.0 ** -23) & (hi <= 1)).all()), hi.min()
    th = _unary(torch.cat([big, -big]), O.TANH).double()
    assert bool((th.abs() == 1).all())


def test_unary_second_grid_stride_trip():
    base = O.unary_inputs(BF16)
    n = O.UNARY_WRAP
    x = base.repeat(-(-n // base.numel()))[:n].contiguous().to(DEV)
    assert n > 65536 * 256
    figs = {}
    for op, fwd, _ in _UNARY:
        y = _unary(x, op)
        want = O.unary(x, op)
        figs[fwd] = O.figure(y, want, want.abs(), bf16_store=True)
        del want
    _check(figs, "unary wrap")


# ------------------------------------------------------------------ reductions and scaling glue
@pytest.mark.parametrize("dtype", O.DTYPES)
def test_sum_all(dtype):
    figs = {}
    for n in O.SUM_N:
        x = O.sum_inputs(n, dtype).to(DEV)
        nb = _lib.query("ttdk_sum_blocks", n)
        for scale in (1.0, O.f32r(1.0 / n)):
            runs = []
            for _ in range(2):
                out, ws = Guarded((1,), dtype), Guarded((nb,), F32)
                _lib.call("ttdk_sum_all", _p(x), DT[dtype], n, _p(ws.t), scale, _p(out.t), _s())
                assert out.written() and ws.written()
                runs.append(out.t)
            assert _same_bits(runs[0], runs[1])
            want, mag = O.sum_all(x, scale)
            _upd(figs, "g_sum", O.figure(runs[0][0], want, mag, bf16_store=dtype == BF16))
            assert _same_bits(K.sum_all(x, scale).reshape(1), runs[0])
    _check(figs, ("sum_all", dtype))


def test_sum_blocks_values():
    for n, want in O.SUM_BLOCKS:
        assert _lib.query("ttdk_sum_blocks", n) == want, n


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_fill_scaled_and_row_scale_are_one_multiply(dtype):
    for n in (1, 257, 1000):
        for gv, scale in ((1.0, 1.0 / n), (-3.3, 0.7)):
            g = torch.tensor([gv], dtype=dtype, device=DEV)
            dx = Guarded((n,), dtype)
            _lib.call("ttdk_fill_scaled", _p(dx.t), DT[dtype], n, _p(g), scale, _s())
            assert dx.written()
            want = O.scaled_fp32(g.cpu(), torch.tensor(scale, dtype=F32)).expand(n)
            assert _same_bits(dx.t.cpu(), want.contiguous())
            assert _same_bits(K.fill_scaled((n,), g[0], scale, dtype), dx.t)
    for rows, C in O.ROW_SCALE_CASES:
        a, g = (t.to(DEV) for t in O.row_scale_inputs(rows, C, dtype))
        out = Guarded((rows, C), dtype)
        _lib.call("ttdk_row_scale", _p(a), _p(g), _p(out.t), DT[dtype], rows, C, _s())
        assert out.written()
        assert _same_bits(out.t.cpu(), O.scaled_fp32(a.cpu(), g.cpu()[:, None]))
        assert _same_bits(K.row_scale(a, g), out.t)


# ------------------------------------------------------------------ the fp32 GEMM
def _in_wider(t, pad):
    wide = torch.full((t.shape[0], t.shape[1] + 2 * pad), NAN, dtype=t.dtype, device=DEV)
    wide[:, pad:pad + t.shape[1]] = t
    return wide[:, pad:pad + t.shape[1]]


def test_gemm_f32():
    figs = {}
    pad = O.GEMM_PAD
    for M, N, K_, ta, tb, bias, beta, sliced in O.gemm_cases():
        label = (M, N, K_, ta, tb, bias, beta, sliced)
        inp = _dev(O.gemm_inputs(M, N, K_, ta, tb, sliced))
        A, B = inp["A"], inp["B"]
        bv, C0 = (inp["bias"] if bias else None), (inp["C0"] if beta else None)
        if sliced:  # columns of tensors 2*pad wider, NaN either side: what is read outside the slice shows
            A, B = _in_wider(A, pad), _in_wider(B, pad)
            assert A.stride() == (A.shape[1] + 2 * pad, 1) and B.stride() == (B.shape[1] + 2 * pad, 1)
        buf = Guarded((M, N + 2 * pad) if sliced else (M, N), F32)
        out = buf.t[:, pad:pad + N] if sliced else buf.t
        out.copy_(C0) if beta else out.fill_(NAN)  # beta = 0 must not read C
        got = G.gemm_f32(A, B, trans_a=ta, trans_b=tb, out=out, bias=bv, beta=beta)
        assert got.data_ptr() == out.data_ptr() and buf.intact(), label
        if sliced:  # the columns of the wider C outside the slice
            assert bool((_bits(buf.t[:, :pad]) == 0x5A5A5A5A).all()) and bool((_bits(buf.t[:, pad + N:]) == 0x5A5A5A5A).all())
        assert bool(torch.isfinite(out).all()), label
        if K_ == 0:  # exactly bias + beta*C
            exact = torch.zeros((M, N), device=DEV) + (bv if bias else 0.0)
            assert _same_bits(out.contiguous(), exact + C0 if beta else exact), label
        _upd(figs, "f32_gemm", O.figure(out, O.gemm(A, B, ta, tb, bv, C0), O.gemm_scale(A, B, ta, tb, bv, C0)))
        if not (sliced or beta):
            assert _same_bits(G.gemm_f32(A, B, trans_a=ta, trans_b=tb, bias=bv), out)
    _check(figs, "gemm_f32")


@pytest.mark.parametrize("Bt,shape", O.BATCHED_CASES)
def test_gemm_batched_fp32(Bt, shape):
    M, N, K_ = shape
    figs = {}
    for ta, tb in ((False, False), (True, False), (False, True)):
        inp = _dev(O.gemm_inputs(M, N, K_, ta, tb, batch=Bt))
        A, B = inp["A"], inp["B"]
        got = G.gemm_batched(A, B, trans_a=ta, trans_b=tb)
        assert got.shape == (Bt, M, N) and got.dtype == F32
        for z in range(Bt):  # each entry: the bits of the 2-D call
            assert _same_bits(got[z], G.gemm_f32(A[z], B[z], trans_a=ta, trans_b=tb)), (z, ta, tb)
        _upd(figs, "f32_gemm", O.figure(got, O.gemm(A, B, ta, tb), O.gemm_scale(A, B, ta, tb)))
    # through the ABI into a guarded C
    inp = _dev(O.gemm_inputs(M, N, K_, False, False, batch=Bt))
    A, B = inp["A"], inp["B"]
    C = Guarded((Bt, M, N), F32)
    _lib.call("ttdk_gemm_f32_batched", _p(A), K_, M * K_, 0, _p(B), N, K_ * N, 0, _p(C.t), N, M * N, M, N, K_, Bt, _s())
    assert C.written() and _same_bits(C.t, G.gemm_batched(A, B))
    _check(figs, ("gemm_batched", Bt, shape))


# ------------------------------------------------------------------ refusals
def test_refusals_make_no_launch():
    """Every refused call returns an error before any launch and leaves its outputs as they were.
    The buffers hold 8 x 16 elements, which every size below that is not itself refused stays within."""
    M, C = 8, 16
    x = torch.randn(M, C, device=DEV)
    v = torch.ones(C, device=DEV)
    ids = torch.zeros(M, dtype=torch.int32, device=DEV)
    out, part, st0, st1 = Guarded((M, C), F32), Guarded((4, 2, C), F32), Guarded((M,), F32), Guarded((M,), F32)

    def refused(name, *args):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args, _s())

    px, pv, po, pp = _p(x), _p(v), _p(out.t), _p(part.t)
    for a in ((px, px, pv, pv, 0, 0, M, 0, pp, 1),        # C = 0
              (px, px, pv, pv, 0, 0, 0, C, pp, 1),        # M = 0
              (px, px, pv, pv, 0, 0, M, C, pp, 0),        # T = 0
              (px, None, pv, pv, 0, 1, M, C, pp, 1),      # mode 1 without b
              (px, px, None, pv, 0, 2, M, C, pp, 1),      # mode 2 without mu
              (px, px, pv, pv, 0, 3, M, C, pp, 1),        # mode 3
              (px, px, pv, pv, 2, 0, M, C, pp, 1)):       # dt = 2
        refused("ttdk_col_stats", *a)
    refused("ttdk_col_affine", px, None, 0, pv, None, None, po, M * C, 0)     # C = 0
    refused("ttdk_col_affine", px, px, 0, pv, None, None, po, M * C, C)       # b without c1
    refused("ttdk_col_affine", px, None, 2, pv, None, None, po, M * C, C)     # dt = 2
    for rows, H, dt in ((M, 0, 0), (0, C, 0), (M, C, 2)):
        refused("ttdk_ln_generic_fwd", px, pv, pv, po, _p(st0.t), _p(st1.t), dt, rows, H, 1e-5)
        refused("ttdk_ln_generic_bwd_dx", px, px, pv, pv, pv, po, dt, rows, H)
    for op, dt in ((2, 0), (0, 2)):
        refused("ttdk_unary", px, po, dt, M * C, op)
        refused("ttdk_unary_bwd", px, px, po, dt, M * C, op)
    refused("ttdk_gather_generic", px, _p(ids), 0, po, 2, M, C, M)
    refused("ttdk_scatter_add_generic", px, _p(ids), 0, po, 2, M, C, M)
    refused("ttdk_gemm_f32", px, C, 0, px, C, 0, po, C, None, 0, 0, C, M)     # M = 0
    refused("ttdk_gemm_f32", px, C, 0, px, C, 0, po, C, None, 0, M, C, -1)    # K = -1
    for batch in (0, 65536):
        refused("ttdk_gemm_f32_batched", px, C, 0, 0, px, C, 0, 0, po, C, 0, M, C, M, batch)
    torch.cuda.synchronize()
    for buf in (out, part, st0, st1):
        assert buf.untouched()


# ------------------------------------------------------------------ through ttd.nn
class _Spy:
    """The names _lib.call is given while it is active."""

    def __init__(self, monkeypatch):
        self.names = []
        real = _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *a: (self.names.append(name), real(name, *a))[1])
        self.undo = monkeypatch.undo

    def ran(self, *names):
        self.undo()
        missing = [n for n in names if n not in self.names]
        assert not missing, (missing, self.names)


def _leaf(t, dtype=None):
    return t.to(DEV).to(dtype or t.dtype).requires_grad_(True)


@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("affine", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("training", (True, False))
def test_nn_batch_norm(training, affine, dtype, monkeypatch):
    """[2, 5, 7, 10] NHWC: 70 rows of 10 channels. Forward and every gradient against float64
    autograd of the plain formula (the stored output's rounding and the statistics' errors come on
    top of the kernels' own, so the bars are those of the parts added up: the training forward and
    its gradients are held to the end-to-end bars of tests/batchnorm_oracle.py)."""
    import batchnorm_oracle as B
    gen = O._gen(int(training), int(affine[0]), int(affine[1]), 31)
    shape, Cc, eps, mom = (2, 5, 7, 10), 10, 1e-3, 0.9
    xc = (torch.randn(shape, generator=gen) * 1.5 + 0.5).to(dtype)
    dyc = torch.randn(shape, generator=gen).to(dtype)
    gc = torch.rand(Cc, generator=gen) + 0.5 if affine[0] else None
    bc = torch.randn(Cc, generator=gen) if affine[1] else None
    rm0, rv0 = torch.randn(Cc, generator=gen), torch.rand(Cc, generator=gen) + 0.5
    x = _leaf(xc)
    gamma, beta = (None if gc is None else _leaf(gc)), (None if bc is None else _leaf(bc))
    rm, rv = rm0.clone().to(DEV), rv0.clone().to(DEV)
    spy = _Spy(monkeypatch)
    y = ttd.nn.batch_norm(x, gamma, beta, rm, rv, training=training, momentum=mom, eps=eps)
    y.backward(dyc.to(DEV))
    spy.ran("ttdk_col_stats", "ttdk_col_affine", *(() if training else ("ttdk_bn_infer_coef", "ttdk_bn_infer_bwd")))
    assert y.dtype == dtype and y.shape == x.shape
    # float64 autograd of the plain formula
    M = 70
    x2 = xc.reshape(M, Cc).double().requires_grad_(True)
    ga = (gc.double() if gc is not None else torch.ones(Cc, dtype=F64)).requires_grad_(True)
    ba = (bc.double() if bc is not None else torch.zeros(Cc, dtype=F64)).requires_grad_(True)
    mean, var = (x2.mean(0), x2.var(0, unbiased=False)) if training else (rm0.double(), rv0.double())
    ya = (x2 - mean) / torch.sqrt(var + O.f32r(eps)) * ga + ba
    ya.backward(dyc.reshape(M, Cc).double())
    bf = dtype == BF16
    xd, dd = xc.reshape(M, Cc).double(), dyc.reshape(M, Cc).double()
    if training:
        ref = B.fwd_stats(xd, gc, bc, O.f32r(eps))
        A1, Q = B.data_scales(xd)
        ssc = B.stats_scales(A1, Q, ref, gc, bc, O.f32r(eps), M, O.f32r(mom), rm0, rv0)
        want_rm, want_rv = B.running(rm0, rv0, ref["mean"], ref["var"], M, O.f32r(mom))
        figs = {"bn_run_mean": O.figure(rm.cpu(), want_rm, ssc["run_mean"]),
                "bn_run_var": O.figure(rv.cpu(), want_rv, ssc["run_var"])}
        # y = x*scale + shift: the errors of scale and shift at their scales, and the pass itself
        ysc = xd.abs() * ssc["scale"] + ssc["shift"] + B.apply_scale(xd, ref["scale"], ref["shift"])
        figs["bn_out"] = O.figure(y.detach().cpu().reshape(M, Cc), ya.detach(), ysc, bf16_store=bf)
        esc = B.e2e_scales(xd, dd, ref, gc, O.f32r(eps))
        figs["bn_e2e_dz"] = O.figure(x.grad.cpu().reshape(M, Cc), x2.grad, esc["e2e_dz"], bf16_store=bf)
        if gamma is not None:
            figs["bn_e2e_dgamma"] = O.figure(gamma.grad.cpu(), ga.grad, esc["e2e_dgamma"])
        if beta is not None:
            figs["bn_e2e_dbeta"] = O.figure(beta.grad.cpu(), ba.grad, esc["e2e_dbeta"])
        print(("nn.batch_norm", training, affine, dtype), {k: "%.2e" % v for k, v in figs.items()})
        B.check(figs, ("nn.batch_norm", affine, dtype))
        return
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    co = O.bn_infer_coef(rm0, rv0, gc, bc, O.f32r(eps))
    csc = O.bn_infer_coef_scales(rm0, rv0, gc, bc, O.f32r(eps))
    # y = x*scale + shift and dx = dy*scale: the coefficients' errors at their scales on top of the pass
    ysc = xd.abs() * csc["scale"] + csc["shift"] + O.col_affine_scale(xd, co["scale"], c2=co["shift"])
    figs = {"cs_affine": O.figure(y.detach().cpu().reshape(M, Cc), ya.detach(), ysc, bf16_store=bf)}
    _upd(figs, "cs_affine", O.figure(x.grad.cpu().reshape(M, Cc), x2.grad,
                                     dd.abs() * csc["scale"] + O.col_affine_scale(dd, co["scale"]), bf16_store=bf))
    # dgamma = rstd*(sum g*x - mm*sum g), from sums of 70 terms: the terms' magnitudes, and rstd's own error
    sg, sgx = dd.abs().sum(0), (dd * xd).abs().sum(0)
    if gamma is not None:
        figs["bni_dgamma"] = O.figure(gamma.grad.cpu(), ga.grad, (co["rstd"] + csc["rstd"]) * (sgx + rm0.double().abs() * sg))
    if beta is not None:
        figs["bni_dbeta"] = O.figure(beta.grad.cpu(), ba.grad, sg)
    _check(figs, ("nn.batch_norm", training, affine, dtype))


@pytest.mark.parametrize("H,dtype", [(100, F32), (768, F32), (768, BF16)])
def test_nn_layer_norm_generic_path(H, dtype, monkeypatch):
    rows, eps = 6, 1e-5
    inp = O.ln_inputs(H, rows, dtype)
    x, gamma, beta = _leaf(inp["x"].reshape(2, 3, H)), _leaf(inp["gamma"]), _leaf(inp["beta"])
    spy = _Spy(monkeypatch)
    y = ttd.nn.layer_norm(x, gamma, beta, eps)
    y.backward(inp["dy"].reshape(2, 3, H).to(DEV))
    spy.ran("ttdk_ln_generic_fwd", "ttdk_ln_generic_bwd_dx", "ttdk_col_stats", "ttdk_col_reduce2")
    xa, ga, ba = (t.double().requires_grad_(True) for t in (inp["x"], inp["gamma"], inp["beta"]))
    mu = xa.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((xa - mu) ** 2).mean(1, keepdim=True) + O.f32r(eps))
    ya = (xa - mu) * rstd * ga + ba
    ya.backward(inp["dy"].double())
    m, r = mu.detach()[:, 0], rstd.detach()[:, 0]
    sc = O.ln_scales(inp["x"], inp["dy"], m, r, inp["gamma"], inp["beta"])
    bf = dtype == BF16
    # end to end y also carries the statistics' errors, d y = gamma*(-rstd*d mean + xh*d rstd/rstd), at
    # their own scales (max_c |x| and rstd, under bars no larger than y's): where xh and beta are both
    # near 0 the error of the mean is all there is
    g = inp["gamma"].double().abs()
    xh = ((xa - mu) * rstd).detach().abs()
    sc["y"] = sc["y"] + g * (r * sc["mean"])[:, None] + g * xh
    assert O.BARS["gln_mean"] <= O.BARS["gln_y"] and O.BARS["gln_rstd"] <= O.BARS["gln_y"]
    _check({"gln_y": O.figure(y.detach().cpu().reshape(rows, H), ya.detach(), sc["y"], bf16_store=bf),
            "gln_dx": O.figure(x.grad.cpu().reshape(rows, H), xa.grad, sc["dx"], bf16_store=bf),
            "gln_dgamma": O.figure(gamma.grad.cpu(), ga.grad, sc["dgamma"]),
            "gln_dbeta": O.figure(beta.grad.cpu(), ba.grad, sc["dbeta"])}, ("nn.layer_norm", H, dtype))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_nn_embedding_lookup_with_an_out_of_range_id(dtype, monkeypatch):
    V, H = 50, 24
    inp = O.embed_inputs(V, H, torch.int64, dtype)
    table = _leaf(inp["table"])
    spy = _Spy(monkeypatch)
    out = ttd.nn.embedding_lookup(table, inp["ids"].to(DEV))
    out.backward(inp["dy"].to(DEV))
    spy.ran("ttdk_gather_generic", "ttdk_scatter_add_generic")
    assert _same_bits(out.detach().cpu(), O.gather(inp["table"], inp["ids"]))
    want, mag = O.scatter_add(inp["dy"], inp["ids"], torch.zeros(V, H))
    assert table.grad.dtype == dtype
    _check({"g_scatter": O.figure(table.grad.cpu(), want, mag, bf16_store=dtype == BF16)}, ("nn.embedding", dtype))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_nn_reduce_mean_tanh_sigmoid(dtype, monkeypatch):
    bf = dtype == BF16
    xc = O.sum_inputs(4097, dtype).reshape(17, 241)
    x = _leaf(xc)
    spy = _Spy(monkeypatch)
    m = ttd.nn.reduce_mean(x)
    m.backward()
    spy.ran("ttdk_sum_all", "ttdk_fill_scaled")
    want, mag = O.sum_all(xc, O.f32r(1 / 4097))
    figs = {"g_sum": O.figure(m.detach().cpu(), want, mag, bf16_store=bf)}
    assert _same_bits(x.grad.cpu(), O.scaled_fp32(torch.ones((), dtype=dtype), torch.tensor(O.f32r(1 / 4097))).expand(17, 241).contiguous())
    for op, fn, fwd, bwd in ((O.TANH, ttd.nn.tanh, "g_tanh", "g_dtanh"), (O.SIGMOID, ttd.nn.sigmoid, "g_sigmoid", "g_dsigmoid")):
        xc = (torch.randn(3, 91, generator=O._gen(op, 33)) * 3).to(dtype)
        dyc = torch.randn(3, 91, generator=O._gen(op, 34)).to(dtype)
        x = _leaf(xc)
        spy = _Spy(monkeypatch)
        y = fn(x)
        y.backward(dyc.to(DEV))
        spy.ran("ttdk_unary", "ttdk_unary_bwd")
        want = O.unary(xc, op)
        figs[fwd] = O.figure(y.detach().cpu(), want, want.abs(), bf16_store=bf)
        ys = y.detach().cpu()  # the gradient from the stored y
        figs[bwd] = O.figure(x.grad.cpu(), O.unary_bwd(dyc, ys, op), O.unary_bwd_scale(dyc, ys, op), bf16_store=bf)
    _check(figs, ("nn.unary", dtype))


def test_nn_dense_fp32_on_a_slice_of_a_wider_tensor(monkeypatch):
    gen = O._gen(37, 91, 35)
    wide = torch.randn(37, 120, generator=gen)
    wc, bc, dyc = torch.randn(91, 29, generator=gen), torch.randn(29, generator=gen), torch.randn(37, 29, generator=gen)
    base = wide.to(DEV)
    x = base[:, 11:102].requires_grad_(True)
    assert x.shape == (37, 91) and not x.is_contiguous()
    w, b = _leaf(wc), _leaf(bc)
    spy = _Spy(monkeypatch)
    y = ttd.nn.dense(x, w, b)
    y.backward(dyc.to(DEV))
    spy.ran("ttdk_gemm_f32")
    xc = wide[:, 11:102]
    figs = {"f32_gemm": O.figure(y.detach().cpu(), O.gemm(xc, wc, bias=bc), O.gemm_scale(xc, wc, bias=bc))}
    _upd(figs, "f32_gemm", O.figure(x.grad.cpu(), O.gemm(dyc, wc, tb=True), O.gemm_scale(dyc, wc, tb=True)))
    _upd(figs, "f32_gemm", O.figure(w.grad.cpu(), O.gemm(xc, dyc, ta=True), O.gemm_scale(xc, dyc, ta=True)))
    assert float((b.grad.cpu().double() - dyc.double().sum(0)).abs().max()) <= O.BARS["cs_reduce"] * float(dyc.abs().sum(0).max())
    _check(figs, "nn.dense")


def test_zz_report_gpu_maxima():
    """Runs last in this file: the largest figure of the tests above beside its bar, printed, and
    written to nn_generic_maxima.txt in the directory TTD_TEST_REPORT_DIR names, if it is set."""
    lines = ["%-14s gpu max %.3e   bar %.1e" % (k, _seen[k], O.BARS[k]) for k in sorted(_seen)]
    print("\n".join(lines))
    out = os.environ.get("TTD_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "nn_generic_maxima.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert set(_seen) == set(O.BARS)
