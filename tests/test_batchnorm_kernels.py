"""The kernels of csrc/kernels/batchnorm.hip (the partial-sum kernels, the fixed-order fold and
finalize, the legacy atomic fold with its two finalize kernels, the apply and backward-apply
streaming passes with their mask, g_out and fp8 options) against the float64 statements of
tests/batchnorm_oracle.py, at the shapes where each kernel takes another path.

Every comparison is element-wise: |got - want| <= half a bf16 ulp of want (bf16 outputs only: the
store) + bar * scale, with the scale of each figure and its bar in batchnorm_oracle.BARS. A bar is
16 x the largest value the same figure takes when the oracle itself runs in float32 with the
kernel's one-pass formulas (tests/test_batchnorm_oracle_cpu.py), never less than 16 x 2^-24. The
statistics are checked first; the apply output and dz are then checked on the kernel's own
coefficients. What is exact (the mask, g_out, the bit-mask path against the `out` path, a repeated
fixed-order fold, masked and gamma = 0 channels, the bf16 results beside an fp8 copy) is compared
exactly. Outputs sit between guard rows of a fixed byte pattern that must survive.

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure          MI355X     fp32      bar
  bn_partial      7.3e-7     2.1e-7    4e-6   (C = 8: 256 row lanes folded one after the other)
  bn_sums         5.1e-7     2.4e-7    4e-6   (atomics: the last digit moves from run to run)
  bn_mean         5.2e-7     2.6e-7    5e-6
  bn_var          7.4e-7     5.5e-7    9e-6
  bn_rstd         4.9e-7     2.7e-7    5e-6
  bn_scale        4.9e-7     2.7e-7    5e-6
  bn_shift        4.6e-7     2.7e-7    5e-6
  bn_run_mean     3.8e-7     2.4e-7    4e-6
  bn_run_var      7.4e-7     4.7e-7    8e-6
  bn_out          3.0e-8     1.3e-7    3e-6
  bn_dbeta        2.8e-7     2.7e-7    5e-6
  bn_dgamma       2.9e-7     2.7e-7    5e-6
  bn_coef         3.2e-7     3.2e-7    5e-6
  bn_dz           5.0e-8     1.6e-7    3e-6
  bn_e2e_dbeta    1.3e-8     1.3e-8    1e-6
  bn_e2e_dgamma   4.2e-8     3.4e-8    1e-6
  bn_e2e_dz       6.4e-9     1.4e-7    3e-6

The one-pass variance E[x^2] - mean^2 holds its bar at every case here, the channel of mean 64 and
unit spread included: its error is charged at the scale E[x^2], where the formula works."""
import numpy as np
import pytest
import torch

import batchnorm_oracle as O
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
PATTERN = 0x5A
EPS, MOM = O.f32r(O.EPS), O.f32r(O.MOMENTUM)

_seen = {}


def _check(figs, label):
    for k, v in figs.items():
        _seen[k] = max(_seen.get(k, 0.0), v)
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    return O.check(figs, label)


class Guarded:
    """A tensor `t` of `shape` with O.GUARD rows (elements of a 1-D shape) of the byte PATTERN on
    either side in one allocation; `t` starts out as the pattern too (or as `init`), so what a
    kernel leaves unwritten shows."""

    def __init__(self, shape, dtype, init=None):
        shape = tuple(shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.n = int(np.prod(shape)) * item
        self.g = O.GUARD * (int(np.prod(shape[1:])) if len(shape) > 1 else 1) * item
        self.g = (self.g + 15) // 16 * 16  # the kernels move 16 B at a time: keep `t` aligned
        self.raw = torch.full((2 * self.g + self.n,), PATTERN, dtype=U8, device=DEV)
        self.t = self.raw[self.g:self.g + self.n].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())


def _bits(t):
    t = t.contiguous()
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _state(C, mean=None, rstd=None):
    """A BNState whose four rows lie in one guarded buffer."""
    buf = Guarded((4, C), F32)
    st = K.BNState.__new__(K.BNState)
    st.mean, st.rstd, st.scale, st.shift = buf.t[0], buf.t[1], buf.t[2], buf.t[3]
    if mean is not None:
        st.mean.copy_(mean)
        st.rstd.copy_(rstd)
    return st, buf


def _got_state(st, rm=None, rv=None):
    got = {"mean": st.mean, "rstd": st.rstd, "scale": st.scale, "shift": st.shift}
    if rm is not None:
        got["run_mean"], got["run_var"] = rm, rv
    return got


# ------------------------------------------------------------------ statistics from data
def _stats_case(M, C, affine=True, run=True):
    inp = _dev(O.stats_inputs(M, C))
    x = inp["x"]
    gamma, beta = (inp["gamma"], inp["beta"]) if affine else (None, None)
    T = K.bn_num_partials(M, C)
    assert T == max(1, min(2048, -(-M // (16 * O.rlanes(C)))))
    part = Guarded((T, 2, C), F32)
    _, T2 = K.bn_stats_partial(x, part.t)
    assert T2 == T and part.intact()
    want, mag = O.block_sums(x, T)
    figs = {"bn_partial": O.figure(part.t, want, mag)}

    A1, Q = O.data_scales(x)
    ref = O.fwd_stats(x, gamma, beta, EPS)
    ub = (M - 1) / M if M > 1 else 1.0

    def fold(finalize, momentum, rm, rv, old):
        st, sbuf = _state(C)
        finalize(st, momentum, rm.t if run else None, rv.t if run else None)
        assert sbuf.intact()
        r = dict(ref)
        got = _got_state(st)
        if run:
            assert rm.intact() and rv.intact()
            r["run_mean"], r["run_var"] = O.running(old[0], old[1], ref["mean"], ref["var"], M, momentum)
            got = _got_state(st, rm.t, rv.t)
        sc = O.stats_scales(A1, Q, r, gamma, beta, EPS, M, momentum, *(old if run else (None, None)))
        f = O.stats_figures(got, r, sc)
        if run and momentum == 0.0:  # the running variance is then the batch variance itself
            f["bn_var"] = O.figure(rv.t.double() * ub, ref["var"], Q)
        return f, st

    def fused(st, momentum, rm, rv):
        K.bn_fwd_stats(part.t, T, M, gamma, beta, EPS, momentum, rm, rv, st)

    sums = Guarded((2, C), F32)
    K.bn_reduce_partials(part.t, T, C, sums.t)
    assert sums.intact()
    p64 = part.t.double()
    figs["bn_sums"] = O.figure(sums.t, p64.sum(0), p64.abs().sum(0))

    def legacy(st, momentum, rm, rv):
        K.bn_fwd_finalize(sums.t, M, gamma, beta, EPS, momentum, rm, rv, st)

    for name, fin in (("fused", fused), ("legacy", legacy)):
        rm, rv = Guarded((C,), F32, inp["rm0"]), Guarded((C,), F32, inp["rv0"])
        f0, st0 = fold(fin, 0.0, rm, rv, (inp["rm0"], inp["rv0"]))
        old = (rm.t.clone(), rv.t.clone())
        f1, st1 = fold(fin, MOM, rm, rv, old)  # the second call starts from what the first left
        for k in ("mean", "rstd", "scale", "shift"):
            assert _same_bits(getattr(st0, k), getattr(st1, k))
        for f in (f0, f1):
            for k, v in f.items():
                figs[k] = max(figs.get(k, 0.0), v)
    # exact by construction: an all-zero channel has mean 0 and shift = beta
    assert float(st0.mean[O.CH_ZERO]) == 0 and float(st0.shift[O.CH_ZERO]) == (float(beta[O.CH_ZERO]) if affine else 0)
    assert float(st0.scale[O.CH_GAMMA0]) == 0 or not affine
    _check(figs, ("stats", M, C, affine, run))


@pytest.mark.parametrize("M,C", O.STATS_CASES)
def test_statistics_from_data(M, C):
    _stats_case(M, C)


def test_statistics_without_affine_or_running():
    _stats_case(1361, 24, affine=False)
    _stats_case(1361, 24, run=False)
    _stats_case(34, 2056, affine=False, run=False)


# ------------------------------------------------------------------ folds of synthetic partials
def _reduce_finalize(p, T, C, bwd, count, gamma, beta, momentum, rm, rv, st, dg=None, db=None, coef=None, acc=False):
    """ttdk_bn_reduce_finalize with a guarded slab; returns the slab."""
    S = _lib.query("ttdk_bn_finalize_slices", T)
    assert S == max(1, min(256, -(-T // 32)))
    slab = Guarded((S, 2, C), F32)
    _lib.call("ttdk_bn_reduce_finalize", p.data_ptr(), T, C, slab.t.data_ptr(), int(bwd), float(count), K._p(gamma),
              K._p(beta), EPS, momentum, K._p(rm), K._p(rv), st.mean.data_ptr(), st.rstd.data_ptr(),
              st.scale.data_ptr(), st.shift.data_ptr(), K._p(dg), K._p(db), K._p(coef), int(acc), _lib.stream())
    assert slab.intact()
    if T <= 256:
        assert slab.untouched()
    return slab


@pytest.mark.parametrize("C", O.FOLD_C)
@pytest.mark.parametrize("T", O.FOLD_T)
def test_fold_of_synthetic_partials(T, C):
    inp = _dev(O.fold_inputs(T, C))
    p, gamma, beta, M = inp["partial"], inp["gamma"], inp["beta"], O.FOLD_COUNT
    s, q, a_s, a_q = O.fold_truth(p)
    p0 = p.clone()
    # forward: the wrapper, then the entry itself with a guarded slab: bit for bit the same
    ref = O.stats_from_sums(s, q, M, gamma, beta, EPS)
    ref["run_mean"], ref["run_var"] = O.running(inp["rm0"], inp["rv0"], ref["mean"], ref["var"], M, MOM)
    sc = O.stats_scales(a_s / M, a_q / M, ref, gamma, beta, EPS, M, MOM, inp["rm0"], inp["rv0"])
    st, sbuf = _state(C)
    rm, rv = Guarded((C,), F32, inp["rm0"]), Guarded((C,), F32, inp["rv0"])
    K.bn_fwd_stats(p, T, M, gamma, beta, EPS, MOM, rm.t, rv.t, st)
    assert sbuf.intact() and rm.intact() and rv.intact()
    figs = O.stats_figures(_got_state(st, rm.t, rv.t), ref, sc)
    st2, sbuf2 = _state(C)
    rm2, rv2 = Guarded((C,), F32, inp["rm0"]), Guarded((C,), F32, inp["rv0"])
    _reduce_finalize(p, T, C, False, M, gamma, beta, MOM, rm2.t, rv2.t, st2)
    assert _same_bits(sbuf.t, sbuf2.t) and _same_bits(rm.t, rm2.t) and _same_bits(rv.t, rv2.t)
    assert sbuf2.intact() and rm2.intact() and rv2.intact()

    # backward: the same rows read as (sum g, sum g*y) with a given state
    bst, bbuf = _state(C, inp["mean"], inp["rstd"])
    state0 = bbuf.raw.clone()
    scb = {}
    for acc in (False, True):
        old = (inp["dg0"], inp["db0"]) if acc else (None, None)
        refb = O.bwd_coef(s, q, M, inp["mean"], inp["rstd"], gamma, *old)
        scb[acc] = O.bwd_scales(a_s, a_q, M, inp["mean"], inp["rstd"], gamma, *old)
        runs = []
        for rep in range(2):
            dg, db, coef = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"]), Guarded((3, C), F32)
            if rep == 0:
                coef.t.copy_(K.bn_backward_coef(M, C, gamma, bst, dg.t, db.t, p, T, accumulate=acc))
            else:
                _reduce_finalize(p, T, C, True, M, gamma, None, 0.0, None, None, bst, dg.t, db.t, coef.t, acc)
            assert dg.intact() and db.intact() and coef.intact()
            runs.append((dg.t, db.t, coef.t))
        assert all(_same_bits(a, b) for a, b in zip(*runs))
        for k, v in O.bwd_figures({"dgamma": runs[0][0], "dbeta": runs[0][1], "coef": runs[0][2]}, refb, scb[acc]).items():
            figs[k] = max(figs.get(k, 0.0), v)
    assert torch.equal(bbuf.raw, state0)  # the backward reads the state only

    # the atomic fold and the two legacy finalize kernels: held to the bars only
    sums = Guarded((2, C), F32)
    K.bn_reduce_partials(p, T, C, sums.t)
    assert sums.intact()
    figs["bn_sums"] = max(O.figure(sums.t[0], s, a_s), O.figure(sums.t[1], q, a_q))
    st3, sbuf3 = _state(C)
    rm3, rv3 = Guarded((C,), F32, inp["rm0"]), Guarded((C,), F32, inp["rv0"])
    K.bn_fwd_finalize(sums.t, M, gamma, beta, EPS, MOM, rm3.t, rv3.t, st3)
    assert sbuf3.intact() and rm3.intact() and rv3.intact()
    for k, v in O.stats_figures(_got_state(st3, rm3.t, rv3.t), ref, sc).items():
        figs[k] = max(figs.get(k, 0.0), v)
    # ttdk_bn_bwd_finalize against the fused backward finalize on the same sums (one partial row)
    s1, q1 = sums.t[0].double(), sums.t[1].double()
    for acc in (False, True):
        old = (inp["dg0"], inp["db0"]) if acc else (None, None)
        refb = O.bwd_coef(s1, q1, M, inp["mean"], inp["rstd"], gamma, *old)
        sc1 = O.bwd_scales(s1.abs(), q1.abs(), M, inp["mean"], inp["rstd"], gamma, *old)
        dg, db, coef = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"]), Guarded((3, C), F32)
        _lib.call("ttdk_bn_bwd_finalize", sums.t.data_ptr(), float(M), C, gamma.data_ptr(), bst.mean.data_ptr(),
                  bst.rstd.data_ptr(), dg.t.data_ptr(), db.t.data_ptr(), coef.t.data_ptr(), int(acc), _lib.stream())
        assert dg.intact() and db.intact() and coef.intact()
        dg2, db2 = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
        coef2 = K.bn_backward_coef(M, C, gamma, bst, dg2.t, db2.t, sums.t.view(1, 2, C), 1, accumulate=acc)
        for got in ({"dgamma": dg.t, "dbeta": db.t, "coef": coef.t}, {"dgamma": dg2.t, "dbeta": db2.t, "coef": coef2}):
            for k, v in O.bwd_figures(got, refb, sc1).items():
                figs[k] = max(figs.get(k, 0.0), v)
        two = {"dgamma": dg2.t, "dbeta": db2.t, "coef": coef2}
        for k, v in {"dgamma": dg.t, "dbeta": db.t, "coef": coef.t}.items():
            assert O.figure(v, two[k], sc1[k]) <= O.BARS["bn_" + k]
    assert torch.equal(p, p0)
    _check(figs, ("fold", T, C))


# ------------------------------------------------------------------ apply
def _apply_args(inp, option):
    res, rs, rh, relu = O.apply_kwargs(inp, option)
    return dict(residual=res, residual_bn=(rs, rh) if rs is not None else None, relu=relu), (res, rs, rh, relu)


def _apply_case(M, C, option):
    inp = _dev(O.apply_inputs(M, C))
    kw, (res, rs, rh, relu) = _apply_args(inp, option)
    y, scale, shift = inp["y"], inp["scale"], inp["shift"]
    want = O.apply(y, scale, shift, res, rs, rh, relu=relu)
    sc = O.apply_scale(y, scale, shift, res, rs, rh)
    out = Guarded((M, C), BF16)
    ret = K.bn_apply(y, scale, shift, out=out.t, **kw)
    assert ret.data_ptr() == out.t.data_ptr() and out.intact()
    figs = {"bn_out": O.figure(out.t, want, sc, bf16_store=True)}
    # with the mask: the same output bit for bit; the mask is [stored out > 0]
    out2, mask = Guarded((M, C), BF16), Guarded((M * C // 8,), U8)
    K.bn_apply(y, scale, shift, out=out2.t, mask=mask.t, **kw)
    assert out2.intact() and mask.intact()
    assert _same_bits(out.t, out2.t)
    assert torch.equal(mask.t, O.mask_bits(out2.t))
    keep = O.mask_bools(mask.t, (M, C))
    sure = want.abs() > O.BARS["bn_out"] * sc + O.bf16_half_ulp(want)
    assert torch.equal(keep[sure], (want > 0)[sure])
    # the elements built to land on +0, -0 and 2^-140: stored as zero, mask bit 0
    rows = O.zero_rows(M)
    assert bool((out.t[rows, 0:3].float() == 0).all()) and not bool(keep[rows, 0:3].any())
    if not relu:
        assert bool((out.t.float() < 0).any())
    return figs, out2.t, mask.t


@pytest.mark.parametrize("option", O.APPLY_OPTIONS)
@pytest.mark.parametrize("C", O.APPLY_C)
def test_apply(C, option):
    figs = {}
    for M in O.apply_Ms(C):
        f, _, _ = _apply_case(M, C, option)
        figs["bn_out"] = max(figs.get("bn_out", 0.0), f["bn_out"])
    _check(figs, ("apply", C, option))


def _slot(scale):
    init = torch.zeros(K.FP8_SLOT, dtype=F32)
    init[2], init[3] = scale, 1.0 / scale
    return Guarded((K.FP8_SLOT,), F32, init), init.to(DEV)


def _check_fp8(q8, slot, slot0, stored, qs, e5m2):
    """The fp8 copy of the stored bf16 values: within half a step of stored*qs clamped to the
    format's range; the slot's amax lanes hold max |stored| exactly and nothing else moved."""
    fmax = 57344.0 if e5m2 else 448.0
    v = (stored.double() * qs).clamp(-fmax, fmax).cpu().reshape(-1)
    dec = O.fp8_decode(q8, e5m2)
    assert bool(((dec - v).abs() <= O.fp8_half_step(v, e5m2)).all())
    assert float(slot[8:72].max()) == float(stored.float().abs().max())
    assert torch.equal(slot[:8], slot0[:8])
    return bool((v.abs() == fmax).any())


@pytest.mark.parametrize("C", O.APPLY_C)
def test_apply_fp8_copy(C):
    M = O.apply_Ms(C)[-1]
    qs = 64.0
    for option in ("relu", "residual_bn"):
        inp = _dev(O.apply_inputs(M, C))
        kw, _ = _apply_args(inp, option)
        _, out_ref, mask_ref = _apply_case(M, C, option)
        slot, slot0 = _slot(qs)
        out, mask, q8 = Guarded((M, C), BF16), Guarded((M * C // 8,), U8), Guarded((M * C,), U8)
        K.bn_apply(inp["y"], inp["scale"], inp["shift"], out=out.t, mask=mask.t, q8=q8.t, q8_slot=slot.t, **kw)
        assert out.intact() and mask.intact() and q8.intact() and slot.intact()
        assert _same_bits(out.t, out_ref) and torch.equal(mask.t, mask_ref)
        assert _check_fp8(q8.t, slot.t, slot0, out.t, qs, False)  # some values are clamped at 448
        slot2, _ = _slot(qs)
        mask2, q82 = Guarded((M * C // 8,), U8), Guarded((M * C,), U8)
        assert K.bn_apply(inp["y"], inp["scale"], inp["shift"], mask=mask2.t, q8=q82.t, q8_slot=slot2.t,
                          store_out=False, **kw) is None
        assert mask2.intact() and q82.intact() and slot2.intact()
        assert torch.equal(mask2.t, mask.t) and torch.equal(q82.t, q8.t) and _same_bits(slot2.t, slot.t)


# ------------------------------------------------------------------ backward
def _bwd_run(inp, M, C, src, with_g_out, acc, figs):
    """bn_backward with the ReLU source `src` ("out", "mask" or None); returns what it wrote."""
    y, dy, gamma = inp["y"], inp["dy"], inp["gamma"]
    keep = inp["out"].float() > 0 if src else None
    out = inp["out"] if src == "out" else None
    mask = O.mask_bits(inp["out"]) if src == "mask" else None
    g = O.relu_grad(dy, keep)
    st, sbuf = _state(C, inp["mean"], inp["rstd"])
    state0 = sbuf.raw.clone()
    old = (inp["dg0"], inp["db0"]) if acc else (None, None)
    # the partial kernel and the finalize on their own: the kernel's coefficients
    T = K.bn_num_partials(M, C)
    part, gbuf0 = Guarded((T, 2, C), F32), Guarded((M, C), BF16)
    _lib.call("ttdk_bn_bwd_partial", dy.data_ptr(), K._p(out), K._p(mask), y.data_ptr(), M, C, part.t.data_ptr(), T,
              gbuf0.t.data_ptr() if with_g_out else None, _lib.stream())
    assert part.intact() and gbuf0.intact()
    want, mag = O.block_sums(g, T, other=y)
    figs["bn_partial"] = max(figs.get("bn_partial", 0.0), O.figure(part.t, want, mag))
    dgc, dbc = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
    coef = K.bn_backward_coef(M, C, gamma, st, dgc.t, dbc.t, part.t, T, accumulate=acc)
    sg, sgy = O.bwd_sums(g, y)
    asg, asgy = O.bwd_sums(g.abs(), y.double().abs())
    ref = O.bwd_coef(sg, sgy, M, inp["mean"], inp["rstd"], gamma, *old)
    sc = O.bwd_scales(asg, asgy, M, inp["mean"], inp["rstd"], gamma, *old)
    for k, v in O.bwd_figures({"dgamma": dgc.t, "dbeta": dbc.t, "coef": coef}, ref, sc).items():
        figs[k] = max(figs.get(k, 0.0), v)
    # the whole of bn_backward, dz passed in
    dz, gbuf = Guarded((M, C), BF16), Guarded((M, C), BF16)
    dg, db = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
    ret = K.bn_backward(dy, out, y, gamma, st, dg.t, db.t, g_out=gbuf.t if with_g_out else None, dz=dz.t,
                        accumulate=acc, mask=mask)
    assert ret.data_ptr() == dz.t.data_ptr()
    assert dz.intact() and gbuf.intact() and dg.intact() and db.intact() and torch.equal(sbuf.raw, state0)
    assert _same_bits(dg.t, dgc.t) and _same_bits(db.t, dbc.t)  # the fold is fixed-order
    figs["bn_dz"] = max(figs.get("bn_dz", 0.0), O.figure(dz.t, O.dz_from_coef(coef, g, y), O.dz_scale(coef, g, y),
                                                         bf16_store=True))
    if with_g_out and src:
        want_g = torch.where(keep, dy, torch.zeros_like(dy))  # dy where the mask is set, +0 elsewhere
        assert _same_bits(gbuf.t, want_g) and _same_bits(gbuf0.t, want_g)
    else:
        assert gbuf.untouched() and gbuf0.untouched()
    assert bool((dz.t[:, O.CH_GAMMA0].float() == 0).all())
    if src:  # CH_MASKED is nowhere positive: its sums are exact zeros
        assert bool((dz.t[:, O.CH_MASKED].float() == 0).all())
        assert float(dg.t[O.CH_MASKED]) == (float(inp["dg0"][O.CH_MASKED]) if acc else 0.0)
        assert float(db.t[O.CH_MASKED]) == (float(inp["db0"][O.CH_MASKED]) if acc else 0.0)
    return dz.t, dg.t, db.t, gbuf.t


@pytest.mark.parametrize("acc", (False, True))
@pytest.mark.parametrize("C", O.APPLY_C)
def test_backward(C, acc):
    figs = {}
    for M in O.apply_Ms(C):
        inp = _dev(O.apply_inputs(M, C))
        a = _bwd_run(inp, M, C, "out", True, acc, figs)
        b = _bwd_run(inp, M, C, "mask", True, acc, figs)
        assert all(_same_bits(u, v) for u, v in zip(a, b))  # the bit-mask path is the `out` path
        c = _bwd_run(inp, M, C, "mask" if acc else "out", False, acc, figs)
        assert all(_same_bits(u, v) for u, v in zip(a[:3], c[:3]))
        _bwd_run(inp, M, C, None, False, acc, figs)
    _check(figs, ("backward", C, acc))


def _row_split(g, y, T):
    """partial fp32 [T, 2, C] of (sum g, sum g*y) over T even row chunks, summed in float64."""
    M = y.shape[0]
    want, _ = O.block_sums(g, T, other=y)
    assert T * (-(-M // T)) >= M
    return want.float().contiguous()


@pytest.mark.parametrize("C", O.APPLY_C)
def test_backward_from_partial(C):
    figs = {}
    qs, clamped = 2.0 ** 15, False
    for i, M in enumerate(O.apply_Ms(C)):
        inp = _dev(O.apply_inputs(M, C))
        y, gamma = inp["y"], inp["gamma"]
        acc = bool(i % 2)
        old = (inp["dg0"], inp["db0"]) if acc else (None, None)
        g = O.relu_grad(inp["dy"], inp["out"].float() > 0).bfloat16()
        T = min(M, 3)
        part = _row_split(g, y, T)
        part0 = part.clone()
        st, sbuf = _state(C, inp["mean"], inp["rstd"])
        dgc, dbc = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
        coef = K.bn_backward_coef(M, C, gamma, st, dgc.t, dbc.t, part, T, accumulate=acc)
        s, q, a_s, a_q = O.fold_truth(part)
        ref = O.bwd_coef(s, q, M, inp["mean"], inp["rstd"], gamma, *old)
        sc = O.bwd_scales(a_s, a_q, M, inp["mean"], inp["rstd"], gamma, *old)
        for k, v in O.bwd_figures({"dgamma": dgc.t, "dbeta": dbc.t, "coef": coef}, ref, sc).items():
            figs[k] = max(figs.get(k, 0.0), v)
        dz, dg, db = Guarded((M, C), BF16), Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
        ret = K.bn_backward_from_partial(g, y, gamma, st, dg.t, db.t, part, T, dz=dz.t, accumulate=acc)
        assert ret.data_ptr() == dz.t.data_ptr() and dz.intact() and dg.intact() and db.intact() and sbuf.intact()
        assert _same_bits(dg.t, dgc.t) and _same_bits(db.t, dbc.t) and torch.equal(part, part0)
        figs["bn_dz"] = max(figs.get("bn_dz", 0.0), O.figure(dz.t, O.dz_from_coef(coef, g, y), O.dz_scale(coef, g, y),
                                                             bf16_store=True))
        assert bool((dz.t[:, O.CH_GAMMA0].float() == 0).all()) and bool((dz.t[:, O.CH_MASKED].float() == 0).all())
        # the e5m2 copy: the bf16 result is the same beside it, and it alone is the same too
        slot, slot0 = _slot(qs)
        dz2, q8 = Guarded((M, C), BF16), Guarded((M * C,), U8)
        dg2, db2 = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
        K.bn_backward_from_partial(g, y, gamma, st, dg2.t, db2.t, part, T, dz=dz2.t, accumulate=acc, q8=q8.t,
                                   q8_slot=slot.t)
        assert dz2.intact() and q8.intact() and slot.intact()
        assert _same_bits(dz2.t, dz.t) and _same_bits(dg2.t, dg.t) and _same_bits(db2.t, db.t)
        clamped |= _check_fp8(q8.t, slot.t, slot0, dz.t, qs, True)
        slot3, _ = _slot(qs)
        q83 = Guarded((M * C,), U8)
        dg3, db3 = Guarded((C,), F32, inp["dg0"]), Guarded((C,), F32, inp["db0"])
        assert K.bn_backward_from_partial(g, y, gamma, st, dg3.t, db3.t, part, T, accumulate=acc, q8=q83.t,
                                          q8_slot=slot3.t, store_dz=False) is None
        assert q83.intact() and slot3.intact()
        assert torch.equal(q83.t, q8.t) and _same_bits(slot3.t, slot.t) and _same_bits(dg3.t, dg.t)
    assert clamped  # some values of some M are clamped at 57344
    _check(figs, ("from_partial", C))


@pytest.mark.parametrize("M,C", O.E2E_CASES)
def test_end_to_end(M, C):
    """The kernels' own forward state, output and mask feed the backward; the oracle is the whole
    training-mode BN + residual + ReLU in float64, with g taken through the kernel's stored out
    (its sign near 0 is the apply test's business)."""
    inp = _dev(O.e2e_inputs(M, C))
    y, res, dy, gamma, beta = inp["y"], inp["res"], inp["dy"], inp["gamma"], inp["beta"]
    part, T = K.bn_stats_partial(y)
    st, _ = _state(C)
    rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
    K.bn_fwd_stats(part, T, M, gamma, beta, EPS, MOM, rm, rv, st)
    mask = torch.empty(M * C // 8, dtype=U8, device=DEV)
    out = K.bn_apply(y, st.scale, st.shift, residual=res, relu=True, mask=mask)
    dg, db, gout = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.empty_like(y)
    dz = K.bn_backward(dy, None, y, gamma, st, dg, db, g_out=gout, mask=mask)
    ref = O.fwd_stats(y, gamma, beta, EPS)
    g = O.relu_grad(dy, out.float() > 0)
    assert _same_bits(gout, g.bfloat16())
    want_dz, want_dg, want_db = O.bwd_direct(g, y, ref["mean"], ref["rstd"], gamma)
    sc = O.e2e_scales(y, g, ref, gamma, EPS)
    _check({"bn_e2e_dbeta": O.figure(db, want_db, sc["e2e_dbeta"]),
            "bn_e2e_dgamma": O.figure(dg, want_dg, sc["e2e_dgamma"]),
            "bn_e2e_dz": O.figure(dz, want_dz, sc["e2e_dz"], bf16_store=True)}, ("e2e", M, C))


# ------------------------------------------------------------------ the grid-stride wrap
def test_grid_stride_wrap():
    """C = 64, M = 2^20 + 8: M*C/8 is 64 vectors past 8192 blocks of 1024, so block 0 of the apply
    and backward-apply kernels takes a second trip of its grid-stride loop, for the last 8 rows."""
    M, C = O.WRAP_M, O.WRAP_C
    assert M * C // 8 == 8192 * 1024 + 64
    gen = torch.Generator(device=DEV).manual_seed(77)
    y, res, dy = (torch.randn(M, C, device=DEV, dtype=BF16, generator=gen) for _ in range(3))
    small = _dev(O.apply_inputs(16, C))
    scale, shift = small["scale"], small["shift"]
    rows = torch.cat([torch.randperm(M - 4096, generator=torch.Generator().manual_seed(78))[:4096],
                      torch.arange(M - 4096, M)]).to(DEV)
    out, mask = Guarded((M, C), BF16), Guarded((M * C // 8,), U8)
    K.bn_apply(y, scale, shift, residual=res, relu=True, out=out.t, mask=mask.t)
    assert out.intact() and mask.intact()
    figs = {}
    for lo in range(0, rows.numel(), 2048):  # the float64 reference in row chunks
        r = rows[lo:lo + 2048]
        want = O.apply(y[r], scale, shift, res[r], relu=True)
        f = O.figure(out.t[r], want, O.apply_scale(y[r], scale, shift, res[r]), bf16_store=True)
        figs["bn_out"] = max(figs.get("bn_out", 0.0), f)
        assert torch.equal(O.mask_bools(mask.t.view(M, C // 8)[r].reshape(-1), (r.numel(), C)), out.t[r].float() > 0)
    del out, mask
    st, _ = _state(C, small["mean"], small["rstd"])
    part = torch.stack([small["dg0"], small["db0"] * 50]).view(1, 2, C).contiguous()
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    coef = K.bn_backward_coef(M, C, small["gamma"], st, dg, db, part, 1)
    dz = Guarded((M, C), BF16)
    K.bn_backward_from_partial(dy, y, small["gamma"], st, dg, db, part, 1, dz=dz.t)
    assert dz.intact()
    for lo in range(0, rows.numel(), 2048):
        r = rows[lo:lo + 2048]
        f = O.figure(dz.t[r], O.dz_from_coef(coef, dy[r], y[r]), O.dz_scale(coef, dy[r], y[r]), bf16_store=True)
        figs["bn_dz"] = max(figs.get("bn_dz", 0.0), f)
    _check(figs, ("wrap", M, C))


# ------------------------------------------------------------------ refusals
def test_refusals_make_no_launch():
    C = 8
    inp = _dev(O.apply_inputs(4, C))
    y, sc, sh = inp["y"], inp["scale"], inp["shift"]
    out, q8, part = Guarded((4, C), BF16), Guarded((4 * C,), U8), Guarded((1, 2, 16), F32)
    p, s = (lambda t: t.data_ptr()), _lib.stream

    def refused(name, *args):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args, s())

    # C % 8, n % 8
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), None, None, None, p(out.t), None, None, None, 24, 12, 0)
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), None, None, None, p(out.t), None, None, None, 28, C, 0)
    # q8 without a slot; residual_bn without a residual, or without its shift; nothing to write
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), None, None, None, p(out.t), None, p(q8.t), None, 32, C, 0)
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), None, p(sc), p(sh), p(out.t), None, None, None, 32, C, 0)
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), p(y), p(sc), None, p(out.t), None, None, None, 32, C, 0)
    refused("ttdk_bn_apply", p(y), p(sc), p(sh), None, None, None, None, None, None, None, 32, C, 0)
    coef = torch.zeros(3, 16, device=DEV)
    refused("ttdk_bn_bwd_apply", p(y), None, None, p(y), p(coef), p(out.t), 24, 12)
    refused("ttdk_bn_bwd_apply", p(y), None, None, p(y), p(coef), p(out.t), 28, C)
    refused("ttdk_bn_bwd_apply_q8", p(y), None, None, p(y), p(coef), p(out.t), p(q8.t), None, 32, C)
    refused("ttdk_bn_bwd_apply_q8", p(y), None, None, p(y), p(coef), None, None, None, 32, C)
    refused("ttdk_bn_stats_partial", p(y), 2, 12, p(part.t), 1)
    refused("ttdk_bn_bwd_partial", p(y), None, None, p(y), 2, 12, p(part.t), 1, None)
    with pytest.raises(ValueError):
        K.bn_apply(y, sc, sh, store_out=False)
    torch.cuda.synchronize()
    assert out.untouched() and q8.untouched() and part.untouched()


def test_zz_report_gpu_maxima():
    """Runs last in this file: the largest figure of the tests above beside its bar."""
    for k in sorted(_seen):
        print("%-14s gpu max %.3e   bar %.1e" % (k, _seen[k], O.BARS[k]))
    assert set(_seen) <= set(O.BARS)
