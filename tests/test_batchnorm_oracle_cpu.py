"""The float64 reference of tests/batchnorm_oracle.py, checked on the CPU against independent
statements of the same operations (F.batch_norm in training mode with ReLU and a residual under
double autograd, one case worked out by hand, the running statistics by value); then the
reference run in float32 against itself in float64 on the case tables of
tests/test_batchnorm_kernels.py: those maxima, times O.MARGIN, are the bars of the GPU tests (run
with -s to see them)."""
import pytest
import torch

import batchnorm_oracle as O

F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("residual,relu,affine", [(True, True, True), (False, True, True), (False, False, True),
                                                  (True, True, False)])
def test_oracle_matches_torch_double_autograd(residual, relu, affine):
    M, C, eps = 37, 16, 1e-5
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(M, C, generator=gen, dtype=F64) * 2 + 1
    res = torch.randn(M, C, generator=gen, dtype=F64) if residual else None
    dy = torch.randn(M, C, generator=gen, dtype=F64)
    gamma = torch.randn(C, generator=gen, dtype=F64) if affine else None
    beta = torch.randn(C, generator=gen, dtype=F64) if affine else None
    st = O.fwd_stats(y, gamma, beta, eps)
    out = O.apply(y, st["scale"], st["shift"], residual=res, relu=relu)
    g = O.relu_grad(dy, out > 0 if relu else None)
    dz, dgamma, dbeta = O.bwd_direct(g, y, st["mean"], st["rstd"], gamma)

    ya = y.clone().requires_grad_(True)
    ga = gamma.clone().requires_grad_(True) if affine else None
    ba = beta.clone().requires_grad_(True) if affine else None
    ra = res.clone().requires_grad_(True) if residual else None
    z = torch.nn.functional.batch_norm(ya, None, None, ga, ba, training=True, eps=eps)
    z = z + ra if residual else z
    oa = torch.relu(z) if relu else z
    oa.backward(dy)
    kw = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(st["mean"], y.mean(0), **kw)
    torch.testing.assert_close(st["var"], y.var(0, unbiased=False), **kw)
    torch.testing.assert_close(out, oa.detach(), **kw)
    torch.testing.assert_close(dz, ya.grad, **kw)
    if affine:
        torch.testing.assert_close(dgamma, ga.grad, **kw)
        torch.testing.assert_close(dbeta, ba.grad, **kw)
    if residual:
        torch.testing.assert_close(g, ra.grad, **kw)
    # the split form: sums, coef rows, dz = a*g + b*y + c; and accumulate
    dg0, db0 = torch.randn(C, generator=gen, dtype=F64), torch.randn(C, generator=gen, dtype=F64)
    sg, sgy = O.bwd_sums(g, y)
    sp = O.bwd_coef(sg, sgy, M, st["mean"], st["rstd"], gamma, dg0, db0)
    torch.testing.assert_close(sp["dgamma"], dgamma + dg0, **kw)
    torch.testing.assert_close(sp["dbeta"], dbeta + db0, **kw)
    torch.testing.assert_close(O.dz_from_coef(sp["coef"], g, y), dz, **kw)
    _, dg1, db1 = O.bwd_direct(g, y, st["mean"], st["rstd"], gamma, dg0, db0)
    torch.testing.assert_close(dg1, dgamma + dg0, **kw)
    torch.testing.assert_close(db1, dbeta + db0, **kw)
    # the one-pass statistics and the statistics from sums are the same numbers in float64
    one = O.fwd_stats(y, gamma, beta, eps, one_pass=True)
    tot = O.stats_from_sums(y.sum(0), (y * y).sum(0), M, gamma, beta, eps)
    for k in st:
        torch.testing.assert_close(one[k], st[k], rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(tot[k], st[k], rtol=1e-11, atol=1e-12)
    # a residual that is itself a BN output: the two-step form
    if residual:
        rs, rh = torch.randn(C, generator=gen, dtype=F64), torch.randn(C, generator=gen, dtype=F64)
        both = O.apply(y, st["scale"], st["shift"], res, rs, rh, relu=relu)
        torch.testing.assert_close(both, O.apply(y, st["scale"], st["shift"], O.apply(res, rs, rh), relu=relu), **kw)


def test_one_case_by_hand():
    """M = 4, C = 8, eps = 0, every channel the column x = [1, 3, 5, 7] times (c + 1) for
    c = 0..3 and [2, 2, 4, 4] for c = 4..7. Column [1, 3, 5, 7]: mean 4, var (9 + 1 + 1 + 9)/4 = 5,
    rstd 1/sqrt5; times k: mean 4k, var 5k^2. Column [2, 2, 4, 4]: mean 3, var 1, rstd 1.
    gamma = 2, beta = 1: scale = 2*rstd, shift = 1 - mean*scale; channel 0: scale 2/sqrt5,
    shift 1 - 8/sqrt5; channel 4: scale 2, shift -5, out = 2x - 5 = [-1, -1, 3, 3], ReLU [0, 0, 3, 3].
    Backward in channel 4 with dy = [1, 2, 3, 4]: g = [0, 0, 3, 4], dbeta = 7, xhat = [-1, -1, 1, 1],
    dgamma = 7, dz = 2*(g - 7/4 - xhat*7/4) = 2*[0, 0, -1/2, 1/2] = [0, 0, -1, 1]. The sums:
    sg = 7, sgy = 28, dgamma = 1*(28 - 3*7) = 7; a = 2, b = -2*7/4 = -7/2, c = -2*7/4 + 7/2*3 = 7;
    a*g + b*y + c = [0 - 7 + 7, 0 - 7 + 7, 6 - 14 + 7, 8 - 14 + 7] = [0, 0, -1, 1].
    Channel 0 without ReLU, dy = [1, 0, 0, 1]: dbeta = 2, xhat = [-3, -1, 1, 3]/sqrt5, dgamma = 0,
    dz = (2/sqrt5)*([1, 0, 0, 1] - 1/2) = [1, -1, -1, 1]/sqrt5."""
    r5 = 5 ** 0.5
    a, b = torch.tensor([1.0, 3, 5, 7], dtype=F64), torch.tensor([2.0, 2, 4, 4], dtype=F64)
    x = torch.stack([a, 2 * a, 3 * a, 4 * a, b, b, b, b], 1)
    gamma, beta = torch.full((8,), 2.0, dtype=F64), torch.ones(8, dtype=F64)
    st = O.fwd_stats(x, gamma, beta, 0.0)
    assert torch.equal(st["mean"], torch.tensor([4.0, 8, 12, 16, 3, 3, 3, 3], dtype=F64))
    assert torch.equal(st["var"], torch.tensor([5.0, 20, 45, 80, 1, 1, 1, 1], dtype=F64))
    torch.testing.assert_close(st["rstd"], torch.tensor([1 / r5, 0.5 / r5, 1 / (3 * r5), 0.25 / r5, 1, 1, 1, 1],
                                                        dtype=F64), rtol=1e-15, atol=0)
    torch.testing.assert_close(st["scale"][[0, 4]], torch.tensor([2 / r5, 2.0], dtype=F64), rtol=1e-15, atol=0)
    torch.testing.assert_close(st["shift"][[0, 4]], torch.tensor([1 - 8 / r5, -5.0], dtype=F64), rtol=1e-14, atol=0)
    out = O.apply(x, st["scale"], st["shift"], relu=True)
    assert torch.equal(out[:, 4], torch.tensor([0.0, 0, 3, 3], dtype=F64))
    assert O.mask_bits(out.reshape(-1)[:8].clone()).tolist() == [0] and O.mask_bits(out[3]).tolist() == [0xFF]
    assert O.mask_bits(out[1]).tolist() == [0x0F]  # row 1: x = 3k -> 1 - 2/sqrt5 > 0; x = 2 -> -1
    dy = torch.tensor([1.0, 2, 3, 4], dtype=F64)[:, None].repeat(1, 8)
    g = O.relu_grad(dy, out > 0)
    assert torch.equal(g[:, 4], torch.tensor([0.0, 0, 3, 4], dtype=F64))
    dz, dgamma, dbeta = O.bwd_direct(g, x, st["mean"], st["rstd"], gamma)
    assert float(dbeta[4]) == 7 and float(dgamma[4]) == 7
    assert torch.equal(dz[:, 4], torch.tensor([0.0, 0, -1, 1], dtype=F64))
    sg, sgy = O.bwd_sums(g, x)
    assert float(sg[4]) == 7 and float(sgy[4]) == 28
    sp = O.bwd_coef(sg, sgy, 4, st["mean"], st["rstd"], gamma)
    assert sp["coef"][:, 4].tolist() == [2.0, -3.5, 7.0] and float(sp["dgamma"][4]) == 7
    assert torch.equal(O.dz_from_coef(sp["coef"], g, x)[:, 4], torch.tensor([0.0, 0, -1, 1], dtype=F64))
    dy0 = torch.tensor([1.0, 0, 0, 1], dtype=F64)[:, None].repeat(1, 8)
    dz, dgamma, dbeta = O.bwd_direct(O.relu_grad(dy0, None), x, st["mean"], st["rstd"], gamma)
    assert float(dbeta[0]) == 2 and abs(float(dgamma[0])) < 1e-15
    torch.testing.assert_close(dz[:, 0], torch.tensor([1.0, -1, -1, 1], dtype=F64) / r5, rtol=1e-14, atol=1e-15)
    # mask bits: element 8*i + j is bit j of byte i; -0 and 0 are not set
    v = torch.tensor([1.0, -1, 0.0, -0.0, 2, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 1e-30])
    m = O.mask_bits(v)
    assert m.tolist() == [0b10010001, 0b10000000]
    assert torch.equal(O.mask_bools(m, (16,)), v > 0)


def test_running_statistics_by_value():
    """M = 1: the batch variance is 0 and stays biased. M = 2, x = [1, 3]: mean 2, var 1, unbiased
    2. From moving mean 10 and variance 4 at momentum 0.75: 7.5 + 0.25*mean, 3 + 0.25*unbiased."""
    rm0, rv0 = torch.tensor([10.0], dtype=F64), torch.tensor([4.0], dtype=F64)
    st = O.fwd_stats(torch.tensor([[5.0]], dtype=F64), None, None, 0.25)
    assert float(st["mean"]) == 5 and float(st["var"]) == 0 and float(st["rstd"]) == 2
    assert float(st["scale"]) == 2 and float(st["shift"]) == -10
    rm, rv = O.running(rm0, rv0, st["mean"], st["var"], 1, 0.75)
    assert float(rm) == 8.75 and float(rv) == 3.0
    st = O.fwd_stats(torch.tensor([[1.0], [3.0]], dtype=F64), None, None, 0.0)
    assert float(st["mean"]) == 2 and float(st["var"]) == 1
    rm, rv = O.running(rm0, rv0, st["mean"], st["var"], 2, 0.75)
    assert float(rm) == 8.0 and float(rv) == 3.5


def test_case_tables_and_inputs():
    assert O.stats_Ms(8) == [1, 2, 255, 4096, 4097, 8194] and O.stats_Ms(2048) == [1, 2, 16, 17, 34]
    assert O.stats_Ms(24) == [1, 2, 84, 1360, 1361, 2722]
    assert O.apply_Ms(8) == [255, 1024, 1025, 3173] and O.apply_Ms(2048) == [1, 4, 5, 13]
    inp = O.apply_inputs(5, 8)
    rows = O.zero_rows(5)
    assert bool(torch.signbit(inp["y"][rows, 1].float()).all()) and bool(torch.signbit(inp["shift"][1]))
    assert float(inp["y"][0, 2]) == 2.0 ** -120 and float(inp["out"][:, O.CH_MASKED].max()) <= 0
    want = O.apply(inp["y"], inp["scale"], inp["shift"])
    assert float(want[0, 2]) == 2.0 ** -140 and float(want[0, 2].bfloat16()) == 0.0
    s = O.stats_inputs(300, 24)
    assert float(s["gamma"][O.CH_GAMMA0]) == 0 and float(s["gamma"][O.CH_GAMMA_NEG]) < 0
    assert bool((s["x"][:, O.CH_CONST] == 3).all()) and bool((s["x"][:, O.CH_ZERO] == 0).all())
    assert float(s["x"][150, O.CH_OUTLIER]) == 200
    assert torch.equal(O.stats_inputs(300, 24)["x"], s["x"])


# ------------------------------------------------------------------ float32 against float64
_maxima = {}


def _note(figs):
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
    return figs


def _hold(figs, label):
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in _note(figs).items():
        assert O.bar_holds(k, v), (label, k, v, O.BARS[k])


def _stats_fp32(x_or_sums, gamma, beta, rm0, rv0, M, scales_AQ):
    """Figures of the float32 statistics (one-pass) against the float64 ones, running statistics
    at momentum 0 (the batch values themselves: the `var` figure of the GPU tests) and MOMENTUM."""
    figs = {}
    for mom in (0.0, O.f32r(O.MOMENTUM)):
        if isinstance(x_or_sums, tuple):
            ref = O.stats_from_sums(*x_or_sums, M, gamma, beta, O.f32r(O.EPS))
            got = O.stats_from_sums(*(t.float() for t in x_or_sums), M, gamma, beta, O.f32r(O.EPS), dtype=F32)
        else:
            ref = O.fwd_stats(x_or_sums, gamma, beta, O.f32r(O.EPS))
            got = O.fwd_stats(x_or_sums, gamma, beta, O.f32r(O.EPS), dtype=F32)
        ref["run_mean"], ref["run_var"] = O.running(rm0, rv0, ref["mean"], ref["var"], M, mom)
        got["run_mean"], got["run_var"] = O.running(rm0, rv0, got["mean"], got["var"], M, mom, dtype=F32)
        sc = O.stats_scales(*scales_AQ, ref, gamma, beta, O.f32r(O.EPS), M, mom, rm0, rv0)
        for k, v in O.stats_figures(got, ref, sc).items():
            figs[k] = max(figs.get(k, 0.0), v)
    return figs


@pytest.mark.parametrize("C", O.STATS_C)
def test_fp32_statistics_within_bars(C):
    for M in O.stats_Ms(C):
        inp = O.stats_inputs(M, C)
        x = inp["x"]
        figs = _stats_fp32(x, inp["gamma"], inp["beta"], inp["rm0"], inp["rv0"], M, O.data_scales(x))
        T = max(1, min(2048, -(-M // (16 * O.rlanes(C)))))
        want, mag = O.block_sums(x, T)
        figs["bn_partial"] = O.figure(O.block_sums(x, T, dtype=F32)[0], want, mag)
        _hold(figs, ("stats", M, C))


@pytest.mark.parametrize("C", O.FOLD_C)
def test_fp32_folds_within_bars(C):
    for T in O.FOLD_T:
        inp = O.fold_inputs(T, C)
        p = inp["partial"]
        s, q, a_s, a_q = O.fold_truth(p)
        s32, q32 = p[:, 0].sum(0), p[:, 1].sum(0)
        figs = {"bn_sums": max(O.figure(s32, s, a_s), O.figure(q32, q, a_q))}
        # the fold in fp32, then the one-pass finalize in fp32
        eps, M = O.f32r(O.EPS), O.FOLD_COUNT
        ref = O.stats_from_sums(s, q, M, inp["gamma"], inp["beta"], eps)
        got = O.stats_from_sums(s32, q32, M, inp["gamma"], inp["beta"], eps, dtype=F32)
        mom = O.f32r(O.MOMENTUM)
        ref["run_mean"], ref["run_var"] = O.running(inp["rm0"], inp["rv0"], ref["mean"], ref["var"], M, mom)
        got["run_mean"], got["run_var"] = O.running(inp["rm0"], inp["rv0"], got["mean"], got["var"], M, mom, dtype=F32)
        sc = O.stats_scales(a_s / M, a_q / M, ref, inp["gamma"], inp["beta"], eps, M, mom, inp["rm0"], inp["rv0"])
        figs.update(O.stats_figures(got, ref, sc))
        for acc in (False, True):
            old = (inp["dg0"], inp["db0"]) if acc else (None, None)
            refb = O.bwd_coef(s, q, M, inp["mean"], inp["rstd"], inp["gamma"], *old)
            gotb = O.bwd_coef(s32, q32, M, inp["mean"], inp["rstd"], inp["gamma"], *old, dtype=F32)
            scb = O.bwd_scales(a_s, a_q, M, inp["mean"], inp["rstd"], inp["gamma"], *old)
            for k, v in O.bwd_figures(gotb, refb, scb).items():
                figs[k] = max(figs.get(k, 0.0), v)
        _hold(figs, ("fold", T, C))


@pytest.mark.parametrize("C", O.APPLY_C)
def test_fp32_apply_and_backward_within_bars(C):
    for M in O.apply_Ms(C):
        inp = O.apply_inputs(M, C)
        figs = {}
        for option in O.APPLY_OPTIONS:
            res, rs, rh, relu = O.apply_kwargs(inp, option)
            a = (inp["y"], inp["scale"], inp["shift"], res, rs, rh)
            v = O.figure(O.apply(*a, relu=relu, dtype=F32), O.apply(*a, relu=relu), O.apply_scale(*a))
            figs["bn_out"] = max(figs.get("bn_out", 0.0), v)
        for keep in (inp["out"].float() > 0, None):
            g = O.relu_grad(inp["dy"], keep)
            sg, sgy = O.bwd_sums(g, inp["y"])
            asg, asgy = O.bwd_sums(g.abs(), inp["y"].double().abs())
            for acc in (False, True):
                old = (inp["dg0"], inp["db0"]) if acc else (None, None)
                ref = O.bwd_coef(sg, sgy, M, inp["mean"], inp["rstd"], inp["gamma"], *old)
                got = O.bwd_coef(*O.bwd_sums(g, inp["y"], dtype=F32), M, inp["mean"], inp["rstd"], inp["gamma"], *old,
                                 dtype=F32)
                sc = O.bwd_scales(asg, asgy, M, inp["mean"], inp["rstd"], inp["gamma"], *old)
                for k, v in O.bwd_figures(got, ref, sc).items():
                    figs[k] = max(figs.get(k, 0.0), v)
            coef = ref["coef"].float()  # stands in for the kernel's own
            v = O.figure(O.dz_from_coef(coef, g, inp["y"], dtype=F32), O.dz_from_coef(coef, g, inp["y"]),
                         O.dz_scale(coef, g, inp["y"]))
            figs["bn_dz"] = max(figs.get("bn_dz", 0.0), v)
        _hold(figs, ("apply", M, C))


def e2e_fp32_figures(M, C):
    inp = O.e2e_inputs(M, C)
    eps = O.f32r(O.EPS)
    y, gamma = inp["y"], inp["gamma"]
    ref = O.fwd_stats(y, gamma, inp["beta"], eps)
    out = O.apply(y, ref["scale"], ref["shift"], residual=inp["res"], relu=True).bfloat16()
    g = O.relu_grad(inp["dy"], out.float() > 0)
    dz, dgamma, dbeta = O.bwd_direct(g, y, ref["mean"], ref["rstd"], gamma)
    st = O.fwd_stats(y, gamma, inp["beta"], eps, dtype=F32)
    got = O.bwd_coef(*O.bwd_sums(g, y, dtype=F32), M, st["mean"], st["rstd"], gamma, dtype=F32)
    sc = O.e2e_scales(y, g, ref, gamma, eps)
    return {"bn_e2e_dbeta": O.figure(got["dbeta"], dbeta, sc["e2e_dbeta"]),
            "bn_e2e_dgamma": O.figure(got["dgamma"], dgamma, sc["e2e_dgamma"]),
            "bn_e2e_dz": O.figure(O.dz_from_coef(got["coef"], g, y, dtype=F32), dz, sc["e2e_dz"])}


@pytest.mark.parametrize("M,C", O.E2E_CASES)
def test_fp32_end_to_end_within_bars(M, C):
    _hold(e2e_fp32_figures(M, C), ("e2e", M, C))


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars; every bar
    has a measured figure."""
    for k in sorted(_maxima):
        print("%-14s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        assert O.MARGIN * max(v, O.FLOOR) <= O.BARS[k]
