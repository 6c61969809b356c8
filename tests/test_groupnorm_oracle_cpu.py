"""The float64 oracle of the group normalisation tests (groupnorm_oracle.py), checked without a GPU:
against torch's own group_norm under float64 autograd, against one case worked out by hand, and
run in float32 with the kernels' pivoted statistics against itself in float64 over the case
tables of tests/test_groupnorm.py. Those float32 maxima are what the bars stand on."""
import math

import pytest
import torch
import torch.nn.functional as F

import groupnorm_oracle as O

F64 = O.F64
_maxima = {}


def _torch_reference(x, gamma, beta, G, eps, dy):
    """F.group_norm on the channels-first permutation, float64, with autograd."""
    x = x.clone().requires_grad_(True)
    g = gamma.clone().requires_grad_(True) if gamma is not None else None
    b = beta.clone().requires_grad_(True) if beta is not None else None
    perm = (0, x.dim() - 1) + tuple(range(1, x.dim() - 1))
    inv = (0,) + tuple(range(2, x.dim())) + (1,)
    # an absent gamma is passed as constant ones: torch's backward of (weight None, bias given) fails
    w = g if g is not None else torch.ones(x.shape[-1], dtype=F64)
    y = F.group_norm(x.permute(perm), G, w, b, eps).permute(inv)
    y.backward(dy)
    return y.detach(), x.grad, None if g is None else g.grad, None if b is None else b.grad


@pytest.mark.parametrize("affine", ["both", "gamma", "beta", "none"])
@pytest.mark.parametrize("shape", [(5, 12), (3, 7, 12), (2, 3, 5, 12), (2, 2, 3, 2, 12)], ids=lambda s: "rank%d" % len(s))
@pytest.mark.parametrize("G", [1, 12, 3, 4])
def test_oracle_matches_torch_double_autograd(affine, shape, G):
    gen = torch.Generator().manual_seed(11 + len(shape) + G)
    C = shape[-1]
    x = torch.randn(shape, generator=gen, dtype=F64) * 2 + 1
    dy = torch.randn(shape, generator=gen, dtype=F64)
    gamma = torch.rand(C, generator=gen, dtype=F64) + 0.5 if affine in ("both", "gamma") else None
    beta = torch.randn(C, generator=gen, dtype=F64) if affine in ("both", "beta") else None
    eps = 1e-3
    y_t, dx_t, dg_t, db_t = _torch_reference(x, gamma, beta, G, eps, dy)
    x3, dy3 = x.reshape(shape[0], -1, C), dy.reshape(shape[0], -1, C)
    for pivoted in (False, True):
        # the definition, and operations 1 and 2 in float64: the same statistics
        mean, var, rstd = O.fold_stats(*O.col_sums(x3), x3.shape[1], G, eps) if pivoted else O.stats_def(x3, G, eps)
        y = O.apply(x3, mean, rstd, gamma, beta).reshape(shape)
        for dx, dg, db in (O.backward_def(dy3, x3, mean, rstd, gamma), O.backward(dy3, x3, mean, rstd, gamma)):
            assert float((y - y_t).abs().max()) <= 1e-12
            assert float((dx.reshape(shape) - dx_t).abs().max()) <= 1e-12
            if gamma is not None:
                assert float((dg - dg_t).abs().max()) <= 1e-12
            if beta is not None:
                assert float((db - db_t).abs().max()) <= 1e-12


def test_one_case_by_hand():
    """N = 1, M = 2, C = 4, G = 2, eps = 0. x = [[1, 3, 2, 2], [5, 7, 4, 4]]. Group 0 holds
    {1, 3, 5, 7}: mean 4, var (9 + 1 + 1 + 9) / 4 = 5, rstd 1/sqrt5, xh = (-3, -1, 1, 3)/sqrt5. Group 1
    holds {2, 2, 4, 4}: mean 3, var 1, rstd 1, xh = (-1, -1, 1, 1). gamma = [1, 2, 1, 1], beta = [0, 1, 0, 0]:
    y = [[-3/sqrt5, 1 - 2/sqrt5, -1, -1], [1/sqrt5, 1 + 6/sqrt5, 1, 1]].
    dy = [[1, 0, 1, 1], [0, 0, 1, 1]], m = 4. Group 0: A = 1, B = xh[0, 0] = -3/sqrt5, so
    dx = (gamma dy - 1/4 + xh * 3/(4 sqrt5)) / sqrt5 = (0.3, -0.4, -0.1, 0.2)/sqrt5 at (r0 c0, r0 c1, r1 c0,
    r1 c1). Group 1: A = 4, B = 0: dx = 1 - 4/4 = 0. dgamma = [-3/sqrt5, 0, 0, 0], dbeta = [1, 0, 2, 2].
    Pivots are row 0: S1 = [4, 4, 2, 2], S2 = [16, 16, 4, 4]."""
    s5 = math.sqrt(5.0)
    x = torch.tensor([[[1.0, 3, 2, 2], [5, 7, 4, 4]]], dtype=F64)
    dy = torch.tensor([[[1.0, 0, 1, 1], [0, 0, 1, 1]]], dtype=F64)
    gamma, beta = torch.tensor([1.0, 2, 1, 1], dtype=F64), torch.tensor([0.0, 1, 0, 0], dtype=F64)
    p, S1, S2 = O.col_sums(x)
    assert p.tolist() == [[1, 3, 2, 2]] and S1.tolist() == [[4, 4, 2, 2]] and S2.tolist() == [[16, 16, 4, 4]]
    for mean, var, rstd in (O.stats_def(x, 2, 0.0), O.fold_stats(p, S1, S2, 2, 2, 0.0)):
        assert torch.allclose(mean, torch.tensor([[4.0, 3.0]], dtype=F64), atol=1e-15, rtol=0)
        assert torch.allclose(var, torch.tensor([[5.0, 1.0]], dtype=F64), atol=1e-14, rtol=0)
        assert torch.allclose(rstd, torch.tensor([[1 / s5, 1.0]], dtype=F64), atol=1e-15, rtol=0)
    y = O.apply(x, mean, rstd, gamma, beta)
    want_y = torch.tensor([[[-3 / s5, 1 - 2 / s5, -1, -1], [1 / s5, 1 + 6 / s5, 1, 1]]], dtype=F64)
    assert torch.allclose(y, want_y, atol=1e-14, rtol=0)
    want_dx = torch.tensor([[[0.3 / s5, -0.4 / s5, 0, 0], [-0.1 / s5, 0.2 / s5, 0, 0]]], dtype=F64)
    for dx, dg, db in (O.backward_def(dy, x, mean, rstd, gamma), O.backward(dy, x, mean, rstd, gamma)):
        assert torch.allclose(dx, want_dx, atol=1e-14, rtol=0)
        assert torch.allclose(dg, torch.tensor([-3 / s5, 0, 0, 0], dtype=F64), atol=1e-14, rtol=0)
        assert db.tolist() == [1, 0, 2, 2]
    f = O.bwd_fold(*O.bwd_sums(dy, x, mean, rstd), mean, rstd, gamma, 2)
    assert torch.allclose(f["A"], torch.tensor([[1.0, 4.0]], dtype=F64), atol=1e-14, rtol=0)
    assert torch.allclose(f["B"], torch.tensor([[-3 / s5, 0.0]], dtype=F64), atol=1e-14, rtol=0)
    # accumulate: the old values are added
    _, dg, db = O.backward_def(dy, x, mean, rstd, gamma, dg0=torch.ones(4), db0=torch.full((4,), 2.0))
    assert torch.allclose(dg, torch.tensor([1 - 3 / s5, 1, 1, 1], dtype=F64), atol=1e-14, rtol=0)
    assert db.tolist() == [3, 2, 4, 4]


def test_case_tables():
    assert O.case_Ms(8, True) == [1, 2, 255, 257] and O.case_Ms(2056, True) == [1, 2, 7, 9]
    assert O.case_Ms(40, True) == [1, 2, 50, 52] and O.case_Ms(65, False) == [1, 2, 3, 5]
    assert O.CAP == 512
    cases = O.all_cases()
    assert len(set(cases)) == len(cases)
    for kind in O.VALUE_KINDS:
        assert any(c[5] == kind for c in cases)
    inp = O.inputs(2, 37, 16, 4, O.F32, "mean_far")
    g0 = inp["x"][:, :, :4].double()
    assert float(g0.mean()) > 990 and 0.5 < float(g0.std()) < 1.5
    inp = O.inputs(2, 37, 16, 4, O.BF16, "mean_far")
    assert inp["x"].dtype == O.BF16 and float(inp["x"][:, :, :4].double().mean()) > 99
    inp = O.inputs(2, 37, 16, 4, O.BF16, "const_group")
    assert bool((inp["x"][0, :, :4] == 3.0).all())
    assert float(O.inputs(2, 37, 16, 4, O.F32, "zero_image")["x"][0].abs().max()) == 0.0
    assert float(O.inputs(2, 37, 16, 4, O.F32, "gamma0")["gamma"][0]) == 0.0


def test_special_values_in_float64():
    """A constant group: var = 0, rstd = 1/sqrt(eps), y = beta; its dx is 0."""
    inp = O.inputs(2, 37, 16, 4, O.F32, "const_group")
    mean, var, rstd = O.stats_def(inp["x"], 4, O.EPS)
    assert float(var[0, 0]) == 0.0 and float(mean[0, 0]) == 3.0
    assert abs(float(rstd[0, 0]) - 1 / math.sqrt(O.EPS)) < 1e-12
    y = O.apply(inp["x"], mean, rstd, inp["gamma"], inp["beta"])
    assert torch.equal(y[0, :, :4], inp["beta"][:4].double().expand(37, 4))
    # the pivoted float32 sums are exactly zero there too
    m32, v32, r32 = O.stats(inp["x"], 4, O.f32r(O.EPS), O.F32)
    assert float(v32[0, 0]) == 0.0 and float(m32[0, 0]) == 3.0


@pytest.mark.parametrize("chunk", range(8))
def test_fp32_run_within_bars(chunk):
    cases = O.all_cases()[chunk::8]
    for case in cases:
        figs = O.fp32_figures(*case)
        for k, v in figs.items():
            _maxima[k] = max(_maxima.get(k, 0.0), v)
            assert O.bar_holds(k, v), (case, k, v, O.BARS[k])


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the test above beside their bars. Every bar has
    a measured figure, stands MARGIN above it (or above one fp32 rounding), and is no looser than
    rounding that product up to one digit makes it."""
    for k in sorted(_maxima):
        print("%-10s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        floor = O.MARGIN * max(v, O.FLOOR)
        assert floor <= O.BARS[k] <= 2 * floor, (k, v, O.BARS[k])
