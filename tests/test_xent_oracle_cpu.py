"""The float64 reference of tests/xent_oracle.py, checked on the CPU against independent
statements of the same operations (F.cross_entropy with reduction="none" and its gradient under
double autograd, torch.topk, rows worked out by hand); then the reference run in float32 against
itself in float64 on the case tables of tests/test_xent_kernels.py: those maxima, times O.MARGIN,
are the bars of the GPU tests (run with -s to see them)."""
import math

import pytest
import torch
import torch.nn.functional as F

import xent_oracle as O

F32, F64 = torch.float32, torch.float64
INF = float("inf")


@pytest.mark.parametrize("V", (1, 2, 10, 257))
def test_oracle_matches_torch_double_autograd(V):
    gen = torch.Generator().manual_seed(V)
    rows = 9
    z = torch.randn(rows, V, generator=gen, dtype=F64) * 3
    labels = torch.randint(0, V, (rows,), generator=gen)
    up = torch.randn(rows, generator=gen, dtype=F64)
    ref = O.xent(z, labels, 0.25)
    za = z.clone().requires_grad_(True)
    loss = F.cross_entropy(za, labels, reduction="none")
    loss.backward(up)
    kw = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["loss"], loss.detach(), **kw)
    torch.testing.assert_close(ref["grad"] * 4 * up[:, None], za.grad, **kw)
    torch.testing.assert_close(ref["sums"][0], loss.detach().mean(), **kw)
    assert torch.equal(ref["correct"], z.argmax(1) == labels)  # tie-free
    assert float(ref["sums"][1]) == float((z.argmax(1) == labels).double().mean())
    for k in (1, 2, 5):
        top = torch.topk(z, min(k, V), dim=1).indices
        assert torch.equal(O.in_top_k(z, labels, k), (top == labels[:, None]).any(1))


def test_rows_by_hand():
    """V = 4. Row 0 [0, 0, 0, 0], label 2: loss log 4, grad 1/4 - onehot, correct (a tie at the
    maximum is correct). Row 1 [1, 3, 3, 2], label 3: two logits are greater: not correct, in the top
    3 but not the top 2. Row 2 [0, -inf, 0, 0], label 1: loss +inf, grad [1/3, -1, 1/3, 1/3], not
    correct for any k. Row 3 [5, 1, 1, 1], label 4 (outside): loss NaN, not correct. Row 4
    [log 1, log 2, log 3, log 4], label 3: se = 10/4, loss = log 10 - log 4, softmax i/10."""
    z = torch.tensor([[0.0, 0, 0, 0], [1, 3, 3, 2], [0, -INF, 0, 0], [5, 1, 1, 1],
                      [0.0, math.log(2), math.log(3), math.log(4)]], dtype=F64)
    labels = torch.tensor([2, 3, 1, 4, 3])
    ref = O.xent(z, labels, 2.0)
    assert abs(float(ref["loss"][0]) - math.log(4)) < 1e-15
    assert ref["grad"][0].tolist() == [0.5, 0.5, -1.5, 0.5]
    assert ref["correct"].tolist() == [True, False, False, False, True]
    assert float(ref["loss"][2]) == INF and math.isnan(float(ref["loss"][3]))
    torch.testing.assert_close(ref["grad"][2], torch.tensor([2 / 3, -2.0, 2 / 3, 2 / 3], dtype=F64), rtol=1e-15, atol=0)
    assert abs(float(ref["loss"][4]) - math.log(2.5)) < 1e-15
    torch.testing.assert_close(ref["grad"][4], torch.tensor([0.2, 0.4, 0.6, 0.8 - 2], dtype=F64), rtol=1e-14, atol=0)
    assert math.isnan(float(ref["sums"][0])) and float(ref["sums"][1]) == 0.4
    assert ref["valid"].tolist() == [True, True, True, False, True]
    # scales: row 4 |max| + |log se| + |z_l| = log 4 + log(10/4) + log 4
    assert abs(float(ref["loss_scale"][4]) - (2 * math.log(4) + math.log(2.5))) < 1e-14
    assert [O.in_top_k(z, labels, k).tolist() for k in (1, 2, 3)] == [
        [True, False, False, False, True], [True, False, False, False, True], [True, True, False, False, True]]
    assert O.in_top_k(z, torch.tensor([-1, 0, 0, 0, 0]), 4).tolist() == [False, True, True, True, True]
    # finite_figure: +inf and NaN must be met as they are
    fig, same = O.finite_figure(ref["loss"].float(), ref["loss"], ref["loss_scale"])
    assert same and fig < 1e-7
    bad = ref["loss"].clone()
    bad[2] = 1e30
    assert not O.finite_figure(bad, ref["loss"], ref["loss_scale"])[1]


def test_case_tables_and_inputs():
    for V in O.XENT_V:
        for dtype in O.XENT_DTYPES:
            z, labels = O.xent_inputs(V, 7, dtype)
            ref = O.xent(z, labels, 1.0)
            assert int(labels[0]) == 0 and int(labels[1]) == V - 1
            want = [None, None, True, V == 1, None, V == 1, True]
            for i, w in enumerate(want):
                assert w is None or bool(ref["correct"][i]) == w, (V, dtype, i)
            if V > 1:
                assert float(ref["loss"][O.ROW_NEGINF]) == INF and float(ref["sums"][0]) == INF
                assert float(z[4].float().max()) == 80 and float(z[4].float().min()) == -80
            fin = O.xent(z, O.finite_labels(z, labels), 1.0)
            assert bool(torch.isfinite(fin["loss"]).all()) and math.isfinite(float(fin["sums"][0]))
            assert abs(float(ref["loss"][6]) - math.log(V)) < 1e-10  # 32768 + log V - 32768 in float64
            assert torch.equal(O.xent_inputs(V, 7, dtype)[0], z)
    kinds = {O.PLANTS[V % 7] for V in O.XENT_V}
    assert len(kinds) >= 5  # the one-row cases see most plants
    z, labels = O.bad_label_inputs(10, F32)
    assert labels[2] == -1 and labels[5] == 10
    z, t = O.topk_inputs(65, 9, torch.bfloat16)
    assert float(z[1, t[1]]) == -INF and float(z[2, t[2]]) == INF and math.isnan(float(z[3, t[3]]))
    assert O.in_top_k(z, t, 1).tolist()[1:5] == [False, False, False, True]


# ------------------------------------------------------------------ float32 against float64
_maxima = {}


def _hold(figs, label):
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
        assert O.bar_holds(k, v), (label, k, v, O.BARS[k])


def fp32_figures(z, labels, gs):
    ref = O.xent(z, labels, gs)
    got = O.xent(z, labels, gs, dtype=F32)
    assert torch.equal(ref["correct"], got["correct"])
    g, _ = O.finite_figure(got["grad"], ref["grad"], abs(gs))
    l, same = O.finite_figure(got["loss"], ref["loss"], ref["loss_scale"])
    assert same
    fin_labels = O.finite_labels(z, labels)
    ref2, got2 = O.xent(z, fin_labels, gs), O.xent(z, fin_labels, gs, dtype=F32)
    return {"sx_grad": g, "sx_loss": l,
            "sx_mean_loss": O.figure(got2["sums"][0], ref2["sums"][0], ref2["sum_scale"])}


@pytest.mark.parametrize("V", O.XENT_V)
def test_fp32_xent_within_bars(V):
    for dtype in O.XENT_DTYPES:
        for rows in O.XENT_ROWS:
            z, labels = O.xent_inputs(V, rows, dtype)
            for gs in O.grad_scales(rows):
                _hold(fp32_figures(z, labels, gs), ("xent", V, rows, dtype, gs))


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars; every bar
    has a measured figure."""
    for k in sorted(_maxima):
        print("%-14s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        assert O.MARGIN * max(v, O.FLOOR) <= O.BARS[k]
