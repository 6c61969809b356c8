"""The float64 reference of tests/transformer_oracle.py, checked on the CPU against independent
statements of the same operations (F.layer_norm with double autograd, F.cross_entropy in double,
index_add_, a LayerNorm backward worked out by hand); then the reference run in float32 against
itself in float64 on the case tables of tests/test_transformer_rows.py: those maxima, times
O.MARGIN, are the bars of the GPU tests (run with -s to see them)."""
import pytest
import torch

import transformer_oracle as O

F64 = torch.float64


def _ln_case(rows=6, H=16, p_in=0.1, p_out=0.2, residual=True, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=gen, dtype=F64)
    res = torch.randn(rows, H, generator=gen, dtype=F64) if residual else None
    dy = torch.randn(rows, H, generator=gen, dtype=F64)
    gamma = torch.randn(H, generator=gen, dtype=F64) * 0.5 + 1
    beta = torch.randn(H, generator=gen, dtype=F64)
    kin = O.keep(3, 1, 11, p_in, rows, H)
    kout = O.keep(3, 1, 12, p_out, rows, H)
    return x, res, dy, gamma, beta, kin, kout


@pytest.mark.parametrize("residual,p_in,p_out", [(True, 0.1, 0.2), (False, 0.0, 0.1), (True, 0.1, 0.0),
                                                 (False, 0.0, 0.0)])
def test_layernorm_matches_torch_double_autograd(residual, p_in, p_out):
    eps = 1e-5
    x, res, dy, gamma, beta, kin, kout = _ln_case(p_in=p_in, p_out=p_out, residual=residual)
    s = O.ln_s(x, res, kin, p_in)
    mean, rstd = O.ln_stats(s, eps)
    y = O.ln_y(s, mean, rstd, gamma, beta, kout, p_out)
    ds, dx, dg, db = O.ln_bwd(dy, s, mean, rstd, gamma, kin, p_in, kout, p_out)
    xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True) if residual else None
    sa = xa * kin / (1 - p_in) + (ra if residual else 0)
    ya = torch.nn.functional.layer_norm(sa, (x.shape[1],), ga, ba, eps) * kout / (1 - p_out)
    ya.backward(dy)
    kw = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(s, sa.detach(), **kw)
    torch.testing.assert_close(y, ya.detach(), **kw)
    torch.testing.assert_close(mean, sa.detach().mean(1), **kw)
    torch.testing.assert_close(rstd, 1 / torch.sqrt(sa.detach().var(1, unbiased=False) + eps), **kw)
    torch.testing.assert_close(dx, xa.grad, **kw)
    if residual:
        torch.testing.assert_close(ds, ra.grad, **kw)
    torch.testing.assert_close(dg, ga.grad, **kw)
    torch.testing.assert_close(db, ba.grad, **kw)
    if p_out > 0:
        assert not bool(kout.all()) and not bool((~kout).all())


def test_layernorm_backward_by_hand():
    """2 x 4, eps = 0, no dropout. Row 0: s = [1, 3, 5, 7]: mean 4, var 5, xh = [-3, -1, 1, 3]/sqrt5.
    gamma = [1, 2, 1, 2], dy = [1, 0, 0, 1]: g = [1, 0, 0, 2], m1 = 3/4,
    m2 = (-3 + 6)/(4 sqrt5) = 3/(4 sqrt5); xh*m2 = [-9, -3, 3, 9]/20;
    ds = (g - m1 - xh*m2)/sqrt5 = [0.7, -0.6, -0.9, 0.8]/sqrt5.
    Row 1: s = [2, 2, 4, 4]: mean 3, var 1, xh = [-1, -1, 1, 1]; dy = [2, 0, 0, 0]: g = [2, 0, 0, 0],
    m1 = 1/2, m2 = -1/2, ds = [2 - 1/2 - 1/2, -1/2 - 1/2, -1/2 + 1/2, -1/2 + 1/2] = [1, -1, 0, 0].
    dgamma = sum_r dy*xh = [-3/sqrt5 - 2, 0, 0, 3/sqrt5]; dbeta = [3, 0, 0, 1]."""
    s = torch.tensor([[1.0, 3, 5, 7], [2, 2, 4, 4]], dtype=F64)
    gamma = torch.tensor([1.0, 2, 1, 2], dtype=F64)
    dy = torch.tensor([[1.0, 0, 0, 1], [2, 0, 0, 0]], dtype=F64)
    ones = torch.ones(2, 4, dtype=torch.bool)
    mean, rstd = O.ln_stats(s, 0.0)
    r5 = 5 ** 0.5
    torch.testing.assert_close(mean, torch.tensor([4.0, 3.0], dtype=F64), rtol=0, atol=0)
    torch.testing.assert_close(rstd, torch.tensor([1 / r5, 1.0], dtype=F64), rtol=1e-15, atol=0)
    ds, dx, dg, db = O.ln_bwd(dy, s, mean, rstd, gamma, ones, 0.0, ones, 0.0)
    want = torch.tensor([[0.7 / r5, -0.6 / r5, -0.9 / r5, 0.8 / r5], [1, -1, 0, 0]], dtype=F64)
    torch.testing.assert_close(ds, want, rtol=1e-14, atol=1e-15)
    assert torch.equal(dx, ds)
    torch.testing.assert_close(dg, torch.tensor([-3 / r5 - 2, 0, 0, 3 / r5], dtype=F64), rtol=1e-14, atol=1e-15)
    assert torch.equal(db, torch.tensor([3.0, 0, 0, 1], dtype=F64))
    # an input dropout of 1/2 that drops column 0: dx = 2*ds elsewhere, 0 there
    kin = torch.tensor([[False, True, True, True]] * 2)
    _, dx, _, _ = O.ln_bwd(dy, s, mean, rstd, gamma, kin, 0.5, ones, 0.0)
    torch.testing.assert_close(dx, torch.where(kin, 2 * want, torch.zeros_like(want)), rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("V,ld", [(5, 8), (1000, 1024)])
def test_xent_matches_torch_double(V, ld):
    logits, labels = O.xent_inputs(V, ld)
    gsc, msc = 0.37, 0.25
    loss, correct, grad, sums = O.xent(logits, V, labels, gsc, msc)
    z = logits[:, :V].double().requires_grad_(True)
    per = torch.nn.functional.cross_entropy(z, labels.long(), ignore_index=-1, reduction="none")
    torch.testing.assert_close(loss, per.detach(), rtol=1e-12, atol=1e-12)
    (per.sum() * gsc).backward()
    torch.testing.assert_close(grad[:, :V], z.grad, rtol=1e-11, atol=1e-15)
    assert float(grad[:, V:].abs().sum()) == 0 and float(grad[2].abs().sum()) == 0 and float(loss[2]) == 0
    valid = labels >= 0
    zz = logits[:, :V].double()
    # strictly greater: a tie at the label (row 3) counts as correct, argmax may name the other one
    want = torch.tensor([float(valid[r]) * float(zz[r, labels[r]] == zz[r].max()) for r in range(O.XENT_ROWS)],
                        dtype=F64)
    assert torch.equal(correct, want) and float(correct[3]) == 1.0
    assert int((zz[3] == zz[3].max()).sum()) == 2
    assert sums[0] == pytest.approx(float(per.detach().sum()) * msc, rel=1e-12)
    assert sums[1] == float(want.sum()) * msc
    assert float(zz[4].max()) == 80 and float(zz[4].min()) == -80


def test_embedding_matches_index_add():
    inp = O.embed_inputs(128, 4)
    B, S = O.EMBED_B, O.EMBED_S
    rows = B * S
    s = O.embed_fwd(inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S)
    want = (inp["word"].double().index_select(0, inp["ids"].long())
            + inp["pos"].double().repeat(B, 1) + inp["typ"].double().index_select(0, inp["tt"].long()))
    assert torch.equal(s, want)
    ds = inp["ds"].double()
    for pos_beta in (0, 1):
        dw, dp, dt = O.embed_bwd(inp["ds"], inp["ids"], inp["tt"], inp["dword0"], inp["dpos0"], 4, B, S, pos_beta)
        kw = dict(rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dw, inp["dword0"].double().index_add_(0, inp["ids"].long(), ds), **kw)
        torch.testing.assert_close(dp, ds.view(B, S, -1).sum(0) + pos_beta * inp["dpos0"].double(), **kw)
        torch.testing.assert_close(dt, torch.zeros(4, 128, dtype=F64).index_add_(0, inp["tt"].long(), ds), **kw)
    assert torch.equal(dw[O.EMBED_V - 2:], inp["dword0"].double()[O.EMBED_V - 2:])
    # without token types every row is type 0
    _, _, dt = O.embed_bwd(inp["ds"], inp["ids"], None, inp["dword0"], inp["dpos0"], 1, B, S, 0)
    torch.testing.assert_close(dt[0], ds.sum(0), rtol=1e-12, atol=1e-12)
    assert rows == 1161


def test_gather_scatter_count_activations_by_value():
    src = torch.arange(24.0).view(12, 2)
    pos = torch.tensor([2, 0, 3, 1], dtype=torch.int32)  # [B = 2, P = 2] positions in sequences of 6
    assert torch.equal(O.gather_rows(src, pos, group=(2, 6)), src[[2, 0, 9, 7]])
    assert torch.equal(O.gather_rows(src, None, group=(1, 6), n=2), src[[0, 6]])
    g = src[[2, 0, 9, 7]]
    out = O.scatter_rows(g, pos, torch.zeros(12, 2), group=(2, 6))
    assert torch.equal(out[[2, 0, 9, 7]], g.double()) and float(out.sum()) == float(g.sum())
    out = O.scatter_rows(g, pos, torch.ones(12, 2), accumulate=True, group=(2, 6))
    assert torch.equal(out[[2, 0, 9, 7]], g.double() + 1) and float(out[1].sum()) == 2.0
    assert O.count_valid(torch.tensor([1, -1, 0, -5]), 3.0) == (1.5,)
    assert O.count_valid(torch.tensor([-1, -1]), 3.0, both=True) == (1.0, 3.0)
    x = torch.linspace(-4, 4, 33, dtype=F64).requires_grad_(True)
    (0.5 * x * (1 + torch.tanh(O.K0 * (x + O.K1 * x ** 3)))).sum().backward()
    torch.testing.assert_close(O.dgelu(x.detach()), x.grad, rtol=1e-12, atol=1e-14)
    a = torch.tanh(x.detach())
    torch.testing.assert_close(O.dact(torch.full_like(a, 2.0), a, 1), 2 / torch.cosh(x.detach()) ** 2,
                               rtol=1e-10, atol=1e-14)
    h = torch.tensor([0.25, 1.0, 1.5], dtype=F64)
    assert torch.equal(O.bf16_half_ulp(h), torch.tensor([2.0 ** -10, 2.0 ** -8, 2.0 ** -8], dtype=F64))


# ------------------------------------------------------------------ float32 against float64
_maxima = {}


def _note(figs):
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
    return figs


def _ln_fp32_figures(mode, H, rows, accumulate=False):
    inp = O.ln_inputs(mode, H, rows)
    kin, kout = O.ln_masks(mode, H, rows)
    p_in = O.LN_MODES[mode][1]
    s64 = O.ln_s(inp["x"], inp["res"], kin, p_in)
    fig_s = O.figure(O.ln_s(inp["x"], inp["res"], kin, p_in, dtype=torch.float32), s64,
                     O.ln_s_scale(inp["x"], inp["res"], p_in))
    s = s64.bfloat16()  # stands in for the kernel's s
    dg0 = db0 = None
    if accumulate:
        dg0, db0 = torch.randn(H, generator=O._gen(H, 99)), torch.randn(H, generator=O._gen(H, 98))
    # float64 statistics rounded to fp32 stand in for the ones the forward kernel hands the backward
    stats = tuple(t.float() for t in O.ln_stats(s, O.LN_MODES[mode][3]))
    ref = O.ln_reference(mode, inp, kin, kout, s, stats, dg0, db0)
    got = O.ln_reference(mode, inp, kin, kout, s, stats, dg0, db0, dtype=torch.float32)
    return dict(O.ln_figures(got, ref, O.ln_scales(mode, inp, kout, s, ref, stats, dg0, db0)), ln_s=fig_s)


@pytest.mark.parametrize("mode,H,rows", O.LN_GRID + O.LN_ENGINE + O.LN_EXTRA + O.LN_PREFETCH0[:1])
def test_fp32_layernorm_within_bars(mode, H, rows):
    figs = _note(_ln_fp32_figures(mode, H, rows, accumulate=(mode, H, rows) == ("layer", 1024, 77)))
    print(mode, H, rows, figs)
    for k, v in figs.items():
        assert O.bar_holds(k, v), (k, v, O.BARS[k])


def test_fp32_small_kernels_within_bars():
    f32 = torch.float32
    figs = {}

    def put(name, v):
        figs[name] = max(figs.get(name, 0.0), v)

    for V, ld in O.XENT_CASES:
        z, labels = O.xent_inputs(V, ld)
        for gsc, msc in ((1.0 / 6, 1.0 / 6), (0.37, 1.0)):
            _, _, grad, sums = O.xent(z, V, labels, gsc, msc)
            _, _, g32, s32 = O.xent(z, V, labels, gsc, msc, dtype=f32)
            sl, sc = O.xent_scales(z, V, labels, msc)
            put("xent_grad", O.figure(g32, grad, gsc))
            put("xent_loss", abs(s32[0] - sums[0]) / sl)
            put("xent_correct", abs(s32[1] - sums[1]) / sc)
    for n in O.COUNT_N:
        for got, want in zip((torch.tensor(3.0, dtype=f32) / max(1, n - n // 3),), (3.0 / max(1, n - n // 3),)):
            put("count", abs(float(got) - want) / want)
    for H in O.EMBED_H + (4096,):
        inp = O.embed_inputs(H, 4)
        B, S = O.EMBED_B, O.EMBED_S
        a = (inp["ids"], inp["tt"], inp["word"], inp["pos"], inp["typ"], S)
        scale = (inp["word"].double().abs()[inp["ids"].long()] + inp["pos"].double().abs().repeat(B, 1)
                 + inp["typ"].double().abs()[inp["tt"].long()])
        put("emb_s", O.figure(O.embed_fwd(*a, dtype=f32), O.embed_fwd(*a), scale))
        if H > 2048:
            continue
        b = (inp["ds"], inp["ids"], inp["tt"], inp["dword0"], inp["dpos0"], 4, B, S, 1)
        scales = O.embed_bwd_abs(*b)
        for name, g, w, sc in zip(("emb_dword", "emb_dpos", "emb_dtype"), O.embed_bwd(*b, dtype=f32), O.embed_bwd(*b),
                                  scales):
            put(name, O.figure(g, w, sc))
    for H in O.GATHER_H:
        gen = O._gen(H, 5)
        src, dst = torch.randn(13, H, generator=gen).bfloat16(), torch.randn(40, H, generator=gen).bfloat16()
        idx = torch.randperm(40, generator=gen)[:13].int()
        put("scatter", O.figure(O.scatter_rows(src, idx, dst, True, dtype=f32), O.scatter_rows(src, idx, dst, True),
                                O.scatter_rows(src.abs(), idx, dst.abs(), True)))
    for n8 in O.DACT_N8:
        x, dy = O.act_inputs(n8 * 8)
        put("dact", O.figure(O.dact(dy, x, 0, dtype=f32), O.dact(dy, x, 0), dy.double().abs()))
        a, dy = O.tanh_outputs(n8 * 8)
        put("dact", O.figure(O.dact(dy, a, 1, dtype=f32), O.dact(dy, a, 1), dy.double().abs()))
    for n in O.TANH_N:
        x, _ = O.act_inputs(n)
        put("tanh", O.figure(O.tanh(x, dtype=f32), O.tanh(x), 1.0))
    print(_note(figs))
    for k, v in figs.items():
        assert O.bar_holds(k, v), (k, v, O.BARS[k])


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars."""
    for k in sorted(_maxima):
        print("%-14s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) <= set(O.BARS)
