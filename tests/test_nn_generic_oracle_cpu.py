"""The float64 reference of tests/nn_generic_oracle.py, checked on the CPU against independent
statements of the same operations (float64 autograd of the plain LayerNorm and inference-mode
BatchNorm formulas, F.embedding, index_add_, cases worked out by hand) and the conditions on its
inputs; then the reference run in float32 against itself in float64 on the case tables of
tests/test_nn_generic_kernels.py: those maxima, times O.MARGIN, are the bars of the GPU tests (run
with -s to see them). For the GEMM the float32 run is torch's float32 matmul of the same operands."""
import pytest
import torch

import nn_generic_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

_maxima = {}


def _hold(figs, label):
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
        assert O.bar_holds(k, v), (label, k, v, O.BARS[k])


def _clean(*ts):
    """No non-finite value in the inputs."""
    return all(bool(torch.isfinite(t.double()).all()) for t in ts if t is not None)


# ------------------------------------------------------------------ the oracle against other statements
@pytest.mark.parametrize("H,rows", [(1, 3), (7, 5), (100, 9)])
def test_layer_norm_matches_double_autograd(H, rows):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(rows, H, generator=gen, dtype=F64)
    dy = torch.randn(rows, H, generator=gen, dtype=F64)
    gamma, beta = torch.randn(H, generator=gen, dtype=F64), torch.randn(H, generator=gen, dtype=F64)
    eps = 1e-5
    mean, rstd = O.ln_stats(x, eps)
    xa, ga, ba = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    mu = xa.mean(1, keepdim=True)
    ya = (xa - mu) / torch.sqrt(((xa - mu) ** 2).mean(1, keepdim=True) + eps) * ga + ba
    ya.backward(dy)
    kw = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(O.ln_y(x, mean, rstd, gamma, beta), ya.detach(), **kw)
    torch.testing.assert_close(O.ln_y(x, mean, rstd, gamma, beta),
                               torch.nn.functional.layer_norm(x, (H,), gamma, beta, eps), **kw)
    torch.testing.assert_close(O.ln_dx(dy, x, mean, rstd, gamma), xa.grad, **kw)
    dg, db = O.ln_dparams(dy, x, mean, rstd)
    torch.testing.assert_close(dg, ga.grad, **kw)
    torch.testing.assert_close(db, ba.grad, **kw)
    # mode 2 of col_stats is the same dgamma / dbeta, block by block
    part, _ = O.col_stats(dy, 2, x, 2, mean, rstd)
    torch.testing.assert_close(part[:, 1].sum(0), dg, **kw)
    torch.testing.assert_close(part[:, 0].sum(0), db, **kw)


@pytest.mark.parametrize("affine", [(True, True), (False, True), (True, False), (False, False)])
def test_bn_inference_matches_double_autograd(affine):
    M, C, eps = 23, 6, 1e-3
    gen = torch.Generator().manual_seed(4)
    x, dy = torch.randn(M, C, generator=gen, dtype=F64), torch.randn(M, C, generator=gen, dtype=F64)
    mm, mv = torch.randn(C, generator=gen, dtype=F64), torch.rand(C, generator=gen, dtype=F64)
    gamma = torch.randn(C, generator=gen, dtype=F64) if affine[0] else None
    beta = torch.randn(C, generator=gen, dtype=F64) if affine[1] else None
    co = O.bn_infer_coef(mm, mv, gamma, beta, eps)
    xa = x.clone().requires_grad_(True)
    ga = (gamma if gamma is not None else torch.ones(C, dtype=F64)).clone().requires_grad_(True)
    ba = (beta if beta is not None else torch.zeros(C, dtype=F64)).clone().requires_grad_(True)
    ya = (xa - mm) / torch.sqrt(mv + eps) * ga + ba
    ya.backward(dy)
    kw = dict(rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(O.col_affine(x, co["scale"], c2=co["shift"]), ya.detach(), **kw)
    torch.testing.assert_close(O.col_affine(dy, co["scale"]), xa.grad, **kw)
    part, _ = O.col_stats(dy, 3, x, 1)
    got = O.bn_infer_bwd(part, mm, co["rstd"])
    torch.testing.assert_close(got["dgamma"], ga.grad, **kw)
    torch.testing.assert_close(got["dbeta"], ba.grad, **kw)


def test_small_cases_by_hand():
    """a = [[1, 2], [3, 4], [5, 6]] in T = 2 blocks of ceil(3/2) = 2 rows: block 0 holds rows 0 and
    1, block 1 row 2; T = 5: one row each, blocks 3 and 4 zeros."""
    a = torch.tensor([[1.0, 2], [3, 4], [5, 6]], dtype=F64)
    part, mag = O.col_stats(a, 2)
    assert part.tolist() == [[[4, 6], [10, 20]], [[5, 6], [25, 36]]] and torch.equal(part, mag)
    part, _ = O.col_stats(a, 5)
    assert part[2].tolist() == [[5, 6], [25, 36]] and float(part[3:].abs().sum()) == 0
    part, mag = O.col_stats(a, 1, -a, 1)
    assert part[0, 1].tolist() == [-35, -56] and mag[0, 1].tolist() == [35, 56]
    o, m = O.col_reduce2(torch.tensor([[[1.0], [2.0]], [[-3.0], [4.0]]]), torch.tensor([[10.0], [-20.0]]))
    assert o.tolist() == [[8.0], [-14.0]] and m.tolist() == [[14.0], [26.0]]
    # the affine forms
    c0, c1, c2 = (torch.tensor(v, dtype=F64) for v in ([2.0, 3], [10.0, 100], [0.5, 0.25]))
    assert O.col_affine(a, c0).tolist() == [[2, 6], [6, 12], [10, 18]]
    assert O.col_affine(a, c0, a, c1, c2)[2].tolist() == [60.5, 618.25]
    # LayerNorm of [1, 3]: mean 2, var 1; eps 3 -> rstd 1/2; a constant row: rstd = 1/sqrt(eps)
    mean, rstd = O.ln_stats(torch.tensor([[1.0, 3.0], [7.0, 7.0]], dtype=F64), 3.0)
    assert mean.tolist() == [2.0, 7.0] and float(rstd[0]) == 0.5 and float(rstd[1]) == 1 / 3.0 ** 0.5
    # BN inference: mv = 0 leaves eps under the root
    co = O.bn_infer_coef(torch.tensor([3.0]), torch.tensor([0.0]), torch.tensor([2.0]), None, 0.25)
    assert float(co["rstd"]) == 2 and float(co["scale"]) == 4 and float(co["shift"]) == -12
    # unary
    z = torch.tensor([0.0, float("inf"), -float("inf")], dtype=F64)
    assert O.unary(z, O.SIGMOID).tolist() == [0.5, 1.0, 0.0] and O.unary(z, O.TANH).tolist() == [0.0, 1.0, -1.0]
    assert float(O.unary_bwd(torch.tensor(2.0), torch.tensor(0.5), O.TANH)) == 1.5
    assert float(O.unary_bwd(torch.tensor(2.0), torch.tensor(0.25), O.SIGMOID)) == 0.375
    # GEMM with K = 0: bias + old C
    A, B = torch.zeros(2, 0), torch.zeros(0, 3)
    bias, C0 = torch.tensor([1.0, 2, 3]), torch.full((2, 3), 10.0)
    assert O.gemm(A, B, bias=bias, C0=C0).tolist() == [[11, 12, 13]] * 2
    assert O.gemm_scale(A, B, bias=-bias, C0=-C0).tolist() == [[11, 12, 13]] * 2
    A, B = torch.tensor([[1.0, 2], [3, 4]]), torch.tensor([[0.0, 1], [1, 0]])
    assert O.gemm(A, B).tolist() == [[2, 1], [4, 3]] and O.gemm(A, B, ta=True).tolist() == [[3, 1], [4, 2]]
    assert O.gemm(A, A, tb=True).tolist() == [[5, 11], [11, 25]]


@pytest.mark.parametrize("idtype", O.EMBED_IDS)
@pytest.mark.parametrize("V,H", O.EMBED_TABLES)
def test_gather_and_scatter_match_torch(V, H, idtype):
    for same in (False, True):
        inp = O.embed_inputs(V, H, idtype, F32, same)
        ids = inp["ids"]
        bad = O.out_of_range(V, idtype)
        assert ids[2, 1:1 + len(bad)].tolist() == bad and ids.dim() == 2
        flat = ids.reshape(-1).long()
        ok = (flat >= 0) & (flat < V)
        assert int((~ok).sum()) == len(bad)
        got = O.gather(inp["table"], ids)
        assert got.shape == ids.shape + (H,)
        g2 = got.reshape(-1, H)
        assert torch.equal(g2[ok], torch.nn.functional.embedding(flat[ok], inp["table"]))
        assert bool((g2[~ok] == 0).all())
        table, mag = O.scatter_add(inp["dy"], ids, inp["old"])
        want = inp["old"].double().index_add_(0, flat[ok], inp["dy"].reshape(-1, H)[ok].double())
        torch.testing.assert_close(table, want, rtol=1e-13, atol=1e-13)
        assert bool((mag >= table.abs() - 1e-12).all())
        if same:
            assert int((flat[ok] == V // 2).all())


def test_case_tables():
    for (M, C), want in O.PARTS_VALUES:
        assert O.col_stats_parts(M, C) == want
    assert [O.col_stats_parts(M, C) for M, C, _ in O.COL_STATS_CASES[:5]] == [1, 1, 1, 2, 5]
    assert all((O.AFFINE_ROWS * C) % 256 for C in O.AFFINE_C)
    n, C = O.AFFINE_WRAP
    assert n > 65536 * 256 and n % C == 1
    V, H, shape = O.GATHER_WRAP
    assert shape[0] * shape[1] * H > 2 ** 24
    assert {h for h, _ in O.LN_CASES} == {1, 2, 63, 64, 65, 100, 1000, 4097}
    assert {r for _, r in O.LN_CASES} == {1, 3, 4, 5, 77}
    cases = O.gemm_cases()
    assert {c[:3] for c in cases} == set(O.GEMM_SHAPES)
    for shape in O.GEMM_ALL_TRANS:
        assert {c[3:5] for c in cases if c[:3] == shape} == {(a, b) for a in (False, True) for b in (False, True)}
    assert torch.equal(O.ln_inputs(65, 77, F32)["x"], O.ln_inputs(65, 77, F32)["x"])


# ------------------------------------------------------------------ float32 against float64
@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("M,C,T", O.COL_STATS_CASES)
def test_fp32_col_stats_within_bars(M, C, T, dtype):
    T = T or O.col_stats_parts(M, C)
    inp = O.col_stats_inputs(M, C, dtype)
    assert _clean(*inp.values())
    figs = {"cs_part": 0.0}
    for mode in (0, 1, 2):
        args = (inp["a"], T, inp["b"], mode, inp["mu"], inp["rs"])
        want, mag = O.col_stats(*args)
        got, _ = O.col_stats(*args, dtype=F32)
        figs["cs_part"] = max(figs["cs_part"], O.figure(got, want, mag))
        if mode == 0 and C > 1:
            # the mean-64 column on its own, at the scale sum x^2
            c = O.CH_MEAN64
            assert abs(float(inp["a"][:, c].double().mean()) - 64) < 4
            assert O.bar_holds("cs_part", O.figure(got[:, 1, c], want[:, 1, c], mag[:, 1, c]))
    _hold(figs, ("col_stats", M, C, T, dtype))


def test_fp32_col_reduce2_within_bars():
    figs = {"cs_reduce": 0.0}
    for T in O.REDUCE_T:
        for C in O.REDUCE_C:
            inp = O.reduce_inputs(T, C)
            assert _clean(*inp.values())
            for old in (None, inp["old"]):
                want, mag = O.col_reduce2(inp["part"], old)
                got, _ = O.col_reduce2(inp["part"], old, dtype=F32)
                figs["cs_reduce"] = max(figs["cs_reduce"], O.figure(got, want, mag))
    _hold(figs, "col_reduce2")


def _affine_fp32(inp, form):
    b, c1, c2 = O.affine_args(inp, form)
    a = (inp["a"], inp["c0"], b, c1, c2)
    return O.figure(O.col_affine(*a, dtype=F32), O.col_affine(*a), O.col_affine_scale(*a))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_fp32_col_affine_within_bars(dtype):
    figs = {"cs_affine": 0.0}
    for C in O.AFFINE_C:
        inp = O.affine_inputs(O.AFFINE_ROWS, C, dtype)
        assert _clean(*inp.values())
        for form in O.AFFINE_FORMS:
            figs["cs_affine"] = max(figs["cs_affine"], _affine_fp32(inp, form))
    _hold(figs, ("col_affine", dtype))


def test_fp32_col_affine_wrap_within_bars():
    inp, n = O.affine_wrap_inputs()
    assert inp["a"].numel() >= n > inp["a"].numel() - O.AFFINE_WRAP[1]
    fig, step = 0.0, 1 << 20  # in chunks of rows: the float64 copies stay small
    for lo in range(0, inp["a"].shape[0], step):
        part = dict(inp, a=inp["a"][lo:lo + step], b=inp["b"][lo:lo + step])
        fig = max(fig, _affine_fp32(part, "b_c1_c2"))
    _hold({"cs_affine": fig}, "col_affine wrap")


def test_fp32_bn_inference_within_bars():
    figs = {}
    eps = O.f32r(O.EPS_BN)
    for C in O.BNI_C:
        for T in O.BNI_T:
            inp = O.bni_inputs(C, T)
            assert _clean(*inp.values()) and float(inp["mv"][0]) == 0
            for gamma in (inp["gamma"], None):
                for beta in (inp["beta"], None):
                    a = (inp["mm"], inp["mv"], gamma, beta, eps)
                    want, got, sc = O.bn_infer_coef(*a), O.bn_infer_coef(*a, dtype=F32), O.bn_infer_coef_scales(*a)
                    for k in want:
                        figs["bni_" + k] = max(figs.get("bni_" + k, 0.0), O.figure(got[k], want[k], sc[k]))
            a = (inp["part"], inp["mm"], inp["rstd"])
            want, got, sc = O.bn_infer_bwd(*a), O.bn_infer_bwd(*a, dtype=F32), O.bn_infer_bwd_scales(*a)
            for k in want:
                figs["bni_" + k] = max(figs.get("bni_" + k, 0.0), O.figure(got[k], want[k], sc[k]))
    _hold(figs, "bn_infer")


def ln_fp32_figures(H, rows, dtype, eps):
    inp = O.ln_inputs(H, rows, dtype)
    assert _clean(*inp.values())
    x, dy, gamma, beta = inp["x"], inp["dy"], inp["gamma"], inp["beta"]
    mean, rstd = O.ln_stats(x, eps)
    m32, r32 = O.ln_stats(x, eps, dtype=F32)
    sc = O.ln_scales(x, dy, mean, rstd, gamma, beta)
    figs = {"gln_mean": O.figure(m32, mean, sc["mean"]), "gln_rstd": O.figure(r32, rstd, sc["rstd"])}
    # y, dx and the parameter gradients on the float32 statistics, as the GPU test takes the kernel's own
    sc = O.ln_scales(x, dy, m32, r32, gamma, beta)
    figs["gln_y"] = O.figure(O.ln_y(x, m32, r32, gamma, beta, dtype=F32), O.ln_y(x, m32, r32, gamma, beta), sc["y"])
    figs["gln_dx"] = O.figure(O.ln_dx(dy, x, m32, r32, gamma, dtype=F32), O.ln_dx(dy, x, m32, r32, gamma), sc["dx"])
    dg, db = O.ln_dparams(dy, x, m32, r32)
    dg32, db32 = O.ln_dparams(dy, x, m32, r32, dtype=F32)
    figs["gln_dgamma"], figs["gln_dbeta"] = O.figure(dg32, dg, sc["dgamma"]), O.figure(db32, db, sc["dbeta"])
    if rows >= 77:
        # the constant row: var = 0 exactly; the offset row alone holds the bars of the statistics
        assert bool((x[O.ROW_CONST] == 0.75).all()) and abs(float(x[O.ROW_OFFSET].double().mean()) - O.LN_OFFSET) < 1
        assert float(rstd[O.ROW_CONST]) == 1 / eps ** 0.5
        if H > 1 and dtype == F32:  # bf16 numbers are 0.5 apart at 100: most of the row rounds to 100
            assert float(x[O.ROW_OFFSET].double().std()) > 0
        r = O.ROW_OFFSET
        assert O.bar_holds("gln_mean", O.figure(m32[r], mean[r], sc["mean"][r]))
        assert O.bar_holds("gln_rstd", O.figure(r32[r], rstd[r], rstd[r]))
    return figs


@pytest.mark.parametrize("dtype", O.DTYPES)
@pytest.mark.parametrize("H,rows", O.LN_CASES)
def test_fp32_layer_norm_within_bars(H, rows, dtype):
    for eps in O.LN_EPS:
        _hold(ln_fp32_figures(H, rows, dtype, O.f32r(eps)), ("ln", H, rows, dtype, eps))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_fp32_scatter_within_bars(dtype):
    figs = {"g_scatter": 0.0}
    for V, H in O.EMBED_TABLES:
        for idtype in O.EMBED_IDS:
            for same in (False, True):
                inp = O.embed_inputs(V, H, idtype, dtype, same)
                assert _clean(inp["table"], inp["dy"], inp["old"])
                for old in (torch.zeros_like(inp["old"]), inp["old"]):
                    want, mag = O.scatter_add(inp["dy"], inp["ids"], old)
                    got, _ = O.scatter_add(inp["dy"], inp["ids"], old, dtype=F32)
                    figs["g_scatter"] = max(figs["g_scatter"], O.figure(got, want, mag))
    _hold(figs, ("scatter", dtype))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_fp32_unary_within_bars(dtype):
    x = O.unary_inputs(dtype)
    assert _clean(x) and float(x.double().abs().max()) == 87 and bool((x == 0).any())
    figs = {}
    for op, name in ((O.TANH, "g_tanh"), (O.SIGMOID, "g_sigmoid")):
        want = O.unary(x, op)
        # every value is a normal float32 (or the 0 of tanh(0)): the figure is relative to it
        w32 = want.float().abs()
        assert bool(((w32 >= 2.0 ** -126) | ((want == 0) & (x.double() == 0))).all())
        assert bool(torch.isfinite(want).all())
        ref32 = torch.tanh(x.float()) if op == O.TANH else torch.sigmoid(x.float())
        figs[name] = max(O.figure(O.unary(x, op, dtype=F32), want, want.abs()), O.figure(ref32, want, want.abs()))
        dy, y = O.unary_bwd_inputs(op, dtype)
        assert _clean(dy, y) and float(y.double().abs().max()) < 1 and (op == O.TANH or float(y.double().min()) > 0)
        for yy in (y, O.unary(x, op).to(dtype)):  # the grid, and stored forward outputs
            d = dy[:1].expand(yy.numel()) if yy.numel() != dy.numel() else dy
            figs["g_d" + name[2:]] = max(figs.get("g_d" + name[2:], 0.0),
                                         O.figure(O.unary_bwd(d, yy, op, dtype=F32), O.unary_bwd(d, yy, op),
                                                  O.unary_bwd_scale(d, yy, op)))
    _hold(figs, ("unary", dtype))


@pytest.mark.parametrize("dtype", O.DTYPES)
def test_fp32_sum_all_within_bars(dtype):
    figs = {"g_sum": 0.0}
    for n in O.SUM_N:
        x = O.sum_inputs(n, dtype)
        assert _clean(x)
        for scale in (1.0, O.f32r(1.0 / n)):
            want, mag = O.sum_all(x, scale)
            got, _ = O.sum_all(x, scale, dtype=F32)
            figs["g_sum"] = max(figs["g_sum"], O.figure(got, want, mag))
    _hold(figs, ("sum_all", dtype))


def test_fp32_gemm_within_bars():
    figs = {"f32_gemm": 0.0}
    for M, N, K, ta, tb, bias, beta, sliced in O.gemm_cases():
        inp = O.gemm_inputs(M, N, K, ta, tb, sliced)
        assert _clean(*inp.values())
        assert inp["A"].is_contiguous() != sliced or 0 in inp["A"].shape or inp["A"].shape[0] == 1
        a = (inp["A"], inp["B"], ta, tb, inp["bias"] if bias else None, inp["C0"] if beta else None)
        want, mag = O.gemm(*a), O.gemm_scale(*a)
        assert want.shape == (M, N)
        figs["f32_gemm"] = max(figs["f32_gemm"], O.figure(O.gemm(*a, dtype=F32), want, mag))
    for Bt, (M, N, K) in O.BATCHED_CASES:
        for ta, tb in ((False, False), (True, False), (False, True)):
            inp = O.gemm_inputs(M, N, K, ta, tb, batch=Bt)
            a = (inp["A"], inp["B"], ta, tb)
            figs["f32_gemm"] = max(figs["f32_gemm"], O.figure(O.gemm(*a, dtype=F32), O.gemm(*a), O.gemm_scale(*a)))
    _hold(figs, "gemm")


def test_scaled_products_are_one_fp32_multiply():
    for dtype in O.DTYPES:
        for rows, C in O.ROW_SCALE_CASES:
            a, g = O.row_scale_inputs(rows, C, dtype)
            got = O.scaled_fp32(a, g[:, None])
            assert got.dtype == dtype and got.shape == a.shape
            # within half an ulp of the output format of the exact product
            exact = a.double() * g.double()[:, None]
            ulp = O.bf16_half_ulp(exact) * (1 if dtype == BF16 else 2.0 ** -16)
            assert bool(((got.double() - exact).abs() <= ulp * (1 + 2.0 ** -14)).all())


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars; every bar
    has a measured figure."""
    for k in sorted(_maxima):
        print("%-14s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        assert O.MARGIN * max(v, O.FLOOR) <= O.BARS[k]
