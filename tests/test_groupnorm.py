"""Group normalisation kernels (groupnorm.hip) on the GPU: `ops.kernels.group_norm_fwd / group_norm_bwd`
in both forms, `ttd.nn.group_norm`, `layers.GroupNormalization`, hipGraph.

Figures and bars are those of groupnorm_oracle.py: mean and rstd against the float64 definition
first; then y against the oracle's apply and dx, dgamma, dbeta against its backward in float64 on
the kernel's own mean / rstd. Every bar is MARGIN times the figure of the oracle's own float32 run
(tests/test_groupnorm_oracle_cpu.py). Every output (y, mean, rstd, dx, dgamma, dbeta, both
workspaces) is a slice of a larger buffer filled with a sentinel bit pattern, which must be
unchanged around the slice afterwards.

The Sequential step runs its convolution on the bf16 MFMA engine for either input dtype
(ttd.nn.conv2d), so it is held to the bf16 bar 2e-2 of test_depthwise.py's Sequential test."""
import functools

import pytest
import torch
import torch.nn.functional as F

import groupnorm_oracle as O
import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import _plan
from tensorflow_train_distributed_amd.ops import kernels as K
from tensorflow_train_distributed_amd.utils import graphs
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

pytestmark = pytest.mark.gpu

GUARD = 64  # elements before and after every output (keeps the slice 16-byte aligned)
BF16, F32 = O.BF16, O.F32


def _sentinel(dtype):
    return 0x5A5B if dtype == BF16 else 0x5A5B5C5D


def _ints(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _guarded(shape, dtype):
    """(whole buffer, the slice shaped `shape`): sentinel bits everywhere, the slice included."""
    n = int(torch.Size(shape).numel())
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
    _ints(buf).fill_(_sentinel(dtype))
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, what):
    v = _ints(buf)
    s = _sentinel(buf.dtype)
    assert bool((v[:GUARD] == s).all()) and bool((v[-GUARD:] == s).all()), "%s: guard elements overwritten" % what


@functools.lru_cache(maxsize=None)
def _case(N_, M, C, G, dt, kind="plain"):
    """CPU inputs of a case, made once and shared (never modified)."""
    return O.inputs(N_, M, C, G, dt, kind)


def _id(case):
    N_, M, C, G, dt = case[:5]
    return "%dx%dx%d_g%d_%s%s" % (N_, M, C, G, str(dt)[6:], "_" + case[5] if len(case) > 5 else "")


def _run(case, form, gamma=True, beta=True, x_dev=None, dy_dev=None, accumulate=False, want_dx=True):
    """Forward and backward of one case into guarded outputs; returns the outputs (GPU tensors)
    after the oracle check."""
    N_, M, C, G, dt = case[:5]
    kind = case[5] if len(case) > 5 else "plain"
    inp = _case(N_, M, C, G, dt, kind)
    eps = O.case_eps(kind)
    x = inp["x"].cuda() if x_dev is None else x_dev
    dy = inp["dy"].cuda() if dy_dev is None else dy_dev
    gm = inp["gamma"].cuda() if gamma else None
    bt = inp["beta"].cuda() if beta else None
    bufs = {}
    for name, shape, d in (("y", (N_, M, C), dt), ("dx", (N_, M, C), dt), ("mean", (N_, G), F32),
                           ("rstd", (N_, G), F32), ("dgamma", (C,), F32), ("dbeta", (C,), F32),
                           ("fwd_ws", (_plan.gn_fwd_ws_floats(N_, M, C),), F32),
                           ("bwd_ws", (_plan.gn_bwd_ws_floats(N_, M, C),), F32)):
        bufs[name] = _guarded(shape, d)
    out = {k: v[1] for k, v in bufs.items()}
    dg0 = db0 = None
    if accumulate:
        dg0, db0 = inp["dg0"], inp["db0"]
        out["dgamma"].copy_(dg0)
        out["dbeta"].copy_(db0)
    y, mean, rstd = K.group_norm_fwd(x, gm, bt, G, eps, out=out["y"], workspace=out["fwd_ws"], form=form,
                                     stats=(out["mean"], out["rstd"]))
    assert y is out["y"] and mean is out["mean"] and rstd is out["rstd"]
    dx = K.group_norm_bwd(dy, x, gm, mean, rstd, out["dgamma"] if gamma else None, out["dbeta"] if beta else None,
                          want_dx=want_dx, accumulate=accumulate, out=out["dx"] if want_dx else None,
                          workspace=out["bwd_ws"], form=form)
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        _guards_intact(buf, name)
    assert (dx is out["dx"]) if want_dx else dx is None
    # the statistics first, against the definition; the rest on the kernel's own statistics
    xc, dyc = x.cpu(), dy.cpu()
    mc, rc = mean.cpu(), rstd.cpu()
    figs = O.stats_figures(mc, rc, xc, G, eps)
    g64 = inp["gamma"] if gamma else None
    figs.update(O.y_figure(y.cpu(), xc, mc, rc, g64, inp["beta"] if beta else None))
    figs.update(O.bwd_figures(dx.cpu() if want_dx else None, out["dgamma"].cpu() if gamma else None,
                              out["dbeta"].cpu() if beta else None, dyc, xc, mc, rc, g64,
                              dg0 if gamma else None, db0 if beta else None))
    print("%s %-7s %s" % (_id(case), form, "  ".join("%s %.2e" % (k[3:], v) for k, v in figs.items())))
    O.check(figs, (_id(case), form))
    return out


def _agree(a, b, case):
    """Two forms of one case: every output within the bar of the other, on the figures' scales."""
    N_, M, C, G, dt = case[:5]
    inp = _case(*case)
    eps = O.case_eps(case[5] if len(case) > 5 else "plain")
    x, dy = inp["x"], inp["dy"]
    mb, rb = b["mean"].cpu(), b["rstd"].cpu()
    sc = O.stats_scales(x, G, eps)
    bs = O.bwd_scales(dy, x, mb, rb, inp["gamma"])
    figs = {"gn_mean": O.figure(a["mean"].cpu(), mb, sc["mean"]), "gn_rstd": O.figure(a["rstd"].cpu(), rb, sc["rstd"]),
            "gn_y": O.figure(a["y"].cpu(), b["y"].cpu(), O.apply_scale(x, mb, rb, inp["gamma"], inp["beta"]),
                             bf16_store=dt == BF16, ulps=1.0),
            "gn_dx": O.figure(a["dx"].cpu(), b["dx"].cpu(), bs["dx"], bf16_store=dt == BF16, ulps=1.0),
            "gn_dgamma": O.figure(a["dgamma"].cpu(), b["dgamma"].cpu(), bs["dgamma"]),
            "gn_dbeta": O.figure(a["dbeta"].cpu(), b["dbeta"].cpu(), bs["dbeta"])}
    O.check(figs, (_id(case), "auto against generic"))


def _both_forms(case):
    N_, M, C, G, dt = case[:5]
    assert _plan.gn_fast_takes(N_, M, C, G, dt == BF16)
    a = _run(case, "auto")
    b = _run(case, "generic")
    _agree(a, b, case)


# ------------------------------------------------------------------ kernels vs the oracle
@pytest.mark.parametrize("CG", O.FAST_CG, ids=lambda cg: "c%d_g%d" % cg)
def test_fast_form_shapes_match_oracle_on_both_forms(CG):
    C, G = CG
    for N_ in O.CASE_N:
        for M in O.case_Ms(C, True):
            _both_forms((N_, M, C, G, BF16))


@pytest.mark.parametrize("case", [(N_, M, C, G, BF16) for N_, M, C, G in O.SLAB_CASES], ids=_id)
def test_slab_boundaries_and_the_slab_cap(case):
    N_, M, C = case[:3]
    T = _plan.gn_parts(N_, M, C)
    cap = O.CAP // N_
    assert T == (M if M <= cap else -(-M // -(-M // cap))) and N_ * T <= O.CAP
    _both_forms(case)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("CG", O.GENERIC_CG, ids=lambda cg: "c%d_g%d" % cg)
def test_generic_form_shapes_match_oracle(CG, dt):
    C, G = CG
    for N_ in O.CASE_N:
        for M in O.case_Ms(C, False):
            assert not _plan.gn_fast_takes(N_, M, C, G, dt == BF16)
            _run((N_, M, C, G, dt), "auto")


@pytest.mark.parametrize("CG", O.FAST_AS_FP32, ids=lambda cg: "c%d_g%d" % cg)
def test_fp32_at_fast_shapes_runs_the_generic_form(CG):
    C, G = CG
    for N_ in O.CASE_N:
        for M in O.case_Ms(C, True):
            assert not _plan.gn_fast_takes(N_, M, C, G, False)
            _run((N_, M, C, G, F32), "auto")


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("kind", O.VALUE_KINDS)
@pytest.mark.parametrize("shape", O.VALUE_SHAPES, ids=lambda s: _id(s))
def test_special_values(shape, kind):
    case = shape + (kind,)
    N_, M, C, G, dt = shape
    forms = ("auto", "generic") if _plan.gn_fast_takes(N_, M, C, G, dt == BF16) else ("auto",)
    for form in forms:
        out = _run(case, form)
        inp = _case(*case)
        Cg = C // G
        if kind == "const_group":
            # every x - pivot is exactly 0: rstd = 1/sqrt(eps), y = beta exactly
            want = 1.0 / torch.sqrt(torch.tensor(O.EPS, dtype=F32))
            assert abs(float(out["rstd"][0, 0]) - float(want)) <= 2.0 ** -22 * float(want)
            assert float(out["mean"][0, 0]) == 3.0
            assert torch.equal(out["y"][0, :, :Cg].cpu(), inp["beta"][:Cg].to(dt).expand(M, Cg))
        if kind == "zero_image":
            assert float(out["mean"][0].abs().max()) == 0.0
            assert torch.equal(out["y"][0].cpu(), inp["beta"].to(dt).expand(M, C))
        if kind == "gamma0":
            assert torch.equal(out["y"][:, :, 0].cpu(), inp["beta"][0].to(dt).expand(N_, M))


@pytest.mark.parametrize("affine", ["gamma", "beta", "none"])
@pytest.mark.parametrize("case", [(3, 9, 16, 4, BF16), (3, 5, 6, 2, F32)], ids=_id)
def test_absent_gamma_and_beta(case, affine):
    out = _run(case, "auto", gamma=affine == "gamma", beta=affine == "beta")
    # the absent gradient's buffer was not touched
    for name, present in (("dgamma", affine == "gamma"), ("dbeta", affine == "beta")):
        if not present:
            assert bool((_ints(out[name]) == _sentinel(F32)).all()), name


# ------------------------------------------------------------------ other behaviour
def _off_by_one(t):
    flat = torch.zeros(t.numel() + 9, dtype=t.dtype, device="cuda")
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


def test_unaligned_views_route_to_the_generic_form():
    """x and dy offset by one element (2 bytes): not 16-byte aligned, so the fast form may not take
    them. The generic kernels' result does not depend on alignment: equal bits to form='generic'."""
    case = (3, 9, 16, 4, BF16)
    inp = _case(*case)
    got = _run(case, "auto", x_dev=_off_by_one(inp["x"]), dy_dev=_off_by_one(inp["dy"]))
    ref = _run(case, "generic")
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        assert torch.equal(got[k], ref[k]), k


def test_bf16_channels_not_a_multiple_of_8_route_to_the_generic_form():
    case = (3, 9, 12, 3, BF16)
    assert not _plan.gn_fast_takes(3, 9, 12, 3, True)
    a, b = _run(case, "auto"), _run(case, "generic")
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("form", ["auto", "generic"])
def test_accumulate_adds_to_the_old_gradients_and_runs_repeat_bitwise(form):
    case = (3, 70, 40, 4, BF16)
    first = _run(case, form)
    again = _run(case, form)
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        assert torch.equal(first[k], again[k]), k  # two runs give identical bits
    acc = _run(case, form, accumulate=True)
    inp = _case(*case)
    # one fp32 add per element onto the same sums
    assert torch.equal(acc["dgamma"], inp["dg0"].cuda() + first["dgamma"])
    assert torch.equal(acc["dbeta"], inp["db0"].cuda() + first["dbeta"])
    assert torch.equal(acc["dx"], first["dx"])


def test_want_dx_false_launches_no_dx_kernel(monkeypatch):
    case = (3, 9, 16, 4, BF16)
    calls = []
    real = K._lib.call
    monkeypatch.setattr(K._lib, "call", lambda name, *a: calls.append(name) or real(name, *a))
    out = _run(case, "auto", want_dx=False)
    assert "ttdk_group_norm_bwd_stats" in calls and "ttdk_group_norm_bwd_dx" not in calls
    assert bool((_ints(out["dx"]) == _sentinel(BF16)).all())  # its buffer is untouched
    del calls[:]
    _run(case, "auto")
    assert calls.count("ttdk_group_norm_bwd_dx") == 1


# ------------------------------------------------------------------ autograd: ttd.nn
@pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", O.RANK_SHAPES + [(2, 5, 5, 16)], ids=lambda s: "x".join(map(str, s)))
def test_nn_group_norm_gradients_at_every_rank(shape, dt):
    C = shape[-1]
    G = 4
    gen = torch.Generator().manual_seed(3 + len(shape))
    x0 = (torch.randn(shape, generator=gen) * 2 + 1).to(dt)
    dy0 = torch.randn(shape, generator=gen).to(dt)
    g0, b0 = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    x, gm, bt = x0.cuda().requires_grad_(True), g0.cuda().requires_grad_(True), b0.cuda().requires_grad_(True)
    y = N.group_norm(x, gm, bt, groups=G, eps=O.EPS)
    assert y.dtype == dt and y.shape == x.shape
    y.backward(dy0.cuda())
    assert x.grad.dtype == dt and gm.grad.dtype == F32 and bt.grad.dtype == F32
    # the same bits as the launch wrappers on [N, M, C], whose results are held to the oracle on the
    # kernel's own statistics
    x3, dy3 = x0.reshape(shape[0], -1, C).cuda(), dy0.reshape(shape[0], -1, C).cuda()
    y3, mean, rstd = K.group_norm_fwd(x3, g0.cuda(), b0.cuda(), G, O.EPS)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx3 = K.group_norm_bwd(dy3, x3, g0.cuda(), mean, rstd, dg, db)
    assert torch.equal(y.detach().reshape(x3.shape), y3) and torch.equal(x.grad.reshape(x3.shape), dx3)
    assert torch.equal(gm.grad, dg) and torch.equal(bt.grad, db)
    xc, mc, rc = x3.cpu(), mean.cpu(), rstd.cpu()
    figs = O.stats_figures(mc, rc, xc, G, O.EPS)
    figs.update(O.y_figure(y3.cpu(), xc, mc, rc, g0, b0))
    figs.update(O.bwd_figures(dx3.cpu(), dg.cpu(), db.cpu(), dy3.cpu(), xc, mc, rc, g0))
    print(shape, str(dt)[6:], figs)
    O.check(figs, (shape, dt))


def test_nn_group_norm_bf16_gamma_gets_a_bf16_gradient_and_none_gets_none():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 6, 16, generator=gen).bfloat16().cuda().requires_grad_(True)
    gm = (torch.rand(16, generator=gen) + 0.5).bfloat16().cuda().requires_grad_(True)
    bt = torch.randn(16, generator=gen).bfloat16().cuda().requires_grad_(True)
    N.group_norm(x, gm, bt, groups=2).sum().backward()
    assert gm.grad.dtype == BF16 and bt.grad.dtype == BF16 and x.grad.dtype == BF16
    x2 = x.detach().clone().requires_grad_(True)
    y = N.group_norm(x2, None, None, groups=2)
    y.sum().backward()
    assert x2.grad is not None
    m, _, r = O.stats_def(x.detach().cpu().reshape(2, 36, 16), 2, O.EPS)
    want = O.apply(x.detach().cpu().reshape(2, 36, 16), m, r, None, None)
    assert float((y.detach().cpu().double().reshape(2, 36, 16) - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


def test_nn_group_norm_skips_dx_when_x_needs_no_gradient(monkeypatch):
    calls = []
    real = K._lib.call
    monkeypatch.setattr(K._lib, "call", lambda name, *a: calls.append(name) or real(name, *a))
    x = torch.randn(2, 4, 4, 16, device="cuda")
    gm = torch.ones(16, device="cuda", requires_grad=True)
    N.group_norm(x, gm, None, groups=4).sum().backward()
    assert "ttdk_group_norm_bwd_dx" not in calls and gm.grad is not None


# ------------------------------------------------------------------ layers: one GradientTape step
def _model(x):
    """The activation is tanh: the two paths differ by the bf16 rounding of the convolution's weights
    and output, and a ReLU right behind the normalisation turns that into flipped mask bits (an
    element within 2^-9 of zero is on in one path and off in the other). With so few elements that
    alone moves the convolution's weight gradient by 3.3e-2 of its maximum when both paths run on the
    CPU and only the rounding is emulated; a smooth activation leaves 2e-3."""
    L.reset_naming(seed=9)
    m = L.Sequential([L.Conv2D(16, 3), L.GroupNormalization(groups=4), L.Activation("tanh"),
                      L.GlobalAveragePooling2D(), L.Dense(10)])
    m(x)
    return m


def test_sequential_gradient_tape_step_matches_cpu_path():
    gen = torch.Generator().manual_seed(6)
    X = torch.randn(8, 12, 12, 8, generator=gen).bfloat16().float()
    Y = torch.randint(0, 10, (8,), generator=gen)
    cpu, gpu = _model(X[:1]), _model(X[:1])
    for (n, a), (_, b) in zip(cpu.named_variables(), gpu.named_variables()):
        assert torch.equal(a, b), n
    cpu.to_flat("cpu")
    gpu.to_flat("cuda")
    names = [n for n, t in cpu.named_variables() if t.requires_grad]
    assert "group_normalization/gamma" in names and "group_normalization/beta" in names
    results = {}
    for tag, model, x, y in (("cpu", cpu, X, Y), ("gpu", gpu, X.cuda(), Y.cuda())):
        opt = ttd.train.MomentumOptimizer(0.1, 0.9)
        with ttd.GradientTape() as tape:
            loss = F.cross_entropy(model(x), y)
        gs = tape.gradient(loss, model.trainable_variables)
        grads = [g.detach().cpu().double().clone() for g in gs]
        opt.apply_gradients(zip(gs, model.trainable_variables))
        after = [t.detach().cpu().double().clone() for t in model.trainable_variables]
        results[tag] = (float(loss.detach()), grads, after)
    (lc, gc, ac), (lg, gg, ag) = results["cpu"], results["gpu"]
    print("loss cpu %.5f gpu %.5f" % (lc, lg))
    assert abs(lg - lc) <= 2e-2 * abs(lc)
    for n, a, b in zip(names, gg, gc):
        err = float((a - b).abs().max() / b.abs().max())
        print("%-40s %.2e" % (n, err))
        assert err <= 2e-2, (n, err)
    for n, a, b in zip(names, ag, ac):
        assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()), n


# ------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize("case", [(3, 70, 40, 4, BF16), (3, 9, 6, 2, F32)], ids=_id)
def test_captured_graph_replays_bit_equal_to_eager(case):
    N_, M, C, G, dt = case
    inp = _case(*case)
    x, dy = inp["x"].cuda(), inp["dy"].cuda()
    gm, bt = inp["gamma"].cuda(), inp["beta"].cuda()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(N_, G, device="cuda"), torch.empty(N_, G, device="cuda")
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    fws, bws = K.group_norm_fwd_workspace(N_, M, C), K.group_norm_bwd_workspace(N_, M, C)

    def step():  # one stream, no parallel branches
        K.group_norm_fwd(x, gm, bt, G, O.EPS, out=y, workspace=fws, stats=(mean, rstd))
        K.group_norm_bwd(dy, x, gm, mean, rstd, dg, db, out=dx, workspace=bws)

    captured, _ = graphs.capture(step)
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):  # fresh inputs in the captured buffers
        x.copy_(torch.randn(x.shape, generator=gen).to(dt))
        dy.copy_(torch.randn(dy.shape, generator=gen).to(dt))
        for o in (y, dx, mean, rstd, dg, db):
            o.zero_()
        captured.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in (y, mean, rstd, dx, dg, db)]
        y2, m2, r2 = K.group_norm_fwd(x, gm, bt, G, O.EPS)
        dg2, db2 = torch.empty_like(dg), torch.empty_like(db)
        dx2 = K.group_norm_bwd(dy, x, gm, m2, r2, dg2, db2)
        for a, b in zip(got, (y2, m2, r2, dx2, dg2, db2)):
            assert torch.equal(a, b)
        assert float(got[0].float().abs().max()) > 0


# ------------------------------------------------------------------ refusals
def test_refusals_on_the_gpu():
    x = torch.randn(2, 4, 4, 8, device="cuda")
    g8 = torch.ones(8, device="cuda")
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x.half(), g8.half(), None, groups=2)  # fp16
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, g8, None, groups=3)  # G does not divide C
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, g8, None, groups=0)
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x[:0], g8, None, groups=2)  # empty
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x[0, 0, 0], g8, None, groups=2)  # rank 1
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, torch.ones(8), None, groups=2)  # gamma on another device
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, torch.ones(4, device="cuda"), None, groups=2)  # gamma of the wrong length
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, None, torch.ones(16, device="cuda"), groups=2)
    # the launch wrappers refuse the same, and mixed dtypes, small buffers, unknown forms
    x3 = x.reshape(2, 16, 8)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3.half(), g8, None, 2, 1e-3)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8, None, 3, 1e-3)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8, None, 0, 1e-3)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3[:0], g8, None, 2, 1e-3)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x, g8, None, 2, 1e-3)  # not [N, M, C]
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8.bfloat16(), None, 2, 1e-3)  # gamma not fp32
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, torch.ones(4, device="cuda"), None, 2, 1e-3)
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8, None, 2, 1e-3, out=torch.empty(2, 16, 4, device="cuda"))
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8, None, 2, 1e-3, workspace=torch.empty(8, device="cuda"))
    with pytest.raises(InvalidArgumentError):
        K.group_norm_fwd(x3, g8, None, 2, 1e-3, form="fast")
    y, mean, rstd = K.group_norm_fwd(x3, g8, None, 2, 1e-3)
    dg = torch.empty(8, device="cuda")
    with pytest.raises(InvalidArgumentError):
        K.group_norm_bwd(x3.bfloat16(), x3, g8, mean, rstd, dg, None)  # dtype mix
    with pytest.raises(InvalidArgumentError):
        K.group_norm_bwd(x3, x3, g8, mean, rstd, dg, None, workspace=torch.empty(8, device="cuda"))
    with pytest.raises(InvalidArgumentError):
        K.group_norm_bwd(x3, x3, g8, mean[:, :1].contiguous(), rstd, dg, None)  # mean / rstd disagree
