"""Depthwise convolution kernels (depthwise.hip) on the GPU: `ops.kernels.dwconv_fwd / dwconv_dgrad /
dwconv_wgrad` in both forms, `ttd.nn.depthwise_conv2d / separable_conv2d`, the two layers, hipGraph.

Measure: max |got - want| / max |want| against the float64 oracle (depthwise_oracle.py) of the
same rounded inputs, the measure and bars of test_nn_gpu_ops.py:
  fp32  1e-5 forward and data gradient, 1e-4 weight gradient;
  bf16  2e-2 forward and data gradient (one bf16 rounding is 2^-9 of max |want|; a dropped tap is
        about 0.3); the weight gradient at the fp32 bar 1e-4: its output is fp32 and products of
        bf16 numbers are exact in fp32.
Every output (y, dx, dw, the partial workspace) is a slice of a larger buffer filled with a
sentinel bit pattern, which must be unchanged around the slice afterwards.

separable_conv2d and the Sequential step run the pointwise conv on the bf16 MFMA engine for either
input dtype (ttd.nn.conv2d), so they are held to the bf16 bar 2e-2 throughout."""
import functools

import pytest
import torch
import torch.nn.functional as F

import depthwise_oracle as O
import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import _plan
from tensorflow_train_distributed_amd.ops import kernels as K
from tensorflow_train_distributed_amd.utils import graphs
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

pytestmark = pytest.mark.gpu

BARS = {torch.float32: (1e-5, 1e-5, 1e-4), torch.bfloat16: (2e-2, 2e-2, 1e-4)}
GUARD = 64  # elements before and after every output (keeps the slice 16-byte aligned)
STRIP = _plan.dw_strip()
CAP = _plan.dw_max_slabs()


def _bf(n, h, w, c, stride=1, padding="SAME"):
    return (n, h, w, c, 1, (3, 3), (stride, stride), (1, 1), padding, torch.bfloat16)


# the last strip of a row partial, exact, and one column long
STRIP_SHAPES = [_bf(2, 5, STRIP - 1, 16), _bf(2, 5, STRIP, 16), _bf(2, 5, STRIP + 1, 16),
                _bf(2, 5, 2 * (STRIP + 1), 16, stride=2), _bf(2, 6, 2 * STRIP + 1, 16, stride=2)]
FAST_SHAPES = O.FAST_SHAPES + STRIP_SHAPES


def _split(rows):
    """(N, H) with N * H == rows and both above 1 when rows has a factor."""
    for n in (7, 5, 3, 2):
        if rows % n == 0 and rows > n:
            return n, rows // n
    return 1, rows


# N * P below, at and above the slab cap (stride 1 SAME: P = H); Q = 5 is one full and one partial strip
SLAB_SHAPES = [_bf(*_split(rows), 5, 8) for rows in (CAP - 1, CAP, CAP + 1, 2 * CAP + 1)] + [_bf(CAP, 1, 5, 8)]


def _id(shape):
    n, h, w, c, m, k, s, d, p, dt = shape
    return "%dx%dx%dx%d_m%d_%dx%d_s%d%d_d%d%d_%s_%s" % (n, h, w, c, m, k[0], k[1], s[0], s[1], d[0], d[1],
                                                      p if isinstance(p, str) else "p%d%d" % p, str(dt)[6:])


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and float64 oracle results of one shape, computed once and shared (never modified)."""
    x, k, dy, geom = O.make_inputs(shape, seed=sum(shape[:4]))
    return (x, k, dy, geom, O.forward(x, k, geom), O.dgrad(dy, k, tuple(x.shape), geom),
            O.wgrad(x, dy, tuple(k.shape), geom))


def _sentinel(dtype):
    return 0x5A5B if dtype == torch.bfloat16 else 0x5A5B5C5D


def _ints(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guarded(shape, dtype, numel=None):
    """(whole buffer, the slice shaped `shape`): sentinel bits everywhere, the slice included."""
    n = numel if numel is not None else int(torch.Size(shape).numel())
    buf = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
    _ints(buf).fill_(_sentinel(dtype) if dtype == torch.bfloat16 else _sentinel(dtype))
    inner = buf[GUARD:GUARD + n]
    return buf, (inner.view(shape) if numel is None else inner)


def _guards_intact(buf, what):
    v = _ints(buf)
    s = _sentinel(buf.dtype)
    assert bool((v[:GUARD] == s).all()) and bool((v[-GUARD:] == s).all()), "%s: guard rows overwritten" % what


def _run(shape, form, x_dev=None, dy_dev=None):
    """The three kernels of one shape into guarded outputs; returns (y, dx, dw) after the oracle check."""
    x64, k64, dy64, geom, y64, dx64, dk64 = _case(shape)
    dt = shape[-1]
    bars = BARS[dt]
    x = x64.to(dt).cuda() if x_dev is None else x_dev
    dy = dy64.to(dt).cuda() if dy_dev is None else dy_dev
    w = k64.float().cuda()
    g = _plan.dw_geom(tuple(x.shape), tuple(w.shape), *geom)
    ybuf, y = _guarded(tuple(y64.shape), dt)
    dxbuf, dx = _guarded(tuple(x64.shape), dt)
    dwbuf, dw = _guarded(tuple(k64.shape), torch.float32)
    wsbuf, ws = _guarded(None, torch.float32, numel=_plan.dw_wgrad_ws_floats(g))
    assert K.dwconv_fwd(x, w, geom, out=y, form=form) is y
    K.dwconv_dgrad(dy, w, tuple(x.shape), geom, out=dx, form=form)
    K.dwconv_wgrad(x, dy, tuple(w.shape), geom, out=dw, workspace=ws, form=form)
    torch.cuda.synchronize()
    for buf, what in ((ybuf, "y"), (dxbuf, "dx"), (dwbuf, "dw"), (wsbuf, "workspace")):
        _guards_intact(buf, what)
    errs = O.rel_err(y, y64), O.rel_err(dx, dx64), O.rel_err(dw, dk64)
    print("%s %-7s fwd %.2e dgrad %.2e wgrad %.2e" % (_id(shape), form, *errs))
    assert errs[0] <= bars[0] and errs[1] <= bars[1] and errs[2] <= bars[2], (errs, bars)
    return y, dx, dw


def _agree(a, b, want, bar):
    err = float((a.double() - b.double()).abs().max().cpu() / want.abs().max())
    assert err <= bar, (err, bar)


# ------------------------------------------------------------------ kernels vs the oracle
@pytest.mark.parametrize("shape", FAST_SHAPES, ids=_id)
def test_fast_form_shapes_match_oracle_on_both_forms(shape):
    x64, k64, _, geom, y64, dx64, dk64 = _case(shape)
    assert _plan.dw_fast_takes(_plan.dw_geom(tuple(x64.shape), tuple(k64.shape), *geom), True)
    ya, dxa, dwa = _run(shape, "auto")
    yg, dxg, dwg = _run(shape, "generic")
    bars = BARS[torch.bfloat16]
    # the summation order may differ between the forms: agreement within the bar, not equal bits
    _agree(ya, yg, y64, bars[0])
    _agree(dxa, dxg, dx64, bars[1])
    _agree(dwa, dwg, dk64, bars[2])


@pytest.mark.parametrize("shape", O.GENERIC_SHAPES, ids=_id)
def test_generic_form_shapes_match_oracle(shape):
    x64, k64, _, geom = _case(shape)[:4]
    assert not _plan.dw_fast_takes(_plan.dw_geom(tuple(x64.shape), tuple(k64.shape), *geom),
                                   shape[-1] == torch.bfloat16)
    _run(shape, "auto")


def test_unaligned_views_route_to_the_generic_form():
    """x and dy offset by one element (2 bytes): not 16-byte aligned, so the fast form may not take
    them. The generic kernels' result does not depend on alignment: equal bits to form='generic'."""
    shape = O.FAST_SHAPES[1]
    x64, _, dy64 = _case(shape)[:3]

    def off_by_one(t64):
        flat = torch.zeros(t64.numel() + 9, dtype=torch.bfloat16, device="cuda")
        v = flat[1:1 + t64.numel()].view(t64.shape)
        v.copy_(t64.to(torch.bfloat16))
        assert v.data_ptr() % 16 == 2 and v.is_contiguous()
        return v

    got = _run(shape, "auto", x_dev=off_by_one(x64), dy_dev=off_by_one(dy64))
    ref = _run(shape, "generic")
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ weight-gradient slabs
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=_id)
def test_wgrad_slabs_accumulate_and_repeat_bitwise(shape):
    x64, k64, dy64, geom, _, _, dk64 = _case(shape)
    g = _plan.dw_geom(tuple(x64.shape), tuple(k64.shape), *geom)
    rows = g.N * g.P
    assert _plan.dw_wgrad_parts(g) == (rows if rows <= CAP else -(-rows // -(-rows // CAP)))
    _, _, dwa = _run(shape, "auto")
    _, _, dwg = _run(shape, "generic")
    _agree(dwa, dwg, dk64, 1e-4)
    x, dy = x64.bfloat16().cuda(), dy64.bfloat16().cuda()
    for form, first in (("auto", dwa), ("generic", dwg)):
        # two runs give identical bits
        again = K.dwconv_wgrad(x, dy, tuple(k64.shape), geom, form=form)
        assert torch.equal(again, first), form
        # accumulate=True adds onto a pre-filled dw
        base = torch.randn(tuple(k64.shape), generator=torch.Generator().manual_seed(5)).cuda()
        acc = K.dwconv_wgrad(x, dy, tuple(k64.shape), geom, out=base.clone(), accumulate=True, form=form)
        err = O.rel_err(acc, base.cpu().double() + dk64)
        assert err <= 1e-4, (form, err)
        assert torch.equal(acc, base + first)  # one fp32 add per element onto the same sum


# ------------------------------------------------------------------ autograd: ttd.nn
@pytest.mark.parametrize("shape", [O.FAST_SHAPES[0], O.FAST_SHAPES[4], O.GENERIC_SHAPES[0], O.GENERIC_SHAPES[1]],
                         ids=_id)
def test_nn_depthwise_conv2d_gradients(shape):
    x64, k64, dy64, geom, y64, dx64, dk64 = _case(shape)
    dt = shape[-1]
    strides, dil, padding = shape[6], shape[7], shape[8]
    x = x64.to(dt).cuda().requires_grad_(True)
    k = k64.float().cuda().requires_grad_(True)
    y = N.depthwise_conv2d(x, k, strides, padding, dil)
    assert y.dtype == dt and tuple(y.shape) == tuple(y64.shape)
    y.backward(dy64.to(dt).cuda())
    assert x.grad.dtype == dt and k.grad.dtype == torch.float32
    errs = O.rel_err(y, y64), O.rel_err(x.grad, dx64), O.rel_err(k.grad, dk64)
    print("nn.depthwise_conv2d %s: fwd %.2e dgrad %.2e wgrad %.2e" % (_id(shape), *errs))
    bars = BARS[dt]
    assert errs[0] <= bars[0] and errs[1] <= bars[1] and errs[2] <= bars[2], (errs, bars)


def test_nn_depthwise_conv2d_bf16_kernel_gets_a_bf16_gradient():
    shape = O.FAST_SHAPES[1]
    x64, k64, dy64, geom, _, _, dk64 = _case(shape)
    k = k64.bfloat16().cuda().requires_grad_(True)
    N.depthwise_conv2d(x64.bfloat16().cuda(), k).backward(dy64.bfloat16().cuda())
    assert k.grad.dtype == torch.bfloat16
    assert O.rel_err(k.grad, dk64) <= 2e-2  # the fp32 gradient rounded once to the kernel's dtype


def test_nn_depthwise_conv2d_launches_no_data_gradient_when_x_needs_none(monkeypatch):
    shape = O.FAST_SHAPES[1]
    x64, k64, dy64, geom, _, _, dk64 = _case(shape)
    calls = []
    real = K.dwconv_dgrad
    monkeypatch.setattr(K, "dwconv_dgrad", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    k = k64.float().cuda().requires_grad_(True)
    N.depthwise_conv2d(x64.bfloat16().cuda(), k).backward(dy64.bfloat16().cuda())
    assert calls == [] and O.rel_err(k.grad, dk64) <= 1e-4
    x = x64.bfloat16().cuda().requires_grad_(True)
    N.depthwise_conv2d(x, k).backward(dy64.bfloat16().cuda())
    assert calls == [1] and x.grad is not None


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_nn_separable_conv2d_gradients(dt):
    shape = (2, 9, 7, 8, 2, (3, 3), (2, 2), (1, 1), "SAME", dt)
    x64, k64, _, geom, y64, _, _ = _case(shape)
    gen = torch.Generator().manual_seed(4)
    pw64 = (torch.randn(1, 1, 16, 24, generator=gen) * 0.3).bfloat16().double()
    dz64 = torch.randn(2, 5, 4, 24, generator=gen).bfloat16().double()
    x, k, pw = [t.to(dt).cuda().requires_grad_(True) for t in (x64, k64, pw64)]
    z = N.separable_conv2d(x, k, pw, (2, 2), "SAME")
    assert tuple(z.shape) == (2, 5, 4, 24) and z.dtype == dt
    z.backward(dz64.to(dt).cuda())
    dy64 = dz64 @ pw64[0, 0].T
    want = [y64 @ pw64[0, 0], O.dgrad(dy64, k64, tuple(x64.shape), geom), O.wgrad(x64, dy64, tuple(k64.shape), geom),
            (y64.reshape(-1, 16).T @ dz64.reshape(-1, 24)).reshape(1, 1, 16, 24)]
    errs = [O.rel_err(a, b) for a, b in zip((z, x.grad, k.grad, pw.grad), want)]
    print("nn.separable_conv2d %s: z %.2e dx %.2e ddepthwise %.2e dpointwise %.2e" % (str(dt)[6:], *errs))
    assert max(errs) <= 2e-2, errs


# ------------------------------------------------------------------ layers: one GradientTape step
def _model(x):
    """Built at once: the variables are drawn from the generator reset_naming seeds, on the first call.
    No bias on the depthwise layer, as in MobileNet: batch normalisation removes a per-channel shift,
    so that bias has an exactly zero gradient and a relative error of rounding noise means nothing."""
    L.reset_naming(seed=9)
    m = L.Sequential([L.Conv2D(16, 3), L.DepthwiseConv2D(3, use_bias=False), L.BatchNormalization(),
                      L.SeparableConv2D(32, 3, strides=2), L.GlobalAveragePooling2D(), L.Dense(10)])
    m(x)
    return m


def test_sequential_gradient_tape_step_matches_cpu_path():
    gen = torch.Generator().manual_seed(6)
    X = torch.randn(8, 12, 12, 8, generator=gen).bfloat16().float()
    Y = torch.randint(0, 10, (8,), generator=gen)
    cpu, gpu = _model(X[:1]), _model(X[:1])
    for (n, a), (_, b) in zip(cpu.named_variables(), gpu.named_variables()):
        assert torch.equal(a, b), n
    gpu.to_flat("cuda")
    names = [n for n, t in cpu.named_variables() if t.requires_grad]
    assert "depthwise_conv2d/depthwise_kernel" in names and "separable_conv2d/pointwise_kernel" in names
    grads = {}
    for tag, model, x, y in (("cpu", cpu, X, Y), ("gpu", gpu, X.cuda(), Y.cuda())):
        with ttd.GradientTape() as tape:
            loss = F.cross_entropy(model(x), y)
        gs = tape.gradient(loss, model.trainable_variables)
        grads[tag] = (float(loss.detach()), [g.detach().cpu().double() for g in gs])
    (lc, gc), (lg, gg) = grads["cpu"], grads["gpu"]
    print("loss cpu %.5f gpu %.5f" % (lc, lg))
    assert abs(lg - lc) <= 2e-2 * abs(lc)
    for n, a, b in zip(names, gg, gc):
        err = float((a - b).abs().max() / b.abs().max())
        print("%-40s %.2e" % (n, err))
        assert err <= 2e-2, (n, err)


# ------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize("shape", [O.FAST_SHAPES[0], O.GENERIC_SHAPES[0]], ids=_id)
def test_captured_graph_replays_bit_equal_to_eager(shape):
    x64, k64, dy64, geom = _case(shape)[:4]
    dt = shape[-1]
    x, dy, w = x64.to(dt).cuda(), dy64.to(dt).cuda(), k64.float().cuda()
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
    ws = K.dwconv_wgrad_workspace(tuple(x.shape), tuple(w.shape), geom)

    def step():  # one stream, no parallel branches
        K.dwconv_fwd(x, w, geom, out=y)
        K.dwconv_dgrad(dy, w, tuple(x.shape), geom, out=dx)
        K.dwconv_wgrad(x, dy, tuple(w.shape), geom, out=dw, workspace=ws)

    captured, _ = graphs.capture(step)
    gen = torch.Generator().manual_seed(8)
    for _ in range(2):  # fresh inputs in the captured buffers
        x.copy_(torch.randn(x.shape, generator=gen).to(dt))
        dy.copy_(torch.randn(dy.shape, generator=gen).to(dt))
        w.copy_(torch.randn(w.shape, generator=gen).bfloat16().float())
        for o in (y, dx, dw):
            o.zero_()
        captured.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in (y, dx, dw)]
        want = [K.dwconv_fwd(x, w, geom), K.dwconv_dgrad(dy, w, tuple(x.shape), geom),
                K.dwconv_wgrad(x, dy, tuple(w.shape), geom)]
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert float(got[0].float().abs().max()) > 0


# ------------------------------------------------------------------ refusals
def test_refusals_on_the_gpu():
    x = torch.randn(2, 8, 8, 8, device="cuda")
    k = torch.randn(3, 3, 8, 1, device="cuda")
    geom = O.geometry(8, 8, 3, 3, (1, 1), "SAME")
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x.half(), k)  # fp16 input
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(3, 3, 16, 1, device="cuda"))  # filter C differs
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x[0], k)  # 3-D input
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(8, 3, 8, 1, device="cuda"))  # R above 7
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(3, 8, 8, 1, device="cuda"))  # S above 7
    # the launch wrappers refuse the same, and mixed dtypes / non-contiguous tensors
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x.half(), k, geom)
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x, torch.randn(3, 3, 16, 1, device="cuda"), geom)
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x[0], k, geom)
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x, torch.randn(8, 3, 8, 1, device="cuda"), geom)
    with pytest.raises(InvalidArgumentError):
        K.dwconv_wgrad(x, torch.randn(2, 8, 8, 8, device="cuda").bfloat16(), (3, 3, 8, 1), geom)  # dtype mix
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x.permute(0, 2, 1, 3), k, geom)  # not contiguous
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x, k, geom, out=torch.empty(2, 8, 8, 4, device="cuda"))  # out of the wrong shape
    with pytest.raises(InvalidArgumentError):
        K.dwconv_fwd(x, k, geom, form="fast")
