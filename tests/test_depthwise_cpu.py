"""Depthwise / separable convolution without a GPU: the float64 oracle of depthwise_oracle.py against
float64 F.conv2d(groups=C) and its autograd, the CPU paths of ttd.nn.depthwise_conv2d /
separable_conv2d and of the two layers, and the launch plan of dwconv_plan.h.

fp32 bars (max |got - want| / max |want| against the oracle, the bars of test_nn_gpu_ops.py): 1e-5
forward and data gradient, 1e-4 weight gradient. The oracle's own fp32 run (F.conv2d in fp32) must
stay a factor 10 inside them at every shape."""
import pytest
import torch
import torch.nn.functional as F

import depthwise_oracle as O
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import _plan
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

FWD_BAR, DGRAD_BAR, WGRAD_BAR = 1e-5, 1e-5, 1e-4
SHAPES = O.FAST_SHAPES + O.GENERIC_SHAPES
IDS = ["%dx%dx%dx%d_m%d_%dx%d_s%s_d%s_%s_%s" % (n, h, w, c, m, k[0], k[1], "%d%d" % s, "%d%d" % d, p if isinstance(p, str)
                                               else "p%d%d" % p, str(dt).split(".")[-1])
       for n, h, w, c, m, k, s, d, p, dt in SHAPES]


_inputs = O.make_inputs


def _torch_ref(x, k, dy, geom, dtype):
    """F.conv2d(groups=C) and autograd on the explicitly padded input, in `dtype`."""
    sh, sw, ph, pw, dh, dw, P, Q = geom
    N_, H, W, C = x.shape
    R, S, _, M = k.shape
    eh = max((P - 1) * sh + (R - 1) * dh + 1 - H - ph, 0)
    ew = max((Q - 1) * sw + (S - 1) * dw + 1 - W - pw, 0)
    xl = x.detach().clone().to(dtype).requires_grad_(True)  # a leaf of its own: the inputs are shared
    kl = k.detach().clone().to(dtype).requires_grad_(True)
    xp = F.pad(xl.permute(0, 3, 1, 2), (pw, ew, ph, eh))
    y = F.conv2d(xp, kl.permute(2, 3, 0, 1).reshape(C * M, 1, R, S), stride=(sh, sw), dilation=(dh, dw), groups=C)
    y = y[:, :, :P, :Q].permute(0, 2, 3, 1)
    y.backward(dy.to(dtype))
    return y.detach(), xl.grad, kl.grad


@pytest.fixture(scope="module")
def oracle():
    """shape index -> (x, k, dy, geom, y64, dx64, dk64), computed once."""
    cache = {}

    def get(i):
        if i not in cache:
            x, k, dy, geom = _inputs(SHAPES[i], seed=i)
            cache[i] = (x, k, dy, geom, O.forward(x, k, geom), O.dgrad(dy, k, x.shape, geom),
                        O.wgrad(x, dy, k.shape, geom))
        return cache[i]
    return get


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_oracle_is_float64_grouped_conv_and_fp32_conv_sits_inside_the_bars(oracle, i):
    x, k, dy, geom, y64, dx64, dk64 = oracle(i)
    y, dx, dk = _torch_ref(x, k, dy, geom, torch.float64)
    errs = O.rel_err(y, y64), O.rel_err(dx, dx64), O.rel_err(dk, dk64)
    print("float64 F.conv2d vs oracle: fwd %.2e dgrad %.2e wgrad %.2e" % errs)
    assert max(errs) <= 1e-12, errs
    y, dx, dk = _torch_ref(x, k, dy, geom, torch.float32)
    errs = O.rel_err(y, y64), O.rel_err(dx, dx64), O.rel_err(dk, dk64)
    print("fp32 F.conv2d vs oracle:    fwd %.2e dgrad %.2e wgrad %.2e" % errs)
    assert errs[0] <= FWD_BAR / 10 and errs[1] <= DGRAD_BAR / 10 and errs[2] <= WGRAD_BAR / 10, errs


def test_oracle_geometry_is_tf_same_and_valid():
    # 10x12, 3x3, stride 2: SAME pads one row / column in all, and it goes to the bottom / right
    assert O.geometry(10, 12, 3, 3, (2, 2), "SAME") == (2, 2, 0, 0, 1, 1, 5, 6)
    assert O.geometry(9, 7, 3, 3, (1, 1), "SAME") == (1, 1, 1, 1, 1, 1, 9, 7)
    assert O.geometry(11, 9, 5, 5, (2, 1), "SAME") == (2, 1, 2, 2, 1, 1, 6, 9)
    assert O.geometry(13, 13, 3, 3, (1, 1), "SAME", (2, 2)) == (1, 1, 2, 2, 2, 2, 13, 13)
    assert O.geometry(11, 9, 3, 3, (2, 2), "VALID") == (2, 2, 0, 0, 1, 1, 5, 4)
    assert O.geometry(9, 7, 3, 3, (1, 1), (2, 0)) == (1, 1, 2, 0, 1, 1, 11, 5)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_nn_depthwise_conv2d_cpu_matches_oracle(oracle, i):
    x64, k64, dy64, geom, y64, dx64, dk64 = oracle(i)
    _, _, _, _, _, _, strides, dil, padding, _ = SHAPES[i]
    x = x64.float().requires_grad_(True)
    k = k64.float().requires_grad_(True)
    y = N.depthwise_conv2d(x, k, strides, padding, dil)
    assert y.shape == y64.shape and y.dtype == torch.float32
    y.backward(dy64.float())
    errs = O.rel_err(y, y64), O.rel_err(x.grad, dx64), O.rel_err(k.grad, dk64)
    print("cpu path vs oracle: fwd %.2e dgrad %.2e wgrad %.2e" % errs)
    assert errs[0] <= FWD_BAR and errs[1] <= DGRAD_BAR and errs[2] <= WGRAD_BAR, errs


def test_nn_depthwise_conv2d_accepts_tf_style_strides_and_dilations():
    x64, k64, _, geom = _inputs(SHAPES[7])  # 5x5, strides (2, 1)
    y = N.depthwise_conv2d(x64.float(), k64.float(), [1, 2, 1, 1], "SAME", 1)
    assert O.rel_err(y, O.forward(x64, k64, geom)) <= FWD_BAR
    y2 = N.depthwise_conv2d(x64.float(), k64.float(), 2, "VALID", [1, 1, 1, 1])
    assert O.rel_err(y2, O.forward(x64, k64, O.geometry(11, 9, 5, 5, (2, 2), "VALID"))) <= FWD_BAR


def test_nn_separable_conv2d_cpu_matches_oracle():
    x64, k64, _, geom = _inputs(SHAPES[8])  # C 5, M 2, dilation 2
    g = torch.Generator().manual_seed(11)
    pw64 = (torch.randn(1, 1, 10, 6, generator=g) * 0.3).bfloat16().double()
    dz64 = torch.randn(2, 13, 13, 6, generator=g).bfloat16().double()
    x, k, pw = [t.float().requires_grad_(True) for t in (x64, k64, pw64)]
    z = N.separable_conv2d(x, k, pw, (1, 1), "SAME", (2, 2))
    z.backward(dz64.float())
    y64 = O.forward(x64, k64, geom)
    z64 = y64 @ pw64[0, 0]
    dy64 = dz64 @ pw64[0, 0].T
    assert z.shape == (2, 13, 13, 6)
    assert O.rel_err(z, z64) <= FWD_BAR
    assert O.rel_err(x.grad, O.dgrad(dy64, k64, x64.shape, geom)) <= DGRAD_BAR
    assert O.rel_err(k.grad, O.wgrad(x64, dy64, k64.shape, geom)) <= WGRAD_BAR
    assert O.rel_err(pw.grad[0, 0], y64.reshape(-1, 10).T @ dz64.reshape(-1, 6)) <= WGRAD_BAR


def test_nn_depthwise_refusals_on_cpu():
    x = torch.randn(2, 8, 8, 4)
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(3, 3, 5, 1))  # filter C differs
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x[0], torch.randn(3, 3, 4, 1))  # 3-D input
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(8, 3, 4, 1))  # R above 7
    with pytest.raises(InvalidArgumentError):
        N.depthwise_conv2d(x, torch.randn(3, 8, 4, 1))  # S above 7
    with pytest.raises(InvalidArgumentError):
        N.separable_conv2d(x, torch.randn(3, 3, 4, 2), torch.randn(1, 1, 4, 6))  # pointwise wants C*M = 8


# ------------------------------------------------------------------ layers
def test_depthwise_and_separable_layers_variables_and_composite():
    L.reset_naming(seed=2)
    torch.manual_seed(2)
    x = torch.randn(2, 9, 7, 3)
    dwl = L.DepthwiseConv2D(3, depth_multiplier=2)
    sep = L.SeparableConv2D(5, 3, strides=2, depth_multiplier=2)
    y, z = dwl(x), sep(x)
    assert [(n, tuple(t.shape)) for n, t in dwl.named_variables()] == [
        ("depthwise_conv2d/depthwise_kernel", (3, 3, 3, 2)), ("depthwise_conv2d/bias", (6,))]
    assert [(n, tuple(t.shape)) for n, t in sep.named_variables()] == [
        ("separable_conv2d/depthwise_kernel", (3, 3, 3, 2)), ("separable_conv2d/pointwise_kernel", (1, 1, 6, 5)),
        ("separable_conv2d/bias", (5,))]
    assert y.shape == (2, 9, 7, 6) and z.shape == (2, 5, 4, 5)
    # the separable layer is its two-op composite
    with torch.no_grad():
        sep.bias.copy_(torch.randn(5))
    want = N.conv2d(N.depthwise_conv2d(x, sep.depthwise_kernel, (2, 2), "SAME"), sep.pointwise_kernel, (1, 1),
                    "VALID") + sep.bias
    torch.testing.assert_close(sep(x), want, atol=1e-6, rtol=1e-6)
    # depth_multiplier = 2 orders the output channels c * M + m
    k = dwl.depthwise_kernel.detach()
    for c in range(3):
        for m in range(2):
            one = F.conv2d(x[..., c][:, None], k[:, :, c, m][None, None], padding=1)[:, 0]
            torch.testing.assert_close(y[..., c * 2 + m].detach(), one + dwl.bias.detach()[c * 2 + m], atol=1e-5,
                                       rtol=1e-5)
    no_bias = L.DepthwiseConv2D((3, 5), use_bias=False, activation="relu")
    out = no_bias(x)
    assert [n for n, _ in no_bias.named_variables()] == ["depthwise_conv2d_1/depthwise_kernel"]
    assert tuple(no_bias.depthwise_kernel.shape) == (3, 5, 3, 1) and float(out.detach().min()) >= 0.0


# ------------------------------------------------------------------ dwconv_plan.h
def _geom(shape):
    n, h, w, c, m, (r, s), strides, dil, padding, _ = shape
    return _plan.dw_geom((n, h, w, c), (r, s, c, m), *O.geometry(h, w, r, s, strides, padding, dil))


def _check_slabs(g):
    T = _plan.dw_wgrad_parts(g)
    rows = g.N * g.P
    assert 1 <= T <= min(rows, _plan.dw_max_slabs())
    nxt = 0
    for t in range(T):
        r0, r1 = _plan.dw_slab_rows(g, t)
        assert r0 == nxt and r1 > r0, (t, r0, r1)  # in order, none empty, no gap, no overlap
        nxt = r1
    assert nxt == rows
    assert _plan.dw_part_stride(g) % 4 == 0 and 0 <= _plan.dw_part_stride(g) - g.R * g.S * g.C * g.M < 4
    assert _plan.dw_wgrad_ws_floats(g) == (T + 1) * _plan.dw_part_stride(g)
    return T


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_plan_slabs_and_admission_at_every_shape(i):
    g = _geom(SHAPES[i])
    _check_slabs(g)
    bf16 = SHAPES[i][-1] == torch.bfloat16
    assert _plan.dw_valid(g)
    assert _plan.dw_fast_takes(g, bf16) == (i < len(O.FAST_SHAPES))
    assert not _plan.dw_fast_takes(g, False)  # fp32 is never the fast form


def test_plan_slabs_around_the_cap():
    cap = _plan.dw_max_slabs()
    assert _plan.dw_strip() >= 1
    for rows in (1, cap - 1, cap, cap + 1, 2 * cap + 1):
        # N * P = rows with P = 1 (a 1-row image, VALID 1x3) and with N = 1
        for n, h in ((rows, 1), (1, rows)):
            g = _plan.dw_geom((n, h, 5, 8), (1, 3, 8, 1), 1, 1, 0, 1, 1, 1, h, 5)
            assert g.N * g.P == rows
            T = _check_slabs(g)
            assert T == (rows if rows <= cap else -(-rows // -(-rows // cap)))
    # a wide filter gradient caps the workspace before the slab count does
    g = _plan.dw_geom((64, 64, 64, 4096), (7, 7, 4096, 1), 1, 1, 3, 3, 1, 1, 64, 64)
    T = _check_slabs(g)
    assert T < cap and _plan.dw_wgrad_ws_floats(g) <= (1 << 22) + 2 * _plan.dw_part_stride(g)


def test_plan_refuses_bad_geometry():
    ok = dict(x=(2, 8, 8, 8), w=(3, 3, 8, 1), geo=(1, 1, 1, 1, 1, 1, 8, 8))
    assert _plan.dw_valid(_plan.dw_geom(ok["x"], ok["w"], *ok["geo"]))
    assert not _plan.dw_valid(_plan.dw_geom(ok["x"], (8, 3, 8, 1), *ok["geo"]))
    assert not _plan.dw_valid(_plan.dw_geom(ok["x"], ok["w"], 0, 1, 1, 1, 1, 1, 8, 8))
    assert not _plan.dw_valid(_plan.dw_geom(ok["x"], ok["w"], 1, 1, 1, 1, 1, 1, 0, 8))


def test_plan_matches_the_kernel_librarys_own_query():
    """ttdk_dwconv_wgrad_parts (libttd_hip.so, a host function) returns the plan's T."""
    from tensorflow_train_distributed_amd.ops import _lib
    from tensorflow_train_distributed_amd.ops import kernels as K  # registers the signatures
    assert K.DwGeom._fields == ("sh", "sw", "ph", "pw", "dh", "dw", "P", "Q")
    for shape in SHAPES:
        g = _geom(shape)
        assert _lib.query("ttdk_dwconv_wgrad_parts", g) == _plan.dw_wgrad_parts(g)
        assert _lib.query("ttdk_dwconv_wgrad_ws_floats", g) == _plan.dw_wgrad_ws_floats(g)
