"""The float64 reference of tests/pooling_oracle.py, checked on the CPU against independent
statements of the same operations (F.max_pool2d on a -inf-padded input under double autograd,
x.mean((1, 2)), three cases worked out by hand); then the reference run in float32 against itself
in float64 on the case tables of tests/test_pooling_kernels.py: those maxima, times O.MARGIN, are
the bars of the GPU tests (run with -s to see them)."""
import pytest
import torch
import torch.nn.functional as F

import pooling_oracle as O

F32, F64 = torch.float32, torch.float64
INF = float("inf")


def _torch_maxpool(x, dy, geom):
    """(y, dx) by F.max_pool2d on an explicitly -inf-padded NCHW copy, under autograd."""
    R, S, sh, sw, ph, pw, P, Q = geom
    N, H, W, C = x.shape
    eh = max((P - 1) * sh + R - H - ph, 0)
    ew = max((Q - 1) * sw + S - W - pw, 0)
    xa = x.clone().requires_grad_(True)
    xp = F.pad(xa.permute(0, 3, 1, 2), (pw, ew, ph, eh), value=-INF)
    y = F.max_pool2d(xp, (R, S), (sh, sw), 0)[:, :, :P, :Q].permute(0, 2, 3, 1)
    y.backward(dy)
    return y.detach(), xa.grad


_TORCH_GEOMS = [(9, 8, O.explicit(9, 8, 3, 2, 1)), (8, 9, O.explicit(8, 9, 5, 3, 2)), (2, 7, O.explicit(2, 7, 2, 2, 0)),
                (7, 9, O.explicit(7, 9, 3, 1, 1))] + [(H, W, g) for _, H, W, g in O.GENERIC_GEOMS]


@pytest.mark.parametrize("H,W,geom", _TORCH_GEOMS)
def test_maxpool_matches_torch_double_autograd(H, W, geom):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, H, W, 5, generator=gen, dtype=F64)  # tie-free
    dy = torch.randn(2, geom[6], geom[7], 5, generator=gen, dtype=F64)
    y, arg, holds = O.maxpool(x, geom)
    assert O.arg_ok(arg, arg, holds, y) and int(holds.sum()) == y.numel()
    dx, mag = O.maxpool_bwd(dy, arg, x.shape, geom)
    y_t, dx_t = _torch_maxpool(x, dy, geom)
    kw = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(y, y_t, **kw)
    torch.testing.assert_close(dx, dx_t, **kw)
    torch.testing.assert_close(mag, _torch_maxpool(x, dy.abs(), geom)[1], **kw)


def test_gap_matches_torch():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(3, 7, 5, 6, generator=gen, dtype=F64)
    dy = torch.randn(3, 6, generator=gen, dtype=F64)
    y, mag = O.gap(x)
    kw = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(y, x.mean((1, 2)), **kw)
    torch.testing.assert_close(mag, x.abs().mean((1, 2)), **kw)
    xa = x.clone().requires_grad_(True)
    xa.mean((1, 2)).backward(dy)
    dx, dmag = O.gap_bwd(dy, x.shape)
    torch.testing.assert_close(dx.contiguous(), xa.grad, **kw)
    torch.testing.assert_close(dmag.contiguous(), xa.grad.abs(), **kw)


def _image(rows):
    return torch.tensor(rows, dtype=F64).view(1, len(rows), len(rows[0]), 1)


def test_tie_by_hand():
    """3x3 input, 2x2 window, stride 1, no padding: four windows, taps numbered 0 1 / 2 3.
        1 5 5        window (0,0) = {1,5,2,5}: max 5 at taps 1 and 3, the first wins: arg 1 -> (0,1)
        2 5 0        window (0,1) = {5,5,5,0}: arg 0 -> (0,1)
        7 7 0        window (1,0) = {2,5,7,7}: arg 2 -> (2,0)
                     window (1,1) = {5,0,7,0}: arg 2 -> (2,1)
    dy = [[1, 2], [4, 8]]: dx (0,1) = 1 + 2 = 3, (2,0) = 4, (2,1) = 8."""
    x = _image([[1, 5, 5], [2, 5, 0], [7, 7, 0]])
    geom = O.explicit(3, 3, 2, 1, 0)
    y, arg, holds = O.maxpool(x, geom)
    assert y.view(2, 2).tolist() == [[5, 5], [7, 7]]
    assert arg.view(2, 2).tolist() == [[1, 0], [2, 2]]
    assert O.arg_ok(arg, arg, holds, y)
    wrong = arg.clone()
    wrong[0, 0, 0, 0] = 3  # holds the maximum too, but is not the first
    assert not O.arg_ok(wrong, arg, holds, y)
    dx, mag = O.maxpool_bwd(_image([[1, 2], [4, 8]]), arg, x.shape, geom)
    assert dx.view(3, 3).tolist() == [[0, 3, 0], [0, 0, 0], [4, 8, 0]]
    assert torch.equal(mag, dx)


def test_all_neginf_border_window_by_hand():
    """2x2 input of -inf, 3x3 window, stride 2, padding 1: one window over rows and columns -1..1;
    its taps inside the input are (1,1) = 4, (1,2) = 5, (2,1) = 7 and (2,2) = 8, all -inf: y = -inf
    and arg = 4, the first tap inside (never 0, which lies in the padding). dy = 3 goes to pixel
    (0,0). With the input [[-inf, 2], [-inf, -inf]] the maximum 2 sits at tap 5 -> pixel (0,1)."""
    x = _image([[-INF, -INF], [-INF, -INF]])
    geom = O.explicit(2, 2, 3, 2, 1)
    assert geom[6:] == (1, 1)
    y, arg, holds = O.maxpool(x, geom)
    assert y.item() == -INF and arg.item() == 4
    assert holds.view(9).tolist() == [False, False, False, False, True, True, False, True, True]
    assert not O.arg_ok(torch.zeros_like(arg), arg, holds, y)
    dx, _ = O.maxpool_bwd(_image([[3]]), arg, x.shape, geom)
    assert dx.view(2, 2).tolist() == [[3, 0], [0, 0]]
    # an arg that names the padding sends the gradient nowhere
    assert float(O.maxpool_bwd(_image([[3]]), torch.zeros_like(arg), x.shape, geom)[0].abs().sum()) == 0
    x2 = _image([[-INF, 2], [-INF, -INF]])
    y2, arg2, _ = O.maxpool(x2, geom)
    assert y2.item() == 2 and arg2.item() == 5


def test_nan_by_hand():
    """1x4 input [1, nan, 3, nan], 1x3 window, stride 1, padding 1 -> four windows:
    {., 1, nan} -> NaN, arg 2; {1, nan, 3} -> NaN, arg 1; {nan, 3, nan} -> NaN, arg 0 or 2;
    {3, nan, .} -> NaN, arg 1. dy = [1, 2, 4, 8] with the first NaN taps: pixel 1 gets 1 + 2 + 4,
    pixel 3 gets 8; with arg 2 in the third window pixel 1 gets 3 and pixel 3 gets 12."""
    nan = float("nan")
    x = _image([[1, nan, 3, nan]])
    geom = (1, 3, 1, 1, 0, 1, 1, 4)
    y, arg, holds = O.maxpool(x, geom)
    assert bool(torch.isnan(y).all()) and arg.view(4).tolist() == [2, 1, 0, 1]
    other = arg.clone()
    other[0, 0, 2, 0] = 2
    assert O.arg_ok(arg, arg, holds, y) and O.arg_ok(other, arg, holds, y)
    other[0, 0, 2, 0] = 1  # the 3: not a NaN tap
    assert not O.arg_ok(other, arg, holds, y)
    dy = _image([[1, 2, 4, 8]])
    assert O.maxpool_bwd(dy, arg, x.shape, geom)[0].view(4).tolist() == [0, 7, 0, 8]
    other[0, 0, 2, 0] = 2
    assert O.maxpool_bwd(dy, other, x.shape, geom)[0].view(4).tolist() == [0, 3, 0, 12]
    # a NaN outside every window's reach changes nothing: 2x2 window, stride 2 on 3 columns
    x3 = _image([[1, 2, nan]])
    y3, arg3, _ = O.maxpool(x3, (1, 2, 1, 2, 0, 0, 1, 1))
    assert y3.item() == 2 and arg3.item() == 1


def test_stem_by_hand_and_tables():
    """One channel group of 8, 2x2 input, scale 1, shift 0 but channel 1 (scale -1) and channel 2
    (scale 0, shift 1): y = [[1, -2], [-3, 0.5]] in every channel. Channel 0: a = [[1, 0], [0, 0.5]],
    pooled 1 at tap 4, mask bits 1, 0, 0, 1 (as channels 3..7). Channel 1: a = [[0, 2], [3, 0]], pooled 3 at tap 7.
    Channel 2: a = 1 everywhere, pooled 1 at tap 4 (first of four equal)."""
    y = torch.tensor([[1.0, -2.0], [-3.0, 0.5]]).view(1, 2, 2, 1).repeat(1, 1, 1, 8)
    scale, shift = torch.ones(8), torch.zeros(8)
    scale[1], scale[2], shift[2] = -1.0, 0.0, 1.0
    a = O.stem_activation(y, scale, shift)
    assert a[0, :, :, 0].tolist() == [[1, 0], [0, 0.5]] and a[0, :, :, 1].tolist() == [[0, 2], [3, 0]]
    pooled, arg, _ = O.maxpool(a, O.stem_geom(2, 2))
    assert pooled.view(8)[:3].tolist() == [1, 3, 1] and arg.view(8)[:3].tolist() == [4, 7, 4]
    m = O.mask_bits(a)
    assert m.tolist() == [0b11111101, 0b00000110, 0b00000110, 0b11111101]
    keep = O.mask_bools(m, a.shape)
    assert torch.equal(keep, a.float() > 0)
    g, mag = O.stem_bwd(torch.full((1, 1, 1, 8), 2.0), arg, keep)
    assert g[0, :, :, 0].tolist() == [[2, 0], [0, 0]] and g[0, :, :, 1].tolist() == [[0, 0], [2, 0]]
    s, smag = O.stem_sums(g.bfloat16(), y)
    assert s[:, 0].tolist() == [2, 2] and s[:, 1].tolist() == [2, -6] and smag[:, 1].tolist() == [2, 6]
    # the case tables: which fast cases have no output, and the SAME geometries' padding
    refused = [(ksp, hw) for ksp, hw, C in O.FAST_CASES if C == 8 and not O.accepted(O.explicit(*hw, *ksp))]
    assert refused == [((2, 2, 0), (1, 1)), ((3, 2, 0), (1, 1)), ((3, 2, 0), (2, 7))]
    geoms = {label: g for label, _, _, g in O.GENERIC_GEOMS}
    assert geoms["same_3x2_s2x1_even"] == (3, 2, 2, 1, 0, 0, 4, 6)
    assert geoms["same_3x2_s2x1_odd"] == (3, 2, 2, 1, 1, 0, 5, 7)
    assert geoms["same_3x3_s2_even"][4:] == (0, 0, 4, 4) and geoms["same_3x3_s2_odd"][4:] == (1, 1, 5, 5)
    assert all(O.accepted(g) for g in geoms.values())
    k, s_, p = O.WRAP["ksp"]
    groups = O.WRAP["N"] * O.pool_out(O.WRAP["H"], k, s_, p) * O.pool_out(O.WRAP["W"], k, s_, p) * O.WRAP["C"] // 8
    assert 0 < groups - 16384 * 256 <= 16384
    inp = O.stem_inputs((2, 4, 4, 8))
    f64 = inp["y"].double() * inp["scale"].double() + inp["shift"].double()
    assert torch.equal((inp["y"].float() * inp["scale"] + inp["shift"]).double(), f64)  # exact in float32


# ------------------------------------------------------------------ float32 against float64
_maxima = {}


def _hold(figs, label):
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
        assert O.bar_holds(k, v), (label, k, v, O.BARS[k])


def _fp32_dx(x, dy, geom, name):
    _, arg, _ = O.maxpool(x, geom)
    want, mag = O.maxpool_bwd(dy, arg, x.shape, geom)
    got, _ = O.maxpool_bwd(dy, arg, x.shape, geom, dtype=F32)
    return {name: O.figure(got, want, mag)}


@pytest.mark.parametrize("ksp", O.FAST_KSP)
def test_fp32_maxpool_backward_within_bars(ksp):
    figs = {"pool_dx": 0.0}
    for hw in O.FAST_HW:
        geom = O.explicit(*hw, *ksp)
        if not O.accepted(geom):
            continue
        for C in O.FAST_C:
            for variant in O.VARIANTS:
                x, d = O.pool_inputs(*hw, C, variant)
                f = _fp32_dx(x, O.cut(d, geom[6], geom[7]), geom, "pool_dx")
                figs["pool_dx"] = max(figs["pool_dx"], f["pool_dx"])
    _hold(figs, ("fast", ksp))


def test_fp32_generic_maxpool_backward_within_bars():
    figs = {"pool_dx": 0.0}
    for label, H, W, geom in O.GENERIC_GEOMS:
        for C in O.GENERIC_C:
            for variant in O.VARIANTS:
                x, d = O.pool_inputs(H, W, C, variant)
                f = _fp32_dx(x, O.cut(d, geom[6], geom[7]), geom, "pool_dx")
                figs["pool_dx"] = max(figs["pool_dx"], f["pool_dx"])
    _hold(figs, "generic")


def _fp32_gap(x, dy):
    want, mag = O.gap(x)
    dwant, dmag = O.gap_bwd(dy, x.shape)
    return {"gap_y": O.figure(O.gap(x, dtype=F32)[0], want, mag),
            "gap_dx": O.figure(O.gap_bwd(dy, x.shape, dtype=F32)[0], dwant, dmag)}


@pytest.mark.parametrize("C", O.AVG_C)
def test_fp32_avgpool_within_bars(C):
    for N, HW, C_ in O.AVG_CASES:
        if C_ == C:
            _hold(_fp32_gap(*O.avg_inputs(N, HW, C)), ("avg", N, HW, C))


def test_fp32_gap_within_bars():
    for HW, C in O.GAP_CASES:
        _hold(_fp32_gap(*O.avg_inputs(O.GAP_N, HW, C)), ("gap", HW, C))


@pytest.mark.parametrize("shape", O.STEM_SHAPES)
def test_fp32_stem_within_bars(shape):
    inp = O.stem_inputs(shape)
    a = O.stem_activation(inp["y"], inp["scale"], inp["shift"])
    assert torch.equal(a, O.stem_activation(inp["y"], inp["scale"], inp["shift"], dtype=F32))
    _, arg, _ = O.maxpool(a, O.stem_geom(shape[1], shape[2]))
    keep = a.float() > 0
    want, mag = O.stem_bwd(inp["dpooled"], arg, keep)
    got, _ = O.stem_bwd(inp["dpooled"], arg, keep, dtype=F32)
    g = want.bfloat16()
    s, smag = O.stem_sums(g, inp["y"])
    _hold({"stem_g": O.figure(got, want, mag),
           "stem_partial": O.figure(O.stem_sums(g, inp["y"], dtype=F32)[0], s, smag)}, ("stem", shape))


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars; every bar
    has a measured figure."""
    for k in sorted(_maxima):
        print("%-14s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        assert O.MARGIN * max(v, O.FLOOR) <= O.BARS[k]
