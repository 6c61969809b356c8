"""The kernels of csrc/kernels/pool.hip (max pooling with its byte argmax and gather backward,
global average pooling, the two stem fusions) and the pooling kernels of csrc/kernels/nn_generic.hip
against the float64 statements of tests/pooling_oracle.py, at the smallest shapes at which each can
still go wrong: every border, channel-group counts that are no power of two, planted constant,
all -inf, NaN and -inf-border images, one grid-stride trip, the stem's lane layouts.

What is a selection is compared exactly: y bit for bit, arg by the rule (a tap inside the input
that holds the maximum, the first of them; any NaN tap where there is one), the ReLU mask, and
the fast path against the generic path on every geometry both accept. What is a sum is compared
element-wise, |got - want| <= half a bf16 ulp of want (bf16 outputs only: the store) + bar * scale,
with dx taken from the kernel's own arg once arg is checked. A bar is 16 x the largest value the
same figure takes when the oracle itself runs in float32 (tests/test_pooling_oracle_cpu.py), never
less than 16 x 2^-24. Outputs sit between guard rows of a fixed byte pattern that must survive, and
start out as the pattern.

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure          MI355X     fp32      bar
  pool_dx         4.3e-19    4.1e-8    1e-6   (sums of at most 25 bf16 numbers: exact in fp32)
  gap_y           4.0e-8     4.0e-8    1e-6   (the largest is the rounding of a sum of 3 divided by 3)
  gap_dx          7.9e-8     5.4e-8    1e-6   (dy * (1/HW): two roundings)
  stem_g          3.4e-19    0         1e-6
  stem_partial    0          0         1e-6
"""
import numpy as np
import pytest
import torch

import pooling_oracle as O
import tensorflow_train_distributed_amd as ttd
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
PATTERN = 0x5A
DT = {F32: 0, BF16: 1}

_seen = {}


def _check(figs, label):
    for k, v in figs.items():
        _seen[k] = max(_seen.get(k, 0.0), v)
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    return O.check(figs, label)


class Guarded:
    """A tensor `t` of `shape` with O.GUARD rows (elements of a 1-D shape) of the byte PATTERN on
    either side in one allocation; `t` starts out as the pattern too, so what a kernel leaves
    unwritten shows."""

    def __init__(self, shape, dtype):
        shape = tuple(shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.n = int(np.prod(shape)) * item
        self.g = O.GUARD * (int(np.prod(shape[1:])) if len(shape) > 1 else 1) * item
        self.g = (self.g + 15) // 16 * 16  # the kernels move 16 B at a time: keep `t` aligned
        self.raw = torch.full((2 * self.g + self.n,), PATTERN, dtype=U8, device=DEV)
        self.t = self.raw[self.g:self.g + self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())


def _bits(t):
    t = t.contiguous()
    return t.view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _same_values(got, ref):
    """Bit for bit, any NaN standing for any NaN."""
    ref = ref.to(got.dtype)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and bool((gn | (_bits(got) == _bits(ref))).all())


def _p(t):
    return t.data_ptr()


# ------------------------------------------------------------------ max pooling: the two paths
def _fwd(path, x, geom):
    R, S, sh, sw, ph, pw, P, Q = geom
    N, H, W, C = x.shape
    y, arg = Guarded((N, P, Q, C), x.dtype), Guarded((N, P, Q, C), U8)
    if path == "fast":
        _lib.call("ttdk_maxpool_fwd", _p(x), _p(y.t), _p(arg.t), N, H, W, C, P, Q, R, S, sh, sw, ph, pw, _lib.stream())
    else:
        _lib.call("ttdk_maxpool_generic_fwd", _p(x), _p(y.t), _p(arg.t), DT[x.dtype], N, H, W, C, P, Q, R, S, sh, sw,
                  ph, pw, _lib.stream())
    assert y.intact() and arg.intact()
    return y.t, arg.t


def _bwd(path, dy, arg, x_shape, geom):
    R, S, sh, sw, ph, pw, P, Q = geom
    N, H, W, C = x_shape
    dx = Guarded(x_shape, dy.dtype)
    if path == "fast":
        _lib.call("ttdk_maxpool_bwd", _p(dy), _p(arg), _p(dx.t), N, H, W, C, P, Q, R, S, sh, sw, ph, pw, _lib.stream())
    else:
        _lib.call("ttdk_maxpool_generic_bwd", _p(dy), _p(arg), _p(dx.t), DT[dy.dtype], N, H, W, C, P, Q, R, S, sh, sw,
                  ph, pw, _lib.stream())
    assert dx.intact()
    return dx.t


def _maxpool_case(path, H, W, C, geom, variant, dtype):
    """y, then arg, then dx from the kernel's own arg; returns (the pool_dx figure, y, arg, dx)."""
    xc, dc = O.pool_inputs(H, W, C, variant)
    x, dy = xc.to(DEV).to(dtype), O.cut(dc, geom[6], geom[7]).to(DEV).to(dtype)
    label = (path, H, W, C, geom, variant, dtype)
    y, arg = _fwd(path, x, geom)
    y_ref, first, holds = O.maxpool(x, geom)
    assert _same_values(y, y_ref), (label, y.flatten()[:16].tolist(), y_ref.flatten()[:16].tolist())
    assert O.arg_ok(arg, first, holds, y_ref), label
    dx = _bwd(path, dy, arg, x.shape, geom)
    want, mag = O.maxpool_bwd(dy, arg, x.shape, geom)
    return O.figure(dx, want, mag, bf16_store=dtype == BF16), y, arg, dx


@pytest.mark.parametrize("ksp", O.FAST_KSP)
def test_maxpool_fast_path(ksp):
    fig, ran = 0.0, 0
    for hw in O.FAST_HW:
        geom = O.explicit(*hw, *ksp)
        if not O.accepted(geom):  # no output at this extent: test_refusals_make_no_launch
            continue
        for C in O.FAST_C:
            for variant in O.VARIANTS:
                fig = max(fig, _maxpool_case("fast", *hw, C, geom, variant, BF16)[0])
                ran += 1
    assert ran
    _check({"pool_dx": fig}, ("fast", ksp))


@pytest.mark.parametrize("dtype", (F32, BF16))
@pytest.mark.parametrize("C", O.GENERIC_C)
def test_maxpool_generic_path(C, dtype):
    fig = 0.0
    for label, H, W, geom in O.GENERIC_GEOMS:
        for variant in O.VARIANTS:
            fig = max(fig, _maxpool_case("generic", H, W, C, geom, variant, dtype)[0])
    _check({"pool_dx": fig}, ("generic", C, dtype))


@pytest.mark.parametrize("ksp", O.FAST_KSP)
def test_both_paths_agree(ksp):
    """bf16, C % 8 == 0, a square window: both entry points take the call, and y, arg and dx are the
    same bits on every input without a NaN (the all -inf image and the -inf border included)."""
    ran = 0
    for hw in O.FAST_HW:
        geom = O.explicit(*hw, *ksp)
        if not O.accepted(geom):
            continue
        for C in O.FAST_C:
            for variant in O.VARIANTS:
                if variant == "nan":
                    continue
                _, y0, a0, d0 = _maxpool_case("fast", *hw, C, geom, variant, BF16)
                _, y1, a1, d1 = _maxpool_case("generic", *hw, C, geom, variant, BF16)
                label = (ksp, hw, C, variant)
                assert _same_bits(y0, y1), label
                assert torch.equal(a0, a1), (label, a0[1, 0, 0, :8].tolist(), a1[1, 0, 0, :8].tolist())
                assert _same_bits(d0, d1), label
                ran += 1
    assert ran


def test_all_neginf_border_window_names_a_tap_inside():
    """3/2/1 on a 2x2 image of -inf: the one window's taps inside the input are 4, 5, 7 and 8; arg
    is 4 on both paths and the gradient arrives at pixel (0, 0)."""
    x = torch.full((1, 2, 2, 8), O.NEG_INF, dtype=BF16, device=DEV)
    dy = torch.full((1, 1, 1, 8), 3.0, dtype=BF16, device=DEV)
    geom = O.explicit(2, 2, 3, 2, 1)
    for path in ("fast", "generic"):
        y, arg = _fwd(path, x, geom)
        assert bool((y.float() == O.NEG_INF).all()), path
        assert arg.view(-1).tolist() == [4] * 8, (path, arg.view(-1).tolist())
        dx = _bwd(path, dy, arg, x.shape, geom)
        assert dx[0, 0, 0].tolist() == [3.0] * 8 and float(dx.float().abs().sum()) == 24.0, path


def test_grid_stride_trip():
    """2 x 513 x 512 outputs of 8 groups: 8192 groups past 16384 blocks of 256, so the first blocks
    of the forward take a second trip of the grid-stride loop (the backward, over the input, takes
    four). Small integers: every selection and every sum is exact, the whole of y, arg and dx is
    compared, image by image."""
    k, s, p = O.WRAP["ksp"]
    x, dy = O.wrap_inputs(DEV)
    N, H, W, C = x.shape
    geom = O.explicit(H, W, k, s, p)
    assert N * geom[6] * geom[7] * (C // 8) == 16384 * 256 + 8192
    y, arg = _fwd("fast", x, geom)
    dx = _bwd("fast", dy, arg, x.shape, geom)
    for n in range(N):
        y_ref, first, holds = O.maxpool(x[n:n + 1], geom, dtype=F32)
        assert _same_bits(y[n:n + 1], y_ref.to(BF16)), n
        assert torch.equal(arg[n:n + 1], first), n
        del holds
        want, _ = O.maxpool_bwd(dy[n:n + 1], first, (1, H, W, C), geom, dtype=F32)
        assert _same_bits(dx[n:n + 1], want.to(BF16)), n


# ------------------------------------------------------------------ global average pooling
@pytest.mark.parametrize("C", O.AVG_C)
def test_avgpool(C):
    figs = {"gap_y": 0.0, "gap_dx": 0.0}
    for N, HW, C_ in O.AVG_CASES:
        if C_ != C:
            continue
        xc, dc = O.avg_inputs(N, HW, C)
        x, dy = xc.to(DEV), dc.to(DEV)
        want, mag = O.gap(x)
        outs = []
        for with_y, with_f in ((True, True), (True, False), (False, True)):
            y, yf = Guarded((N, C), BF16), Guarded((N, C), F32)
            _lib.call("ttdk_avgpool_fwd", _p(x), _p(y.t) if with_y else None, _p(yf.t) if with_f else None, N, HW, C,
                      _lib.stream())
            assert y.intact() and yf.intact()
            assert with_y or y.untouched()
            assert with_f or yf.untouched()
            outs.append((y.t, yf.t))
        assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[2][1])
        figs["gap_y"] = max(figs["gap_y"], O.figure(outs[0][0], want, mag, bf16_store=True),
                            O.figure(outs[0][1], want, mag))
        assert bool((outs[0][1][:, 1] == 0).all())  # the channel of zeros
        dx = Guarded((N, HW, 1, C), BF16)
        _lib.call("ttdk_avgpool_bwd", _p(dy), _p(dx.t), N, HW, C, _lib.stream())
        assert dx.intact()
        dwant, dmag = O.gap_bwd(dy, (N, HW, 1, C))
        figs["gap_dx"] = max(figs["gap_dx"], O.figure(dx.t, dwant, dmag, bf16_store=True))
    _check(figs, ("avgpool", C))


@pytest.mark.parametrize("dtype", (F32, BF16))
def test_gap_generic(dtype):
    figs = {"gap_y": 0.0, "gap_dx": 0.0}
    N = O.GAP_N
    for HW, C in O.GAP_CASES:
        xc, dc = O.avg_inputs(N, HW, C)
        x, dy = xc.to(DEV).to(dtype), dc.to(DEV).to(dtype)
        y = Guarded((N, C), dtype)
        _lib.call("ttdk_gap_fwd", _p(x), _p(y.t), DT[dtype], N, HW, C, _lib.stream())
        assert y.intact()
        want, mag = O.gap(x)
        figs["gap_y"] = max(figs["gap_y"], O.figure(y.t, want, mag, bf16_store=dtype == BF16))
        dx = Guarded((N, HW, 1, C), dtype)
        _lib.call("ttdk_gap_bwd", _p(dy), _p(dx.t), DT[dtype], N, HW, C, _lib.stream())
        assert dx.intact()
        dwant, dmag = O.gap_bwd(dy, (N, HW, 1, C))
        figs["gap_dx"] = max(figs["gap_dx"], O.figure(dx.t, dwant, dmag, bf16_store=dtype == BF16))
    _check(figs, ("gap", dtype))


# ------------------------------------------------------------------ stem fusions
@pytest.mark.parametrize("shape", O.STEM_SHAPES)
def test_stem_fusions(shape):
    N, H, W, C = shape
    P, Q = H // 2, W // 2
    inp = {k: v.to(DEV) for k, v in O.stem_inputs(shape).items()}
    y, scale, shift, dpooled = inp["y"], inp["scale"], inp["shift"], inp["dpooled"]
    assert K.stem_pool_fusable(shape)
    out, arg, mask = Guarded((N, P, Q, C), BF16), Guarded((N, P, Q, C), U8), Guarded((N * H * W * C // 8,), U8)
    _lib.call("ttdk_bn_relu_maxpool", _p(y), _p(scale), _p(shift), _p(out.t), _p(arg.t), _p(mask.t), N, H, W, C, P, Q,
              _lib.stream())
    assert out.intact() and arg.intact() and mask.intact()
    a = O.stem_activation(y, scale, shift)
    pooled_ref, first, holds = O.maxpool(a, O.stem_geom(H, W))
    assert _same_bits(out.t, pooled_ref.to(BF16))
    assert torch.equal(arg.t, first) and O.arg_ok(arg.t, first, holds, pooled_ref)
    assert torch.equal(mask.t, O.mask_bits(a))
    # the wrapper returns the same
    w_out, w_arg, w_mask = K.bn_relu_maxpool(y, scale, shift)
    assert _same_bits(w_out, out.t) and torch.equal(w_arg, arg.t) and torch.equal(w_mask, mask.t)

    T = _lib.query("ttdk_maxpool_bwd_bnstat_blocks", N, P, Q, C)
    lanes = 256 // (C // 8)
    assert T == max(1, min(4096, -(-N * P * Q // (4 * lanes))))
    g, partial = Guarded(shape, BF16), Guarded((T, 2, C), F32)
    _lib.call("ttdk_maxpool_bwd_bnstat", _p(dpooled), _p(arg.t), _p(mask.t), _p(y), _p(g.t), _p(partial.t), N, H, W, C,
              P, Q, _lib.stream())
    assert g.intact() and partial.intact()
    keep = O.mask_bools(mask.t, shape)
    want, mag = O.stem_bwd(dpooled, arg.t, keep)
    figs = {"stem_g": O.figure(g.t, want, mag, bf16_store=True)}
    assert bool((g.t[~keep].float() == 0).all())
    # every row of partial is written (idle blocks write zeros), and the rows sum to the sums of the stored g
    assert bool((_bits(partial.t) != 0x5A5A5A5A).all())
    s, smag = O.stem_sums(g.t, y)
    figs["stem_partial"] = O.figure(partial.t.double().sum(0), s, smag)
    w_g, w_partial, w_T = K.maxpool_bwd_bnstat(dpooled, arg.t, mask.t, y)
    assert w_T == T and w_partial.shape[0] == T
    assert _same_bits(w_g, g.t) and _same_bits(w_partial, partial.t)
    _check(figs, ("stem", shape))


# ------------------------------------------------------------------ refusals
def test_refusals_make_no_launch():
    """Every refused call returns an error and leaves its outputs as they were. None of these calls
    could read or write out of bounds if it were launched: the buffers hold 16x16 pixels of 16
    channels, more than any geometry below reaches, and a P or Q of 0 gives a kernel no window."""
    N, H, W, C = 1, 16, 16, 16
    x = torch.randn(N, H, W, C, device=DEV).bfloat16()
    xf = x.float()
    y, arg, dx = Guarded((N, H, W, C), F32), Guarded((N, H, W, C), U8), Guarded((N, H, W, C), F32)
    small, mask, partial = Guarded((N, C), F32), Guarded((N * H * W * C // 8,), U8), Guarded((64, 2, C), F32)
    arg_in = torch.zeros((N, H, W, C), dtype=U8, device=DEV)
    s = _lib.stream

    def refused(name, *args):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args, s())

    def geometry(C_, P, Q, R, S, sh, sw, ph, pw):
        return (N, H, W, C_, P, Q, R, S, sh, sw, ph, pw)

    bad = {
        "C % 8": geometry(12, 7, 7, 3, 3, 2, 2, 0, 0),
        "R*S > 255": geometry(C, 1, 1, 16, 16, 1, 1, 0, 0),
        "ph >= R": geometry(C, 10, 10, 2, 2, 2, 2, 2, 2),       # windows wholly in padding
        "pw >= S": geometry(C, 8, 8, 3, 1, 2, 2, 1, 1),
        "P <= 0": geometry(C, 0, 7, 3, 3, 2, 2, 0, 0),
        "Q <= 0": geometry(C, 7, 0, 3, 3, 2, 2, 0, 0),
    }
    for why, g in bad.items():
        refused("ttdk_maxpool_fwd", _p(x), _p(y.t), _p(arg.t), *g)
        refused("ttdk_maxpool_bwd", _p(x), _p(arg_in), _p(dx.t), *g)
        if why != "C % 8":
            for dt, src in ((0, xf), (1, x)):
                refused("ttdk_maxpool_generic_fwd", _p(src), _p(y.t), _p(arg.t), dt, *g)
                refused("ttdk_maxpool_generic_bwd", _p(src), _p(arg_in), _p(dx.t), dt, *g)
    ok = geometry(C, 7, 7, 3, 3, 2, 2, 0, 0)
    for dt in (2, -1):  # an unknown dtype code
        refused("ttdk_maxpool_generic_fwd", _p(xf), _p(y.t), _p(arg.t), dt, *ok)
        refused("ttdk_maxpool_generic_bwd", _p(xf), _p(arg_in), _p(dx.t), dt, *ok)
        refused("ttdk_gap_fwd", _p(xf), _p(small.t), dt, N, H * W, C)
        refused("ttdk_gap_bwd", _p(xf), _p(dx.t), dt, N, H * W, C)
    refused("ttdk_avgpool_fwd", _p(x), _p(small.t), _p(small.t), N, H * W, 12)
    refused("ttdk_avgpool_bwd", _p(x), _p(dx.t), N, H * W, 12)
    sc = torch.ones(C, device=DEV)
    # the stem fusions: H != 2P, and a channel-group count that does not divide 256 (C = 24)
    refused("ttdk_bn_relu_maxpool", _p(x), _p(sc), _p(sc), _p(y.t), _p(arg.t), _p(mask.t), N, H, W, C, 7, 8)
    refused("ttdk_bn_relu_maxpool", _p(x), _p(sc), _p(sc), _p(y.t), _p(arg.t), _p(mask.t), N, 8, 8, 24, 4, 4)
    refused("ttdk_maxpool_bwd_bnstat", _p(x), _p(arg_in), _p(arg_in), _p(x), _p(dx.t), _p(partial.t), N, H, W, C, 7, 8)
    torch.cuda.synchronize()
    for buf in (y, arg, dx, small, mask, partial):
        assert buf.untouched()


# ------------------------------------------------------------------ ttd.nn
@pytest.mark.parametrize("padding,path", [(1, "fast"), ("VALID", "fast"), ("SAME", "generic")])
def test_nn_max_pool2d_picks_its_path_and_matches(padding, path, monkeypatch):
    """bf16, C = 8, 3x3 / 2 on 8x10: explicit padding 1 and VALID are geometries the fast kernel's
    own output formula gives, so _MaxPool.forward takes it; SAME on even extents pads only at the
    bottom and right (ph = 0 but P = 4, not 3), which only the generic kernel can do."""
    H, W, C = 8, 10, 8
    xc, dc = O.pool_inputs(H, W, C, "border")
    geom = {1: O.explicit(H, W, 3, 2, 1), "VALID": O.valid(H, W, 3, 3, 2, 2), "SAME": O.same(H, W, 3, 3, 2, 2)}[padding]
    x = xc.to(DEV).bfloat16().requires_grad_(True)
    dy = O.cut(dc, geom[6], geom[7]).to(DEV).bfloat16()
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    y = ttd.nn.max_pool2d(x, 3, 2, padding)
    y.backward(dy)
    monkeypatch.undo()
    want_names = {"fast": ["ttdk_maxpool_fwd", "ttdk_maxpool_bwd"],
                  "generic": ["ttdk_maxpool_generic_fwd", "ttdk_maxpool_generic_bwd"]}[path]
    assert [n for n in names if "maxpool" in n] == want_names
    y_ref, first, _ = O.maxpool(x.detach(), geom)
    assert tuple(y.shape) == tuple(y_ref.shape) and _same_values(y.detach(), y_ref)
    want, mag = O.maxpool_bwd(dy, first, x.shape, geom)
    _check({"pool_dx": O.figure(x.grad, want, mag, bf16_store=True)}, ("nn", padding))


def test_zz_report_gpu_maxima():
    """Runs last in this file: the largest figure of the tests above beside its bar."""
    for k in sorted(_seen):
        print("%-14s gpu max %.3e   bar %.1e" % (k, _seen[k], O.BARS[k]))
    assert set(_seen) == set(O.BARS)
