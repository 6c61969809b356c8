"""ctypes bindings for the GEMM / convolution launch plans (csrc/kernels/gemm_plan.h through
``libttd_rt.so``): the shape-only decisions of the launchers in ``libttd_hip.so`` — kernel
admission, tiles, split-K clamps, sub-pixel phase order, statistics rows — called from Python
to size buffers and pick paths. The launchers include the same header, so there is one copy
of every rule; it needs no GPU (tests/test_gemm_plan.py)."""
from __future__ import annotations

from collections import namedtuple
from ctypes import byref, c_int, c_longlong

from . import _lib
from ._lib import DwConvGeom


def _family(prefix):
    """name -> export prefix + name of libttd_rt.so, typed from the library's own signature table."""
    fns = {}

    def fn(name):
        f = fns.get(name)
        if f is None:
            f = fns[name] = _lib.rt_fn(prefix + name)
        return f
    return fn


# gemm_plan.h, dwconv_plan.h (depthwise convolution) and groupnorm_plan.h (group normalisation;
# shapes are x [N, M, C] with G groups)
_fn, _dw, _gn = _family("ttd_plan_"), _family("ttd_dwplan_"), _family("ttd_gnplan_")


def pick_tile(M, N):
    bm, bn = c_int(), c_int()
    _fn("pick_tile")(M, N, byref(bm), byref(bn))
    return bm.value, bn.value


Phase = namedtuple("Phase", "r0 T off n")  # one axis: first tap, tap count, padding offset, extent


def subpixel_phases(g):
    """(row Phase, column Phase) of every non-empty sub-pixel phase of the stride-s data gradient
    with geometry g, in ttdk_conv_dgrad_subpixel's launch order."""
    out = []
    v = (c_int * 8)()
    for i in range(g.sh * g.sh):
        if _fn("phase_pair")(byref(g), i, v):
            out.append((Phase(*v[:4]), Phase(*v[4:])))
    return out


def dgrad_stat(g, stat_4w_k):
    """(bm, bn, rows) of a unit-stride data gradient with the BN-statistics epilogue."""
    bm, bn, rows = c_int(), c_int(), c_int()
    _fn("dgrad_stat")(byref(g), stat_4w_k, byref(bm), byref(bn), byref(rows))
    return bm.value, bn.value, rows.value


def takes(launcher, g) -> bool:
    """Whether `launcher` (ttdk_<launcher>) admits geometry g, as far as the shape decides."""
    return bool(_fn(launcher + "_takes")(byref(g)))


def _direct(name):
    return lambda *args: _fn(name)(*args)


# big_bn(M, N, K), big_bn_wgrad(M, N, K), g4t_bm(M, rowsum, bm128_enabled), clamp_splits(ktiles, splits),
# clamp_splits_4t(ktiles, splits), gemm4t_takes(M, N, K): arguments and results as in gemm_plan.h
big_bn, big_bn_wgrad, g4t_bm, clamp_splits, clamp_splits_4t, gemm4t_takes = map(
    _direct, ("big_bn", "big_bn_wgrad", "g4t_bm", "clamp_splits", "clamp_splits_4t", "gemm4t_takes"))


def subpixel_stat_rows(g):
    return _fn("subpixel_stat_rows")(byref(g))


# ------------------------------------------------------------------ depthwise convolution
def dw_geom(x_shape, w_shape, sh, sw, ph, pw, dh, dw, P, Q):
    """DwConvGeom of input [N,H,W,C] and filter [R,S,C,M]."""
    N, H, W, C = (int(v) for v in x_shape)
    R, S, _, M = (int(v) for v in w_shape)
    return DwConvGeom(N, H, W, C, M, R, S, int(P), int(Q), int(sh), int(sw), int(ph), int(pw), int(dh), int(dw))


def dw_valid(g) -> bool:
    return bool(_dw("valid")(byref(g)))


def dw_fast_takes(g, bf16: bool) -> bool:
    """Whether the fast form admits geometry g, as far as shape and dtype decide (the launchers
    also want 16-byte aligned bases)."""
    return bool(_dw("fast_takes")(byref(g), 1 if bf16 else 0))


def dw_strip() -> int:
    """Output columns a fast-form thread produces."""
    return _dw("strip")()


def dw_max_slabs() -> int:
    return _dw("max_slabs")()


def dw_wgrad_parts(g) -> int:
    """Slabs T of the weight gradient's N*P output rows."""
    return _dw("wgrad_parts")(byref(g))


def dw_slab_rows(g, t):
    """[r0, r1) of slab t."""
    r0, r1 = c_longlong(), c_longlong()
    _dw("slab_rows")(byref(g), t, byref(r0), byref(r1))
    return r0.value, r1.value


def dw_part_stride(g) -> int:
    return _dw("part_stride")(byref(g))


def dw_wgrad_ws_floats(g) -> int:
    return _dw("wgrad_ws_floats")(byref(g))


# ------------------------------------------------------------------ group normalisation
def gn_valid(N, M, C, G) -> bool:
    return bool(_gn("valid")(N, M, C, G))


def gn_fast_takes(N, M, C, G, bf16: bool) -> bool:
    """Whether the fast form admits the shape, as far as shape and dtype decide (the launchers
    also want 16-byte aligned bases)."""
    return bool(_gn("fast_takes")(N, M, C, G, 1 if bf16 else 0))


def gn_max_slabs() -> int:
    return _gn("max_slabs")()


def gn_max_ws_floats() -> int:
    return _gn("max_ws_floats")()


def gn_lanes(C, fast: bool) -> int:
    """Lanes that share one pixel row in a streaming block."""
    return _gn("lanes")(C, int(fast))


def gn_rows_per_block(C, fast: bool) -> int:
    """Pixel rows a streaming block has in flight."""
    return _gn("rows_per_block")(C, int(fast))


def gn_part_stride(C) -> int:
    return _gn("part_stride")(C)


def gn_rows_per_slab(N, M, C) -> int:
    return _gn("rows_per_slab")(N, M, C)


def gn_parts(N, M, C) -> int:
    """Slabs T the M pixel rows of every image are cut into."""
    return _gn("parts")(N, M, C)


def gn_slab_rows(N, M, C, t):
    """[r0, r1) of slab t of an image."""
    r0, r1 = c_longlong(), c_longlong()
    _gn("slab_rows")(N, M, C, t, byref(r0), byref(r1))
    return r0.value, r1.value


def gn_fwd_ws_floats(N, M, C) -> int:
    return _gn("fwd_ws_floats")(N, M, C)


def gn_bwd_ws_floats(N, M, C) -> int:
    return _gn("bwd_ws_floats")(N, M, C)
