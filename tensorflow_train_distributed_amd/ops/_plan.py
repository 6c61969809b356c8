"""ctypes bindings for the GEMM / convolution launch plans (csrc/kernels/gemm_plan.h through
``libttd_rt.so``): the shape-only decisions of the launchers in ``libttd_hip.so`` — kernel
admission, tiles, split-K clamps, sub-pixel phase order, statistics rows — called from Python
to size buffers and pick paths. The launchers include the same header, so there is one copy
of every rule; it needs no GPU (tests/test_gemm_plan.py)."""
from __future__ import annotations

import ctypes
from collections import namedtuple
from ctypes import c_int, c_longlong

from .. import _native
from ._lib import DG, ConvGeom, DwConvGeom, G

_PI = ctypes.POINTER(c_int)
_TAKES = ("conv_fwd4w", "conv_dgrad4w", "conv_fwd4k8", "conv_dgrad4k8", "conv_wgrad_fp8", "conv_wgrad_bn",
          "conv_dgrad_bnpro", "conv_fwd_bnpro", "conv_wgrad4t", "conv_wgrad4t8")
_SIGS = {
    "conv_size": (c_int, []),
    "big_bn": (c_int, [c_int] * 3),
    "big_bn_wgrad": (c_int, [c_int] * 3),
    "pick_tile": (None, [c_int, c_int, _PI, _PI]),
    "g4t_bm": (c_int, [c_int] * 3),
    "clamp_splits": (c_int, [c_int] * 2),
    "clamp_splits_4t": (c_int, [c_int] * 2),
    "phase_pair": (c_int, [G, c_int, _PI]),
    "dgrad_stat": (None, [G, c_int, _PI, _PI, _PI]),
    "subpixel_stat_rows": (c_longlong, [G]),
    "gemm4t_takes": (c_int, [c_longlong] * 3),
}
_SIGS.update({n + "_takes": (c_int, [G]) for n in _TAKES})
_PL = ctypes.POINTER(c_longlong)
# depthwise convolution (csrc/kernels/dwconv_plan.h), exported as ttd_dwplan_*
_DW_SIGS = {
    "geom_size": (c_int, []),
    "valid": (c_int, [DG]),
    "fast_takes": (c_int, [DG, c_int]),
    "strip": (c_int, []),
    "max_slabs": (c_int, []),
    "wgrad_parts": (c_int, [DG]),
    "slab_rows": (None, [DG, c_int, _PL, _PL]),
    "part_stride": (c_longlong, [DG]),
    "wgrad_ws_floats": (c_longlong, [DG]),
}

_fns = {}


def _fn(name):
    if not _fns:
        lib = _native.rt()
        for n, (res, args) in _SIGS.items():
            f = getattr(lib, "ttd_plan_" + n)
            f.restype, f.argtypes = res, args
            _fns[n] = f
        if _fns["conv_size"]() != ctypes.sizeof(ConvGeom):
            raise RuntimeError("ops._lib.ConvGeom (%d bytes) does not match TtdkConv (%d bytes)"
                               % (ctypes.sizeof(ConvGeom), _fns["conv_size"]()))
    return _fns[name]


def pick_tile(M, N):
    bm, bn = c_int(), c_int()
    _fn("pick_tile")(M, N, bm, bn)
    return bm.value, bn.value


Phase = namedtuple("Phase", "r0 T off n")  # one axis: first tap, tap count, padding offset, extent


def subpixel_phases(g):
    """(row Phase, column Phase) of every non-empty sub-pixel phase of the stride-s data gradient
    with geometry g, in ttdk_conv_dgrad_subpixel's launch order."""
    out = []
    v = (c_int * 8)()
    for i in range(g.sh * g.sh):
        if _fn("phase_pair")(ctypes.byref(g), i, v):
            out.append((Phase(*v[:4]), Phase(*v[4:])))
    return out


def dgrad_stat(g, stat_4w_k):
    """(bm, bn, rows) of a unit-stride data gradient with the BN-statistics epilogue."""
    bm, bn, rows = c_int(), c_int(), c_int()
    _fn("dgrad_stat")(ctypes.byref(g), stat_4w_k, bm, bn, rows)
    return bm.value, bn.value, rows.value


def takes(launcher, g) -> bool:
    """Whether `launcher` (ttdk_<launcher>) admits geometry g, as far as the shape decides."""
    return bool(_fn(launcher + "_takes")(ctypes.byref(g)))


def _direct(name):
    return lambda *args: _fn(name)(*args)


# big_bn(M, N, K), big_bn_wgrad(M, N, K), g4t_bm(M, rowsum, bm128_enabled), clamp_splits(ktiles, splits),
# clamp_splits_4t(ktiles, splits), gemm4t_takes(M, N, K): arguments and results as in gemm_plan.h
big_bn, big_bn_wgrad, g4t_bm, clamp_splits, clamp_splits_4t, gemm4t_takes = map(
    _direct, ("big_bn", "big_bn_wgrad", "g4t_bm", "clamp_splits", "clamp_splits_4t", "gemm4t_takes"))


def subpixel_stat_rows(g):
    return _fn("subpixel_stat_rows")(ctypes.byref(g))


# ------------------------------------------------------------------ depthwise convolution
_dw_fns = {}


def _dw(name):
    if not _dw_fns:
        lib = _native.rt()
        for n, (res, args) in _DW_SIGS.items():
            f = getattr(lib, "ttd_dwplan_" + n)
            f.restype, f.argtypes = res, args
            _dw_fns[n] = f
        if _dw_fns["geom_size"]() != ctypes.sizeof(DwConvGeom):
            raise RuntimeError("ops._lib.DwConvGeom (%d bytes) does not match TtdkDwConv (%d bytes)"
                               % (ctypes.sizeof(DwConvGeom), _dw_fns["geom_size"]()))
    return _dw_fns[name]


def dw_geom(x_shape, w_shape, sh, sw, ph, pw, dh, dw, P, Q):
    """DwConvGeom of input [N,H,W,C] and filter [R,S,C,M]."""
    N, H, W, C = (int(v) for v in x_shape)
    R, S, _, M = (int(v) for v in w_shape)
    return DwConvGeom(N, H, W, C, M, R, S, int(P), int(Q), int(sh), int(sw), int(ph), int(pw), int(dh), int(dw))


def dw_valid(g) -> bool:
    return bool(_dw("valid")(ctypes.byref(g)))


def dw_fast_takes(g, bf16: bool) -> bool:
    """Whether the fast form admits geometry g, as far as shape and dtype decide (the launchers
    also want 16-byte aligned bases)."""
    return bool(_dw("fast_takes")(ctypes.byref(g), 1 if bf16 else 0))


def dw_strip() -> int:
    """Output columns a fast-form thread produces."""
    return _dw("strip")()


def dw_max_slabs() -> int:
    return _dw("max_slabs")()


def dw_wgrad_parts(g) -> int:
    """Slabs T of the weight gradient's N*P output rows."""
    return _dw("wgrad_parts")(ctypes.byref(g))


def dw_slab_rows(g, t):
    """[r0, r1) of slab t."""
    r0, r1 = c_longlong(), c_longlong()
    _dw("slab_rows")(ctypes.byref(g), t, r0, r1)
    return r0.value, r1.value


def dw_part_stride(g) -> int:
    return _dw("part_stride")(ctypes.byref(g))


def dw_wgrad_ws_floats(g) -> int:
    return _dw("wgrad_ws_floats")(ctypes.byref(g))


# ------------------------------------------------------------------ group normalisation
# csrc/kernels/groupnorm_plan.h, exported as ttd_gnplan_*; shapes are x [N, M, C] with G groups
_GN_SIGS = {
    "valid": (c_int, [c_longlong] * 4),
    "fast_takes": (c_int, [c_longlong] * 4 + [c_int]),
    "max_slabs": (c_int, []),
    "max_ws_floats": (c_longlong, []),
    "lanes": (c_int, [c_longlong, c_int]),
    "rows_per_block": (c_int, [c_longlong, c_int]),
    "part_stride": (c_longlong, [c_longlong]),
    "rows_per_slab": (c_longlong, [c_longlong] * 3),
    "parts": (c_int, [c_longlong] * 3),
    "slab_rows": (None, [c_longlong] * 3 + [c_int, _PL, _PL]),
    "fwd_ws_floats": (c_longlong, [c_longlong] * 3),
    "bwd_ws_floats": (c_longlong, [c_longlong] * 3),
}
_gn_fns = {}


def _gn(name):
    if not _gn_fns:
        lib = _native.rt()
        for n, (res, args) in _GN_SIGS.items():
            f = getattr(lib, "ttd_gnplan_" + n)
            f.restype, f.argtypes = res, args
            _gn_fns[n] = f
    return _gn_fns[name]


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
    _gn("slab_rows")(N, M, C, t, r0, r1)
    return r0.value, r1.value


def gn_fwd_ws_floats(N, M, C) -> int:
    return _gn("fwd_ws_floats")(N, M, C)


def gn_bwd_ws_floats(N, M, C) -> int:
    return _gn("bwd_ws_floats")(N, M, C)
