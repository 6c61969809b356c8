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
from ._lib import ConvGeom, G

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
