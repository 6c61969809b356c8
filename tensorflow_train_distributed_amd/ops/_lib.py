"""ctypes bindings for ``libttd_hip.so`` (the gfx950 kernel library).

Every kernel launcher has the C signature ``int ttdk_*(..., hipStream_t)``; this module
launches them on PyTorch's *current* HIP stream, so the kernels compose with torch's stream
semantics, ``torch.cuda.graphs`` capture (hipGraph) and the collective engine's side streams.
A non-zero return (hipError_t) raises immediately.

Argument and return types are not written here. Each library records the signature of every
function defined with ``TTDK_API`` / ``TTD_API`` (csrc/kernels/abi.h), computed from the C
function's own type, and :func:`hip` / :func:`rt` set ``argtypes`` and ``restype`` of all of them
from that table when the library is loaded. To add an export, write it with ``TTDK_API`` and
call it: that is all. A name the table lacks, a letter this module does not know, a wrong
number of arguments or a struct whose layout differs from its mirror below raises.

There is deliberately no fallback here: a GPU op whose kernel library is missing or fails
to load raises (the CPU path of each op lives in :mod:`.reference`).
"""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_uint, c_uint64, c_void_p

import torch

from .. import _native


class Epilogue(ctypes.Structure):
    """Mirror of ``TtdkEpilogue`` in gemm_conv.h."""

    _fields_ = [
        ("mode", c_int), ("out", c_void_p), ("ldo", c_longlong), ("slab_stride", c_longlong),
        ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_longlong), ("act", c_int),
        ("beta", c_int), ("remap", c_int), ("rP", c_int), ("rQ", c_int), ("rOH", c_int),
        ("rOW", c_int), ("rs", c_int), ("stat", c_void_p), ("alpha", c_float), ("aux", c_void_p),
        ("ascale0", c_void_p), ("ascale1", c_void_p), ("by", c_void_p), ("bmask", c_void_p),
        ("by2", c_void_p), ("stat2", c_void_p), ("bH", c_int), ("bW", c_int),
    ]


class ConvGeom(ctypes.Structure):
    """Mirror of ``TtdkConv``: input NHWC [N,H,W,C], filter [K,R,S,C], output [N,P,Q,K]."""

    _fields_ = [(n, c_int) for n in ("N", "H", "W", "C", "K", "R", "S", "P", "Q", "sh", "sw", "ph", "pw", "dh", "dw")]


class DwConvGeom(ctypes.Structure):
    """Mirror of ``TtdkDwConv`` (dwconv_plan.h): input NHWC [N,H,W,C], filter [R,S,C,M], output [N,P,Q,C*M]."""

    _fields_ = [(n, c_int) for n in ("N", "H", "W", "C", "M", "R", "S", "P", "Q", "sh", "sw", "ph", "pw", "dh", "dw")]


class HipKernelError(RuntimeError):
    pass


# signature letter (abi.h) -> ctypes type; structs are passed by reference
_STRUCTS = {"E": Epilogue, "G": ConvGeom, "D": DwConvGeom}
_CODES = {"v": None, "i": c_int, "u": c_uint, "l": c_longlong, "Q": c_uint64, "f": c_float, "d": c_double,
          "P": c_void_p, "z": c_char_p, **{k: ctypes.POINTER(v) for k, v in _STRUCTS.items()}}
# the table's own two functions: the only types set by hand (and entries of the table like any other)
_BOOT = {"_count": "i:", "_entry": "z:i"}


def decode(name, sig):
    """(restype, argtypes) of signature ``ret:args``."""
    try:
        ret, args = sig.split(":")
        return _CODES[ret], [_CODES[c] for c in args]
    except (KeyError, ValueError):
        raise HipKernelError("%s: signature %r has a type code this module does not know" % (name, sig)) from None


def _bind(lib, prefix):
    """Set argtypes / restype of every function in `lib`'s signature table; name -> signature."""
    try:
        boot = {n: getattr(lib, prefix + n) for n in _BOOT}
    except AttributeError:
        raise HipKernelError("%s has no signature table (%s_count): it was built before the table existed, "
                             "so no call into it can be typed" % (lib._name, prefix)) from None
    for n, f in boot.items():
        f.restype, f.argtypes = decode(prefix + n, _BOOT[n])
    sigs = dict(boot["_entry"](i).decode().split(" ") for i in range(boot["_count"]()))
    for name, sig in sigs.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = decode(name, sig)
    return sigs


def _check_size(cls, size):
    if ctypes.sizeof(cls) != size:
        raise HipKernelError("ops._lib.%s (%d bytes) does not match its C struct (%d bytes)"
                             % (cls.__name__, ctypes.sizeof(cls), size))


_sigs = {}


def hip():
    """libttd_hip.so with every export typed; checks the three struct mirrors field by field."""
    lib = _native.hip()
    if "hip" not in _sigs:
        sigs = _bind(lib, "ttdk_abi")
        for code, cls in _STRUCTS.items():
            out = (c_longlong * 64)()
            n = lib.ttdk_abi_layout(ord(code), out, len(out))
            mine = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
            if mine != list(out[:max(n, 0)]):
                raise HipKernelError("ops._lib.%s does not match its C struct: size and field offsets %s here, %s in %s"
                                     % (cls.__name__, mine, list(out[:max(n, 0)]), lib._name))
        _sigs["hip"] = sigs
    return lib


def rt():
    """libttd_rt.so with its plan exports typed (the other ttd_* exports keep their own bindings)."""
    lib = _native.rt()
    if "rt" not in _sigs:
        sigs = _bind(lib, "ttd_abi")
        _check_size(ConvGeom, lib.ttd_plan_conv_size())
        _check_size(DwConvGeom, lib.ttd_dwplan_geom_size())
        _sigs["rt"] = sigs
    return lib


def signatures(kind):
    """name -> ``ret:args`` of every typed export of the "hip" or "rt" library."""
    (hip if kind == "hip" else rt)()
    return _sigs[kind]


def _typed(kind, name):
    sig = signatures(kind).get(name)
    if sig is None:
        raise HipKernelError("%s is not in the signature table of libttd_%s.so" % (name, kind))
    return getattr((_native.hip if kind == "hip" else _native.rt)(), name), sig


def rt_fn(name):
    """Plan export `name` of libttd_rt.so."""
    return _typed("rt", name)[0]


_fns = {}  # name -> (function, number of arguments, return code)


def _entry(name):
    e = _fns.get(name)
    if e is None:
        f, sig = _typed("hip", name)
        e = _fns[name] = (f, len(sig) - 2, sig[0])
    return e


def fn(name):
    return _entry(name)[0]


def _arity(name, n, given):
    # ctypes itself only catches too few arguments: a surplus one would be passed along
    raise TypeError("%s takes %d arguments, %d given" % (name, n, given))


# Per-launch timing for profiling tools (TTD_OP_TIMING=1): every call is bracketed by HIP
# events on the current stream and labelled with the GEMM shapes ops.gemm logged for it.
import os as _os
TIMING = [] if _os.environ.get("TTD_OP_TIMING") else None
_labels = []


def label(x):
    if TIMING is not None:
        _labels.append(x)


def call(name, *args):
    f, n, ret = _fns.get(name) or _entry(name)
    if len(args) != n:
        _arity(name, n, len(args))
    if ret != "i":
        raise TypeError("%s returns %r, not a hipError_t: use query()" % (name, ret))
    if TIMING is not None:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        rc = f(*args)
        e.record()
        TIMING.append((name, list(_labels), s, e))
        _labels.clear()
    else:
        rc = f(*args)
    if rc != 0:
        raise HipKernelError("%s failed with hipError_t %d" % (name, rc))


def query(name, *args):
    """Call a host-side helper that returns a plain int (not a hipError_t)."""
    f, n, _ = _fns.get(name) or _entry(name)
    if len(args) != n:
        _arity(name, n, len(args))
    return f(*args)


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())
