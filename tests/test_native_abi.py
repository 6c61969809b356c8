"""The ctypes types of every call into libttd_hip.so and of the plan exports of libttd_rt.so come
from the libraries' own signature tables (csrc/kernels/abi.h, ops/_lib.py). No GPU needed: the
libraries load on a CPU-only machine."""
import ast
import ctypes
import pathlib

import pytest

from tensorflow_train_distributed_amd import _native
from tensorflow_train_distributed_amd.ops import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
PREFIX = {"hip": "ttdk_abi", "rt": "ttd_abi"}
# exports of libttd_rt.so that go through the table (its other ttd_* exports keep their own bindings)
RT_FAMILIES = ("ttd_plan_", "ttd_dwplan_", "ttd_gnplan_", "ttd_ipc_", "ttd_collective_plan")
ABSENT = "ttdk_no_such_launcher"
PLAN_HELPERS = {"_fn": "ttd_plan_", "_dw": "ttd_dwplan_", "_gn": "ttd_gnplan_"}  # ops/_plan.py


@pytest.mark.parametrize("kind", ["hip", "rt"])
def test_every_entry_decodes(kind):
    sigs = _lib.signatures(kind)
    assert len(sigs) >= {"hip": 188, "rt": 50}[kind]
    lib = {"hip": _native.hip, "rt": _native.rt}[kind]()
    for name, sig in sigs.items():
        restype, argtypes = _lib.decode(name, sig)  # raises on an unknown letter
        f = getattr(lib, name)
        assert (f.restype, list(f.argtypes)) == (restype, argtypes), name
    # the two functions typed by hand to read the table are entries of it, with those very types
    for suffix, by_hand in _lib._BOOT.items():
        assert sigs[PREFIX[kind] + suffix] == by_hand


def test_decoded_types():
    sigs = _lib.signatures("hip")
    assert _lib.decode("f", sigs["ttdk_conv_fwd"]) == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_lib.ConvGeom), ctypes.c_int, ctypes.c_int,
                       ctypes.POINTER(_lib.Epilogue), ctypes.c_void_p])
    assert sigs["ttdk_dwconv_wgrad_ws_floats"] == "l:D"
    assert sigs["ttdc_error"] == "z:P" and sigs["ttdc_destroy"] == "v:Pi"
    assert sigs["ttdk_bias_act_dropout_fwd"] == "i:PPPliifQQiP"
    # the `unsigned` arguments of the attention and row-norm launchers
    for name in ("ttdk_attn_fwd", "ttdk_attn_bwd", "ttdk_attn_band_fwd", "ttdk_attn_band_bwd", "ttdk_ln_fwd",
                 "ttdk_ln_bwd", "ttdk_rms_fwd", "ttdk_rms_bwd"):
        assert "u" in sigs[name], name
    with pytest.raises(_lib.HipKernelError, match="ttdk_x"):
        _lib.decode("ttdk_x", "i:Pb")


def _names_used():
    """(export name, file) of every native function the Python sources name in a call."""
    hip, rt = [], []
    files = [p for d in ("tensorflow_train_distributed_amd", "tests", "tools") for p in sorted((ROOT / d).rglob("*.py"))]
    for path in files:
        for node in ast.walk(ast.parse(path.read_text(), str(path))):
            if isinstance(node, ast.Attribute) and node.attr.startswith(("ttdk_", "ttdc_", "ttdi_")):
                hip.append((node.attr, path.name))  # lib.ttdc_join(...)
            elif isinstance(node, ast.Attribute) and node.attr.startswith(RT_FAMILIES):
                rt.append((node.attr, path.name))
            if not (isinstance(node, ast.Call) and node.args and isinstance(node.args[0], ast.Constant)
                    and isinstance(node.args[0].value, str)):
                continue
            first, func = node.args[0].value, node.func
            if isinstance(func, ast.Attribute) and func.attr in ("call", "query", "fn") and first.startswith("ttdk_"):
                hip.append((first, path.name))  # _lib.call("ttdk_...", ...)
            elif path.name == "_plan.py" and isinstance(func, ast.Name) and func.id in PLAN_HELPERS:
                rt.append((PLAN_HELPERS[func.id] + first, path.name))  # _fn("pick_tile")
    return hip, rt


def test_every_name_python_calls_is_in_the_table():
    hip, rt = _names_used()
    assert len({n for n, _ in hip}) > 150 and len({n for n, _ in rt}) > 30  # the walk found the call sites
    for used, kind in ((hip, "hip"), (rt, "rt")):
        sigs = _lib.signatures(kind)
        missing = sorted({(n, f) for n, f in used if n not in sigs})
        assert not missing, missing


def test_struct_layouts():
    lib = _lib.hip()  # the load itself compares the three layouts and raises on a difference
    for code, cls in _lib._STRUCTS.items():
        out = (ctypes.c_longlong * 64)()
        n = lib.ttdk_abi_layout(ord(code), out, len(out))
        assert n == 1 + len(cls._fields_)
        assert out[0] == ctypes.sizeof(cls)
        assert list(out[1:n]) == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert lib.ttdk_abi_layout(ord("x"), out, len(out)) == -1
    rt = _lib.rt()
    assert rt.ttd_plan_conv_size() == ctypes.sizeof(_lib.ConvGeom) == 60
    assert rt.ttd_dwplan_geom_size() == ctypes.sizeof(_lib.DwConvGeom) == 60
    assert ctypes.sizeof(_lib.Epilogue) == 168


def test_arity_is_checked_before_the_call():
    assert _lib.query("ttdk_conv3_rows", 56, 56, 64, 64, 0) == 448  # as before the table existed
    with pytest.raises(TypeError, match="ttdk_conv3_rows takes 5 arguments, 4 given"):
        _lib.query("ttdk_conv3_rows", 56, 56, 64, 64)
    # ctypes alone passes a surplus argument of a cdecl function along
    with pytest.raises(TypeError, match="ttdk_conv3_rows takes 5 arguments, 6 given"):
        _lib.query("ttdk_conv3_rows", 56, 56, 64, 64, 0, 7)
    with pytest.raises(TypeError, match="ttdk_zero takes 3 arguments, 4 given"):
        _lib.call("ttdk_zero", None, 0, None, None)


def test_call_refuses_a_function_that_returns_no_error_code():
    with pytest.raises(TypeError, match="ttdk_gemm4t_ws returns 'l'"):
        _lib.call("ttdk_gemm4t_ws", 256, 256, 256, 1)
    assert _lib.query("ttdk_gemm4t_ws", 256, 256, 256, 1) >= 0


def test_unknown_name_raises_with_the_name():
    with pytest.raises(_lib.HipKernelError, match=ABSENT):
        _lib.fn(ABSENT)
    with pytest.raises(_lib.HipKernelError, match=ABSENT):
        _lib.call(ABSENT, 1)
    with pytest.raises(_lib.HipKernelError, match="ttd_plan_no_such_rule"):
        _lib.rt_fn("ttd_plan_no_such_rule")
    # an export of libttd_rt.so outside the table is not handed out untyped
    assert hasattr(_native.rt(), "ttd_last_error")
    with pytest.raises(_lib.HipKernelError, match="ttd_last_error"):
        _lib.rt_fn("ttd_last_error")
