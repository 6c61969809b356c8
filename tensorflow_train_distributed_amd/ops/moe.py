"""Launch wrappers for the mixture-of-experts routing kernels (moe_route.hip): the router's
softmax / top-k and its backward, the counting sort of the (token, choice) slots by expert, and the
row gather / weighted k-way sum that dispatch tokens to sorted rows and combine them again.

Every wrapper checks its operands and raises InvalidArgumentError with the offending shape before
anything is launched. Nothing here reads routing data on the host, so every call can be captured
into a graph. Row operands ("rows") are 2-D float32 / bfloat16 CUDA tensors whose rows may be
strided: width and row stride multiples of 8, base 16-byte aligned."""
from __future__ import annotations

import torch

from . import _lib
from ..utils.errors import InvalidArgumentError

_DT = {torch.float32: 0, torch.bfloat16: 1}


def max_experts() -> int:
    """The largest E of topk_route."""
    return _lib.query("ttdk_moe_max_experts")


def max_topk() -> int:
    return _lib.query("ttdk_moe_max_topk")


def sort_chunk() -> int:
    """Slots per chunk of sort_by_expert's counting sort."""
    return _lib.query("ttdk_moe_sort_chunk")


def _check_dense(name, t, what, dtype, shape, dev=None):
    if (t.dtype != dtype or not t.is_cuda or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or (dev is not None and t.device != dev)):
        raise InvalidArgumentError("%s: %s must be a contiguous CUDA %s tensor of shape %s%s (got %s %s shape %s strides %s)"
                                   % (name, what, dtype, tuple(shape), "" if dev is None else " on %s" % dev, t.dtype,
                                      t.device, tuple(t.shape), t.stride()))


def _check_route_shape(name, T, E, k):
    if E < 1 or E > max_experts() or k < 1 or k > max_topk() or k > E:
        raise InvalidArgumentError("%s: need 1 <= k <= min(E, %d) and E <= %d, got E = %d, k = %d (T = %d)"
                                   % (name, max_topk(), max_experts(), E, k, T))


def _check_rows(name, t, what, cols=None, dev=None):
    if t.dtype not in _DT or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or (dev is not None and t.device != dev):
        raise InvalidArgumentError("%s: %s must be a row-major 2-D CUDA float32 / bfloat16 tensor%s (got %s %s shape %s "
                                   "strides %s)" % (name, what, "" if dev is None else " on %s" % dev, t.dtype, t.device,
                                                    tuple(t.shape), t.stride()))
    if cols is not None and t.shape[1] != cols:
        raise InvalidArgumentError("%s: %s must have %d columns, got shape %s" % (name, what, cols, tuple(t.shape)))
    if t.shape[1] < 8 or t.shape[1] % 8 or t.stride(0) % 8 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        raise InvalidArgumentError("%s: %s needs a width and a row stride that are multiples of 8 and a 16-byte "
                                   "aligned base (shape %s, row stride %d, base %% 16 = %d)"
                                   % (name, what, tuple(t.shape), t.stride(0), t.data_ptr() % 16))


def _out_rows(name, out, rows, D, dtype, dev):
    if out is None:
        if dtype not in _DT:
            raise InvalidArgumentError("%s: the output dtype must be float32 or bfloat16, got %s" % (name, dtype))
        return torch.empty((rows, D), dtype=dtype, device=dev)
    _check_rows(name, out, "out", D, dev)
    if out.shape[0] != rows:
        raise InvalidArgumentError("%s: out must be [%d, %d], got %s" % (name, rows, D, tuple(out.shape)))
    return out


def topk_route(logits, k, *, out=None):
    """(probs, expert, gate) of fp32 logits [T, E] (rows may be strided): probs = softmax(logits)
    [T, E]; expert int32 [T, k] the k largest logits of each row, descending, ties to the lowest
    index, NaN first; gate fp32 [T, k] the selected probs over their sum. out: the three tensors to
    write (contiguous)."""
    name = "topk_route"
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2 or (logits.shape[1] and logits.stride(1) != 1):
        raise InvalidArgumentError("%s: logits must be a row-major 2-D CUDA float32 tensor (got %s %s shape %s strides %s)"
                                   % (name, logits.dtype, logits.device, tuple(logits.shape), logits.stride()))
    T, E = logits.shape
    k = int(k)
    _check_route_shape(name, T, E, k)
    if T and logits.stride(0) < E:
        raise InvalidArgumentError("%s: logits rows overlap (shape %s strides %s)" % (name, tuple(logits.shape), logits.stride()))
    dev = logits.device
    if out is None:
        out = (torch.empty((T, E), dtype=torch.float32, device=dev), torch.empty((T, k), dtype=torch.int32, device=dev),
               torch.empty((T, k), dtype=torch.float32, device=dev))
    probs, expert, gate = out
    _check_dense(name, probs, "probs", torch.float32, (T, E), dev)
    _check_dense(name, expert, "expert", torch.int32, (T, k), dev)
    _check_dense(name, gate, "gate", torch.float32, (T, k), dev)
    if T:
        _lib.call("ttdk_moe_topk", logits.data_ptr(), logits.stride(0), probs.data_ptr(), expert.data_ptr(),
                  gate.data_ptr(), T, E, k, _lib.stream())
    return probs, expert, gate


def topk_route_bwd(probs, expert, gate, dgate=None, dprobs=None, *, out=None):
    """dlogits fp32 [T, E] of topk_route from the gradients of gate ([T, k]) and / or probs ([T, E]);
    an absent one counts as zeros."""
    name = "topk_route_bwd"
    if probs.dim() != 2 or expert.dim() != 2:
        raise InvalidArgumentError("%s: probs must be [T, E] and expert [T, k], got %s and %s"
                                   % (name, tuple(probs.shape), tuple(expert.shape)))
    (T, E), k = probs.shape, expert.shape[1]
    _check_route_shape(name, T, E, k)
    _check_dense(name, probs, "probs", torch.float32, (T, E))
    dev = probs.device
    _check_dense(name, expert, "expert", torch.int32, (T, k), dev)
    _check_dense(name, gate, "gate", torch.float32, (T, k), dev)
    if dgate is None and dprobs is None:
        raise InvalidArgumentError("%s: neither dgate nor dprobs given (T = %d, E = %d, k = %d)" % (name, T, E, k))
    if dgate is not None:
        _check_dense(name, dgate, "dgate", torch.float32, (T, k), dev)
    if dprobs is not None:
        _check_dense(name, dprobs, "dprobs", torch.float32, (T, E), dev)
    if out is None:
        out = torch.empty((T, E), dtype=torch.float32, device=dev)
    _check_dense(name, out, "out", torch.float32, (T, E), dev)
    if T:
        _lib.call("ttdk_moe_topk_bwd", probs.data_ptr(), expert.data_ptr(), gate.data_ptr(), _lib.ptr(dgate),
                  _lib.ptr(dprobs), out.data_ptr(), T, E, k, _lib.stream())
    return out


def sort_workspace(S, E, device):
    """The int32 workspace sort_by_expert needs for S slots and E experts."""
    n = _lib.query("ttdk_moe_sort_ws_bytes", int(S), int(E))
    if n < 0:
        raise InvalidArgumentError("sort_by_expert: E must be in [1, %d], got E = %d (S = %d)"
                                   % (_lib.query("ttdk_moe_sort_max_experts"), E, S))
    return torch.empty(n // 4, dtype=torch.int32, device=device)


def sort_by_expert(expert, E, *, out=None, workspace=None):
    """Stable counting sort of the int32 expert ids (any shape, S elements, slot = flat index):
    (offsets int32 [E + 1], order int32 [S] sorted row -> slot, inv int32 [S] slot -> sorted row).
    offsets is the table grouped_gemm reads; ids outside [0, E) sort after offsets[E]. The same
    permutation as torch.argsort(stable=True) of the clamped ids."""
    name = "sort_by_expert"
    E = int(E)
    if expert.dtype != torch.int32 or not expert.is_cuda or not expert.is_contiguous():
        raise InvalidArgumentError("%s: expert must be a contiguous CUDA int32 tensor (got %s %s shape %s strides %s)"
                                   % (name, expert.dtype, expert.device, tuple(expert.shape), expert.stride()))
    S, dev = expert.numel(), expert.device
    if E < 1 or E > _lib.query("ttdk_moe_sort_max_experts"):
        raise InvalidArgumentError("%s: E must be in [1, %d], got E = %d (expert %s)"
                                   % (name, _lib.query("ttdk_moe_sort_max_experts"), E, tuple(expert.shape)))
    if out is None:
        out = (torch.empty(E + 1, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev),
               torch.empty(S, dtype=torch.int32, device=dev))
    offsets, order, inv = out
    _check_dense(name, offsets, "offsets", torch.int32, (E + 1,), dev)
    _check_dense(name, order, "order", torch.int32, (S,), dev)
    _check_dense(name, inv, "inv", torch.int32, (S,), dev)
    if S == 0:
        offsets.zero_()
        return offsets, order, inv
    if workspace is None:
        workspace = sort_workspace(S, E, dev)
    _check_dense(name, workspace, "workspace", torch.int32, (_lib.query("ttdk_moe_sort_ws_bytes", S, E) // 4,), dev)
    _lib.call("ttdk_moe_sort", expert.data_ptr(), S, E, offsets.data_ptr(), order.data_ptr(), inv.data_ptr(),
              workspace.data_ptr(), _lib.stream())
    return offsets, order, inv


def gather_rows(src, idx, k=1, *, scale=None, h=None, dtype=None, out=None):
    """out[r] = scale[idx[r]] * src[idx[r] // k] for the int32 idx [R] over the src.shape[0] * k
    slots (scale fp32 [slots] or None: 1); an idx entry outside the slots gives a zero row. src and
    out are rows of float32 or bfloat16, converted in flight (dtype: of a new out, default src's).
    With h (rows [R, D] of out's dtype) returns (out, dgate) with dgate[idx[r]] = dot(h[r],
    src[idx[r] // k]), fp32 [slots]: the backward of combine_rows in one pass. dgate is written
    where idx points, all of it when idx is a permutation of the slots."""
    name = "gather_rows"
    _check_rows(name, src, "src")
    dev, (n_src, D), k = src.device, src.shape, int(k)
    if idx.dtype != torch.int32 or idx.device != dev or idx.dim() != 1 or not idx.is_contiguous():
        raise InvalidArgumentError("%s: idx must be a contiguous 1-D int32 tensor on %s (got %s %s shape %s)"
                                   % (name, dev, idx.dtype, idx.device, tuple(idx.shape)))
    if k < 1 or k > 256 or n_src * k >= 2 ** 30:
        raise InvalidArgumentError("%s: need 1 <= k <= 256 and fewer than 2^30 slots, got k = %d, src %s"
                                   % (name, k, tuple(src.shape)))
    R, slots = idx.shape[0], n_src * k
    if n_src == 0 and R:
        raise InvalidArgumentError("%s: %d rows asked of an empty src %s" % (name, R, tuple(src.shape)))
    if scale is not None and (scale.dtype != torch.float32 or scale.device != dev or scale.numel() != slots
                              or not scale.is_contiguous()):
        raise InvalidArgumentError("%s: scale must be a contiguous float32 tensor of %d elements on %s (got %s %s "
                                   "shape %s)" % (name, slots, dev, scale.dtype, scale.device, tuple(scale.shape)))
    out = _out_rows(name, out, R, D, dtype or src.dtype, dev)
    dgate = None
    if h is not None:
        _check_rows(name, h, "h", D, dev)
        if h.shape[0] != R or h.dtype != out.dtype:
            raise InvalidArgumentError("%s: h must be %s [%d, %d] like out, got %s %s"
                                       % (name, out.dtype, R, D, h.dtype, tuple(h.shape)))
        dgate = torch.empty(slots, dtype=torch.float32, device=dev)
    if R:
        _lib.call("ttdk_moe_gather", src.data_ptr(), src.stride(0), _DT[src.dtype], idx.data_ptr(), _lib.ptr(scale),
                  out.data_ptr(), out.stride(0), _DT[out.dtype], _lib.ptr(h), h.stride(0) if h is not None else 0,
                  _lib.ptr(dgate), R, n_src, k, D, _lib.stream())
    return out if h is None else (out, dgate)


def combine_rows(src, inv, k, *, w=None, dtype=None, out=None):
    """out[t] = sum_j w[t, j] * src[inv[t * k + j]] for the int32 inv [T * k] (w fp32 [T, k] or
    None: 1), accumulated in fp32 in increasing j; an inv entry outside src's rows adds nothing. src
    and out are rows of float32 or bfloat16 (dtype: of a new out, default float32)."""
    name = "combine_rows"
    _check_rows(name, src, "src")
    dev, (n_src, D), k = src.device, src.shape, int(k)
    if inv.dtype != torch.int32 or inv.device != dev or inv.dim() != 1 or not inv.is_contiguous():
        raise InvalidArgumentError("%s: inv must be a contiguous 1-D int32 tensor on %s (got %s %s shape %s)"
                                   % (name, dev, inv.dtype, inv.device, tuple(inv.shape)))
    if k < 1 or k > 256 or inv.shape[0] % k or inv.shape[0] >= 2 ** 30 or n_src >= 2 ** 30:
        raise InvalidArgumentError("%s: need 1 <= k <= 256 dividing the %d entries of inv (fewer than 2^30), got k = %d"
                                   % (name, inv.shape[0], k))
    T = inv.shape[0] // k
    if w is not None:
        _check_dense(name, w, "w", torch.float32, (T, k), dev)
    out = _out_rows(name, out, T, D, dtype or torch.float32, dev)
    if T:
        _lib.call("ttdk_moe_combine", src.data_ptr(), src.stride(0), _DT[src.dtype], inv.data_ptr(), _lib.ptr(w),
                  out.data_ptr(), out.stride(0), _DT[out.dtype], T, n_src, k, D, _lib.stream())
    return out
