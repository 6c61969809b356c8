"""Launch wrappers for the transformer kernels (attention.hip, transformer.hip, rope.hip,
rmsnorm_glu.hip) plus exact
CPU re-implementations of their dropout hash (used by the numerics tests as oracles).

All device tensors are bf16 token-major [tokens, features] unless noted; statistics fp32.
"""
from __future__ import annotations

import numpy as np
import torch

from ..utils.errors import InvalidArgumentError
from . import _lib


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return _lib.stream()


class RngState:
    """Device-resident dropout RNG state [seed, step]. Kernels read it from HBM, so a
    hipGraph-captured step draws new masks after `advance()` (itself a captured kernel)."""

    def __init__(self, seed: int, device):
        self.t = torch.tensor([int(seed), 0], dtype=torch.int64, device=device)

    def advance(self):
        if self.t.is_cuda:
            _lib.call("ttdk_rng_advance", self.t.data_ptr(), _s())
        else:
            self.t[1:2].add_(1)

    def host(self):
        v = self.t.cpu().tolist()
        return int(v[0]), int(v[1])


# ------------------------------------------------------------------ attention
def _band_window(window):
    """(left, right) of a window argument as the kernel takes it: -1 for an unbounded side."""
    if window is None:
        return -1, -1
    try:
        left, right = window
    except (TypeError, ValueError):
        raise InvalidArgumentError("attention band: window must be None or (left, right), got %r" % (window,))
    out = []
    for side in (left, right):
        if side is None:
            out.append(-1)
            continue
        if int(side) != side or side < 0:
            raise InvalidArgumentError(
                "attention band: a window bound is a non-negative token count or None for no bound, got %r"
                % (window,))
        out.append(min(int(side), 1 << 30))
    return out[0], out[1]


def attention_band_ints(B, S):
    """int32 elements of the band table of B rows of S tokens: a 16-byte record per token and one per
    128-token block."""
    return 4 * B * (S + S // 128)


def _band_check(segment_ids, seqlen, B, S):
    if S <= 0 or S % 128:
        raise InvalidArgumentError("attention band: S must be a positive multiple of 128, got %d" % S)
    if segment_ids is not None and (tuple(segment_ids.shape) != (B, S) or segment_ids.dtype not in
                                    (torch.int32, np.dtype("int32"))):
        raise InvalidArgumentError("attention band: segment_ids must be int32 [B, S] = [%d, %d], got %s %s"
                                   % (B, S, segment_ids.dtype, tuple(segment_ids.shape)))
    if seqlen is not None and (tuple(seqlen.shape) != (B,) or seqlen.dtype not in (torch.int32, np.dtype("int32"))):
        raise InvalidArgumentError("attention band: seqlen must be int32 [B] = [%d], got %s %s"
                                   % (B, seqlen.dtype, tuple(seqlen.shape)))


def attention_band(segment_ids, seqlen, window, causal, B, S, out=None):
    """The band table of the BAND attention kernels (attention.hip, ttdk_attn_band), built on the
    device on the current stream: int32 [attention_band_ints(B, S)], into `out` when given (no
    allocation: a captured step builds it into a per-shape buffer).

    Every query row attends one contiguous key range, the intersection of
      segment_ids  int32 [B, S] or None: a token attends the tokens of its own maximal run of equal
                   ids (an id that reappears later in the row is another document); a negative id
                   is padding — the token attends nothing and nothing attends it: its output row
                   and its dq / dk / dv rows are exactly zero and its lse is -inf;
      window       (left, right) or None: q - left <= k <= q + right, None on a side = no bound;
      causal       clamps right to 0;
      seqlen       int32 [B] or None: keys >= seqlen[b] are masked, queries never.
    A row whose intersection is empty behaves like a padding row. Self-attention only.
    Layout (attention_band_host is the numpy mirror): per token (klo, khi, qlo, qhi) — the keys
    [klo, khi) query s attends and the queries [qlo, qhi) that attend key s, (S, 0) when empty —
    then per 128-token block (kt0, kt1, qt0, qt1): the 64-key tiles a query block streams and the
    64-query tiles a key block streams, qt0 and qt1 even; all zero when the block has nothing."""
    _band_check(segment_ids, seqlen, B, S)
    left, right = _band_window(window)
    dev = segment_ids.device if segment_ids is not None else (seqlen.device if seqlen is not None else None)
    n = attention_band_ints(B, S)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev if dev is not None else "cuda")
    elif out.dtype != torch.int32 or out.numel() < n or not out.is_contiguous():
        raise InvalidArgumentError("attention band: out must be a contiguous int32 tensor of >= %d elements" % n)
    if segment_ids is not None and not segment_ids.is_contiguous():
        segment_ids = segment_ids.contiguous()
    _lib.call("ttdk_attn_band", _p(segment_ids), _p(seqlen), B, S, left, right, int(bool(causal)), out.data_ptr(),
              _s())
    return out


def attention_band_host(segment_ids, seqlen, window, causal, B, S) -> np.ndarray:
    """numpy mirror of attention_band: the same int32 table (see there for semantics and layout)."""
    ids = None if segment_ids is None else np.asarray(segment_ids)
    sl = None if seqlen is None else np.asarray(seqlen)
    _band_check(ids, sl, B, S)
    left, right = _band_window(window)
    if causal:
        right = 0
    tok = np.zeros((B, S, 4), dtype=np.int64)
    s = np.arange(S)
    for b in range(B):
        starts = s == 0
        if ids is not None:
            starts[1:] = ids[b, 1:] != ids[b, :-1]
        rs = np.maximum.accumulate(np.where(starts, s, 0))
        nxt = np.where(starts, s, S)  # the next run's first token, strictly after s
        re = np.append(np.minimum.accumulate(nxt[::-1])[::-1][1:], S)
        n = S if sl is None else min(max(int(sl[b]), 0), S)
        pad = np.zeros(S, dtype=bool) if ids is None else ids[b] < 0
        klo, khi, qlo, qhi = rs.copy(), np.minimum(re, n), rs.copy(), re.copy()
        if left >= 0:
            klo, qhi = np.maximum(klo, s - left), np.minimum(qhi, s + left + 1)
        if right >= 0:
            khi, qlo = np.minimum(khi, s + right + 1), np.maximum(qlo, s - right)
        ek = pad | (klo >= khi)
        eq = pad | (s >= n) | (qlo >= qhi)
        tok[b, :, 0], tok[b, :, 1] = np.where(ek, S, klo), np.where(ek, 0, khi)
        tok[b, :, 2], tok[b, :, 3] = np.where(eq, S, qlo), np.where(eq, 0, qhi)
    t = tok.reshape(B, S // 128, 128, 4)
    lo_k, hi_k, lo_q, hi_q = t[..., 0].min(-1), t[..., 1].max(-1), t[..., 2].min(-1), t[..., 3].max(-1)
    blk = np.zeros((B, S // 128, 4), dtype=np.int64)
    blk[..., 0] = np.where(hi_k > 0, lo_k // 64, 0)
    blk[..., 1] = (hi_k + 63) // 64
    blk[..., 2] = np.where(hi_q > 0, (lo_q // 64) & ~1, 0)
    blk[..., 3] = (hi_q + 127) // 128 * 2
    return np.concatenate([tok.reshape(-1), blk.reshape(-1)]).astype(np.int32)


def _band_arg(band, B, S, Sk, causal, seqlen):
    if Sk is not None and int(Sk) != S:
        raise InvalidArgumentError(
            "attention band: the band kernels are self-attention kernels (got %d queries, %d keys)" % (S, Sk))
    if band.dtype != torch.int32 or band.numel() < attention_band_ints(B, S) or not band.is_contiguous():
        raise InvalidArgumentError("attention band: band must be the int32 table of attention_band(..., B=%d, S=%d)"
                                   % (B, S))
    if causal or seqlen is not None:
        raise InvalidArgumentError("attention band: causal and seqlen are folded into the table by attention_band; "
                                   "pass them there, not beside band=")


def attention_fwd(q, k, v, out, lse, B, H, S, *, Sk=None, Hk=None, seqlen=None, p_drop=0.0, rng=None, site=0,
                  causal=False, band=None):
    """q/out: 2-D bf16 views [B*S, >= H*64], k/v: [B*Sk, >= Hk*64] (row stride = .stride(0), each its
    own); lse fp32 [B*H, S]. Sk (None: S) is the key length — cross-attention over a memory of
    another length; seqlen then holds the memory's valid lengths (keys >= seqlen[b] masked).
    causal: query s attends keys <= s only (combined with seqlen); the key tiles above the diagonal
    are not streamed. causal needs Sk == S.
    Hk (None: H) is the number of key/value heads — grouped-query attention (Hk == 1: multi-query):
    H % Hk == 0 and query head h reads key/value head h // (H // Hk), the layout of
    repeat_interleave over the head axis.
    band (a table of attention_band) runs the BAND kernels: each query row attends the key range the
    table gives it (documents, windows, causal and seqlen, all folded into the table — so seqlen
    and causal are not passed beside it), and key tiles outside a block's range are not streamed.
    Self-attention only: a band with Sk != S raises."""
    if band is not None:
        _band_arg(band, B, S, Sk, causal, seqlen)
        _lib.call("ttdk_attn_band_fwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                  v.stride(0), out.data_ptr(), out.stride(0), lse.data_ptr(), band.data_ptr(), B, H,
                  int(H if Hk is None else Hk), S, S, float(p_drop), _p(rng.t if rng is not None else None),
                  int(site), _s())
        return out, lse
    _lib.call("ttdk_attn_fwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
              out.data_ptr(), out.stride(0), lse.data_ptr(), _p(seqlen), B, H, int(H if Hk is None else Hk), S,
              int(S if Sk is None else Sk), float(p_drop), _p(rng.t if rng is not None else None), int(site),
              int(bool(causal)), _s())
    return out, lse


def set_fused_attention_bwd(on: bool):
    """Select the single-kernel attention backward (S in {128, 256, 512}; opt-in, measured slower
    at BERT-Large: attention.hip) or the split dQ / dK-dV kernels (default;
    TTD_ATTN_FUSED_BWD=1 at start-up selects the fused one). A causal backward ignores the switch:
    the fused kernel has no causal form, so attention_bwd(..., causal=True) always runs the split
    kernels; so does a cross-attention backward (Sk != S) and a grouped-query one (Hk != H)."""
    _lib.call("ttdk_attn_set_fused_bwd", int(bool(on)))


def attention_bwd(q, k, v, o, dout, lse, dq, dk, dv, B, H, S, *, Sk=None, Hk=None, delta=None, seqlen=None,
                  p_drop=0.0, rng=None, site=0, causal=False, band=None):
    """Backward of attention_fwd with the same Sk / Hk / seqlen / p_drop / rng / site / causal / band.
    dq has the query's B*S rows, dk / dv the keys' B*Sk; delta fp32 [B*H, S]. Sk != S always runs the
    split kernels (the fused backward is a self-attention kernel), and so does Hk != H: dk / dv then
    have Hk*64 columns, each key/value head the sum over its H // Hk query heads — summed in fp32
    registers in head order (deterministic), rounded to bf16 once. A band backward always runs the
    split kernels too (the fused backward has no band form)."""
    if delta is None:
        delta = torch.empty((B * H, S), dtype=torch.float32, device=q.device)
    if band is not None:
        _band_arg(band, B, S, Sk, causal, seqlen)
        _lib.call("ttdk_attn_band_bwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                  v.stride(0), o.data_ptr(), o.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(),
                  delta.data_ptr(), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(),
                  dv.stride(0), band.data_ptr(), B, H, int(H if Hk is None else Hk), S, S, float(p_drop),
                  _p(rng.t if rng is not None else None), int(site), _s())
        return dq, dk, dv
    _lib.call("ttdk_attn_bwd", q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
              o.data_ptr(), o.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(), delta.data_ptr(),
              dq.data_ptr(), dq.stride(0), dk.data_ptr(), dk.stride(0), dv.data_ptr(), dv.stride(0), _p(seqlen),
              B, H, int(H if Hk is None else Hk), S, int(S if Sk is None else Sk), float(p_drop),
              _p(rng.t if rng is not None else None), int(site), int(bool(causal)), _s())
    return dq, dk, dv


# ------------------------------------------------------------------ rotary position embeddings
_ROPE_DT = {torch.float32: 0, torch.bfloat16: 1}
_rope_tables = {}  # (device, base, rows) -> table; never evicted (a captured hipGraph may hold the pointer)


def rope_table(rows, base=10000.0, device="cuda"):
    """fp32 [rows, 2, 32] table of the rotary embedding (rope.hip): [p, 0, i] = cos(p * base**(-i/32)),
    [p, 1, i] the sine, computed on the host in float64 and rounded once to fp32. Cached per
    (device, base, rows) and never evicted, because a captured hipGraph may hold the pointer; a
    cache miss while the current stream is capturing raises instead of copying inside the capture
    (build the table before the capture). A CPU device gives the same table."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (str(dev), float(base), int(rows))
    t = _rope_tables.get(key)
    if t is None:
        if rows <= 0 or not base > 0:
            raise ValueError("rope_table needs rows > 0 and base > 0 (got rows %r, base %r)" % (rows, base))
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "rope_table(%d, base=%r) is not cached and the current stream is capturing a graph: the table's "
                "host-to-device copy cannot run inside a capture; build the table before the capture" % (rows, base))
        ang = np.arange(int(rows), dtype=np.float64)[:, None] * float(base) ** (-np.arange(32, dtype=np.float64) / 32.0)
        t = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)).to(dev)
        _rope_tables[key] = t
    return t


def rope(x, y, table, S, heads, *, pos0=0, inverse=False):
    """y[r, :heads*64] = the half-split rotation of x[r, :heads*64] at position pos0 + r % S
    (inverse=True: the inverse rotation, which is also the backward). x, y: 2-D views [tokens,
    >= heads*64] of one dtype (bf16 or fp32) with unit column stride, each with its own row stride;
    columns from heads*64 on are not touched. y may be x (in place, e.g. x = qkv with heads =
    H + Hk rotates q and k of the fused projection in one launch); any other overlap of x and y is
    the caller's error. table: rope_table(rows >= pos0 + S) on x's device."""
    if x.dtype != y.dtype or x.dtype not in _ROPE_DT or x.dim() != 2 or y.shape[0] != x.shape[0] \
            or x.stride(1) != 1 or y.stride(1) != 1 or table.dtype != torch.float32 or not table.is_contiguous():
        raise _lib.HipKernelError("rope: x and y must be 2-D bf16 or fp32 views of one dtype and row count with unit "
                                  "column stride, table contiguous fp32")
    _lib.call("ttdk_rope", x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), _ROPE_DT[x.dtype],
              table.data_ptr(), table.shape[0], x.shape[0], int(S), int(heads), int(pos0), int(bool(inverse)), _s())
    return y


def rope_max_threads():
    """Threads the capped rope grid launches; more work items than this are grid-strided."""
    return _lib.query("ttdk_rope_max_threads")


# ------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, *, res=None, eps=1e-12, p_in=0.0, site_in=0, p_out=0.0, site_out=0, rng=None,
                  save_s=True, out=None, s_out=None, mean=None, rstd=None):
    rows, H = x.shape
    dev = x.device
    out = out if out is not None else torch.empty_like(x)
    need_s = save_s and (res is not None or p_in > 0)
    s_out = s_out if s_out is not None else (torch.empty_like(x) if need_s else None)
    mean = mean if mean is not None else torch.empty(rows, dtype=torch.float32, device=dev)
    rstd = rstd if rstd is not None else torch.empty(rows, dtype=torch.float32, device=dev)
    _lib.call("ttdk_ln_fwd", x.data_ptr(), _p(res), _p(s_out), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), rows, H, float(eps), float(p_in), int(site_in), float(p_out),
              int(site_out), _p(rng.t if rng is not None else None), _s())
    return out, (s_out if s_out is not None else x), mean, rstd


def ln_bwd_workspace(rows, H, device):
    nb = _lib.query("ttdk_ln_bwd_num_blocks", rows)
    return torch.empty((nb, 2, H), dtype=torch.float32, device=device)


def layernorm_bwd(dy, s, mean, rstd, gamma, dgamma, dbeta, *, ds_out=None, want_dx=False, accumulate=False,
                  p_in=0.0, site_in=0, p_out=0.0, site_out=0, rng=None, work=None, dx_out=None):
    rows, H = dy.shape
    ds_out = ds_out if ds_out is not None else torch.empty_like(dy)
    if want_dx and dx_out is None:
        dx_out = torch.empty_like(dy)
    work = work if work is not None else ln_bwd_workspace(rows, H, dy.device)
    _lib.call("ttdk_ln_bwd", dy.data_ptr(), s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
              ds_out.data_ptr(), _p(dx_out if want_dx else None), work.data_ptr(), dgamma.data_ptr(),
              dbeta.data_ptr(), int(accumulate), rows, H, float(p_in), int(site_in), float(p_out), int(site_out),
              _p(rng.t if rng is not None else None), _s())
    return ds_out, (dx_out if want_dx else None)


# ------------------------------------------------------------------ RMSNorm (rmsnorm_glu.hip, fast widths)
RMS_FAST_WIDTHS = (512, 1024, 1536, 2048, 4096)


def _rms_check(what, H, **tensors):
    """bf16 [rows, H] dense 16-byte-aligned activations (fp32 for names ending in '32')."""
    if H not in RMS_FAST_WIDTHS:
        raise InvalidArgumentError("%s: width %d is not one of %s" % (what, H, RMS_FAST_WIDTHS))
    for name, t in tensors.items():
        if t is None:
            continue
        want = torch.float32 if name.endswith("32") else torch.bfloat16
        if t.dtype != want or not t.is_contiguous() or t.data_ptr() % 16:
            raise InvalidArgumentError("%s: %s must be a contiguous 16-byte-aligned %s tensor (got %s, strides %s, "
                                       "address %% 16 = %d)" % (what, name.rstrip("32"), want, t.dtype, tuple(t.stride()),
                                                                t.data_ptr() % 16))
        if want == torch.bfloat16 and (t.dim() != 2 or t.shape[1] != H):
            raise InvalidArgumentError("%s: %s must be [rows, %d], got %s" % (what, name, H, tuple(t.shape)))


def rmsnorm_fwd(x, gamma, *, res=None, eps=1e-6, p_in=0.0, site_in=0, p_out=0.0, site_out=0, rng=None, save_s=True,
                out=None, s_out=None, rstd=None):
    """y = drop_out(s * rstd * gamma), s = res + drop_in(x) rounded to bf16, rstd = rsqrt(mean(s^2) + eps):
    the residual / dropout frame of layernorm_fwd with one statistic. x, res: bf16 [rows, H], H in
    RMS_FAST_WIDTHS; gamma fp32 [H]. Returns (y, s, rstd); s is x itself when there is neither a
    residual nor an input dropout."""
    if x.dim() != 2:
        raise InvalidArgumentError("rmsnorm_fwd: x must be [rows, H], got %s" % (tuple(x.shape),))
    rows, H = x.shape
    dev = x.device
    out = out if out is not None else torch.empty_like(x)
    need_s = save_s and (res is not None or p_in > 0)
    s_out = s_out if s_out is not None else (torch.empty_like(x) if need_s else None)
    rstd = rstd if rstd is not None else torch.empty(rows, dtype=torch.float32, device=dev)
    _rms_check("rmsnorm_fwd", H, x=x, res=res, out=out, s_out=s_out, gamma32=gamma)
    if gamma.numel() != H or rstd.dtype != torch.float32 or rstd.numel() != rows or not rstd.is_contiguous():
        raise InvalidArgumentError("rmsnorm_fwd: gamma must be fp32 [%d] and rstd fp32 [%d]" % (H, rows))
    if (p_in > 0 or p_out > 0) and rng is None:
        raise InvalidArgumentError("rmsnorm_fwd: dropout needs rng")
    _lib.call("ttdk_rms_fwd", x.data_ptr(), _p(res), _p(s_out), out.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
              rows, H, float(eps), float(p_in), int(site_in), float(p_out), int(site_out),
              _p(rng.t if rng is not None else None), _s())
    return out, (s_out if s_out is not None else x), rstd


def rmsnorm_bwd_workspace(rows, H, device):
    nb = _lib.query("ttdk_rms_bwd_num_blocks", rows)
    return torch.empty((nb, H), dtype=torch.float32, device=device)


def rmsnorm_bwd(dy, s, rstd, gamma, dgamma, *, ds_out=None, want_dx=False, accumulate=False, p_in=0.0, site_in=0,
                p_out=0.0, site_out=0, rng=None, work=None, dx_out=None):
    """Backward of rmsnorm_fwd with the same dropouts: ds = dL/ds (the residual branch), dx = ds through
    the input dropout (want_dx), dgamma fp32 [H] written or added to (accumulate). dgamma is summed
    in a fixed order (no atomics). work: rmsnorm_bwd_workspace(rows, H)."""
    if dy.dim() != 2:
        raise InvalidArgumentError("rmsnorm_bwd: dy must be [rows, H], got %s" % (tuple(dy.shape),))
    rows, H = dy.shape
    ds_out = ds_out if ds_out is not None else torch.empty_like(dy)
    if want_dx and dx_out is None:
        dx_out = torch.empty_like(dy)
    if H in RMS_FAST_WIDTHS:
        nb = _lib.query("ttdk_rms_bwd_num_blocks", rows)
        if work is None:
            work = torch.empty((nb, H), dtype=torch.float32, device=dy.device)
        elif work.dtype != torch.float32 or work.numel() < nb * H or not work.is_contiguous():
            raise InvalidArgumentError("rmsnorm_bwd: workspace must be contiguous fp32 with >= %d x %d elements "
                                       "(rmsnorm_bwd_workspace), got %s %s" % (nb, H, work.dtype, tuple(work.shape)))
    _rms_check("rmsnorm_bwd", H, dy=dy, s=s, ds_out=ds_out, dx_out=dx_out if want_dx else None, gamma32=gamma,
               dgamma32=dgamma, work32=work, rstd32=rstd)
    if gamma.numel() != H or dgamma.numel() != H or rstd.numel() != rows:
        raise InvalidArgumentError("rmsnorm_bwd: gamma / dgamma must be fp32 [%d] and rstd fp32 [%d]" % (H, rows))
    if (p_in > 0 or p_out > 0) and rng is None:
        raise InvalidArgumentError("rmsnorm_bwd: dropout needs rng")
    _lib.call("ttdk_rms_bwd", dy.data_ptr(), s.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), ds_out.data_ptr(),
              _p(dx_out if want_dx else None), work.data_ptr(), dgamma.data_ptr(), int(accumulate), rows, H,
              float(p_in), int(site_in), float(p_out), int(site_out), _p(rng.t if rng is not None else None), _s())
    return ds_out, (dx_out if want_dx else None)


# ------------------------------------------------------------------ SwiGLU (rmsnorm_glu.hip)
_GLU_DT = {torch.float32: 0, torch.bfloat16: 1}


def _glu_view(what, name, t, width):
    if t.dim() != 2 or t.shape[1] != width or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < width):
        raise InvalidArgumentError("%s: %s must be a 2-D [rows, %d] view with unit column stride and row stride >= "
                                   "its width, got shape %s strides %s" % (what, name, width, tuple(t.shape),
                                                                           tuple(t.stride())))


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def swiglu_fwd(x2, out=None):
    """h = silu(x2[:, :I]) * x2[:, I:] for x2 [rows, 2I] (gate columns first), bf16 or fp32. x2 and out
    are 2-D views with unit column stride, each with its own row stride (row-padded column views);
    16-byte accesses when I, the strides and the addresses allow, a scalar kernel otherwise."""
    if x2.dtype not in _GLU_DT:
        raise InvalidArgumentError("swiglu_fwd takes float32 / bfloat16, got %s" % x2.dtype)
    if x2.dim() != 2 or x2.shape[1] % 2 or x2.shape[1] == 0:
        raise InvalidArgumentError("swiglu_fwd: x2 must be [rows, 2I], got %s" % (tuple(x2.shape),))
    rows, I2 = x2.shape
    Iw = I2 // 2
    _glu_view("swiglu_fwd", "x2", x2, I2)
    if out is None:
        out = torch.empty((rows, Iw), dtype=x2.dtype, device=x2.device)
    if out.dtype != x2.dtype or out.shape[0] != rows:
        raise InvalidArgumentError("swiglu_fwd: out must be %s [%d, %d]" % (x2.dtype, rows, Iw))
    _glu_view("swiglu_fwd", "out", out, Iw)
    _lib.call("ttdk_swiglu_fwd", x2.data_ptr(), _ld(x2), out.data_ptr(), _ld(out), _GLU_DT[x2.dtype], rows, Iw, _s())
    return out


def swiglu_bwd(dh, x2, out=None):
    """dx2 = [da | db] of swiglu_fwd from dh [rows, I] and the forward's input x2 [rows, 2I]. out may be
    x2 itself (in place: every work item reads its gate / value pair before it writes)."""
    if x2.dtype not in _GLU_DT or dh.dtype != x2.dtype:
        raise InvalidArgumentError("swiglu_bwd takes float32 / bfloat16 tensors of one dtype, got %s and %s"
                                   % (dh.dtype, x2.dtype))
    if x2.dim() != 2 or x2.shape[1] % 2 or x2.shape[1] == 0:
        raise InvalidArgumentError("swiglu_bwd: x2 must be [rows, 2I], got %s" % (tuple(x2.shape),))
    rows, I2 = x2.shape
    Iw = I2 // 2
    _glu_view("swiglu_bwd", "x2", x2, I2)
    _glu_view("swiglu_bwd", "dh", dh, Iw)
    if dh.shape[0] != rows:
        raise InvalidArgumentError("swiglu_bwd: dh has %d rows, x2 %d" % (dh.shape[0], rows))
    if out is None:
        out = torch.empty((rows, I2), dtype=x2.dtype, device=x2.device)
    if out.dtype != x2.dtype or out.shape[0] != rows:
        raise InvalidArgumentError("swiglu_bwd: out must be %s [%d, %d]" % (x2.dtype, rows, I2))
    _glu_view("swiglu_bwd", "out", out, I2)
    _lib.call("ttdk_swiglu_bwd", dh.data_ptr(), _ld(dh), x2.data_ptr(), _ld(x2), out.data_ptr(), _ld(out),
              _GLU_DT[x2.dtype], rows, Iw, _s())
    return out


def swiglu_max_threads():
    """Threads the capped SwiGLU grid launches; more work items than this are grid-strided."""
    return _lib.query("ttdk_swiglu_max_threads")


# ------------------------------------------------------------------ embeddings / rows
def embed_fwd(ids, tt, word, pos, typ, S, out=None):
    rows = ids.numel()
    H = word.shape[1]
    out = out if out is not None else torch.empty((rows, H), dtype=torch.bfloat16, device=ids.device)
    _lib.call("ttdk_embed_fwd", ids.data_ptr(), _p(tt), word.data_ptr(), pos.data_ptr(), typ.data_ptr(),
              out.data_ptr(), rows, S, H, _s())
    return out


def embed_bwd(ds, ids, tt, dword, dpos, dtype, B, S, pos_beta=0):
    H = ds.shape[1]
    T = dtype.shape[0] if dtype is not None else 0
    _lib.call("ttdk_embed_bwd", ds.data_ptr(), ids.data_ptr(), _p(tt), dword.data_ptr(), dpos.data_ptr(),
              _p(dtype), B, S, H, T, int(pos_beta), _s())


def gather_rows(src, idx, out=None, *, group=(1, 0), n=None):
    """out[r] = src[(idx[r] if idx is not None else 0) + (r // per) * gs], group = (per, gs): e.g.
    per-sequence positions [B, P] of a [B*S, H] activation with group = (P, S); idx None and
    group (1, S) picks every sequence's first row. idx: contiguous int32."""
    per, gs = group
    n = idx.numel() if idx is not None else n
    H = src.shape[1]
    out = out if out is not None else torch.empty((n, H), dtype=src.dtype, device=src.device)
    _lib.call("ttdk_gather_rows", src.data_ptr(), src.stride(0), _p(idx), int(per), int(gs), out.data_ptr(), n, H,
              _s())
    return out


def scatter_rows(src, idx, dst, accumulate=False, *, group=(1, 0)):
    """dst[(idx[r] or 0) + (r // per) * gs] (+)= src[r] (the inverse of gather_rows)."""
    n, H = src.shape
    per, gs = group
    _lib.call("ttdk_scatter_rows", src.data_ptr(), _p(idx), int(per), int(gs), dst.data_ptr(), dst.stride(0), n, H,
              int(accumulate), _s())
    return dst


def count_valid(labels, scale, out):
    _lib.call("ttdk_count_valid", labels.data_ptr(), labels.numel(), float(scale), out.data_ptr(), _s())
    return out


def count_valid2(labels, scale, out):
    """out[0] = 1 / count, out[1] = scale / count (count = labels >= 0), one launch."""
    _lib.call("ttdk_count_valid2", labels.data_ptr(), labels.numel(), float(scale), out.data_ptr(), _s())
    return out


def xent_vocab(logits, V, labels, gscale, *, dlogits=None, sums=None, mscale=None):
    rows = logits.shape[0]
    _lib.call("ttdk_xent_vocab", logits.data_ptr(), logits.stride(0), int(V), labels.data_ptr(), rows,
              gscale.data_ptr(), _p(dlogits), _p(sums), _p(mscale), _s())
    return dlogits


def dact(dy, aux, kind, out=None):
    """dy * act'(aux): kind 0 = tanh-GELU (aux = pre-activation), 1 = tanh (aux = tanh output)."""
    out = out if out is not None else torch.empty_like(dy)
    _lib.call("ttdk_dact_bf16", dy.data_ptr(), aux.data_ptr(), out.data_ptr(), dy.numel(), int(kind), _s())
    return out


def tanh_(x):
    _lib.call("ttdk_tanh_bf16", x.data_ptr(), x.numel(), _s())
    return x


# ------------------------------------------------------------------ CPU mirror of the dropout hash
M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def _attn_mix(h):
    """tile_common.h attn_mix: xorshift, 24 x 24-bit multiply-add of the high byte
    (v_mad_u32_u24), xorshift."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = ((h & np.uint64(0xFFFFFF)) * np.uint64(0x9E3779) + (h >> np.uint64(24))) & M32
    h ^= h >> np.uint64(16)
    return h


def drop_key(seed: int, step: int, site: int) -> int:
    seed &= (1 << 64) - 1
    step &= (1 << 64) - 1
    k = _fmix32(np.uint64((seed & 0xFFFFFFFF) ^ 0x243F6A88))
    k = _fmix32(k ^ np.uint64(seed >> 32) ^ np.uint64((site * 0x9E3779B9) & 0xFFFFFFFF))
    k = _fmix32(k ^ (np.uint64(((step & 0xFFFFFFFF) * 0x85EBCA77) & 0xFFFFFFFF) ^ np.uint64(step >> 32)))
    return int(k)


def drop_threshold(p: float) -> int:
    if p <= 0:
        return 0
    if p >= 1:
        return 0xFFFFFFFF
    # the kernel computes (uint32)(double(float(p)) * 2^32)
    return int(float(np.float32(p)) * 4294967296.0)


def keep_mask(seed: int, step: int, site: int, p: float, idx) -> np.ndarray:
    """Boolean keep mask for flat element indices `idx` (int64 array)."""
    key = np.uint64(drop_key(seed, step, site))
    idx = np.asarray(idx, dtype=np.uint64)
    lo = idx & M32
    hi = idx >> np.uint64(32)
    mixed = ((lo * np.uint64(0x9E3779B1)) + (hi * np.uint64(0x7FEB352D))) & M32
    h = _fmix32(key ^ mixed)
    return h >= np.uint64(drop_threshold(p))


def attention_keep_mask(seed: int, step: int, site: int, p: float, B: int, H: int, S: int, Sk=None) -> np.ndarray:
    """Keep mask [B, H, S(query), Sk(key)] (Sk None: S) of the attention-probability dropout (mirror
    of tile_common.h attn_pair_hash / attn_keep_half: keys k and k + 16 of an aligned 32-key block
    share one hash, pair ((k >> 5) << 4) | (k & 15), 16-bit half (k >> 4) & 1). The row id is
    (b*H + h)*S + query and the pair term depends on the key alone, so a longer memory extends the
    mask of a shorter one. The mask is per QUERY head: with grouped-query attention (Hk < H
    key/value heads) H is still the number of query heads, and the heads of a group draw
    independent masks over their shared keys."""
    Sk = S if Sk is None else int(Sk)
    key = np.uint64(drop_key(seed, step, site))
    thr = 0 if p <= 0 else (0x10000 if p >= 1 else int(float(np.float32(p)) * 65536.0))
    rowid = np.arange(B * H * S, dtype=np.uint64).reshape(B * H, S, 1)
    k = np.arange(Sk, dtype=np.uint64).reshape(1, 1, Sk)
    pair = ((k >> np.uint64(5)) << np.uint64(4)) | (k & np.uint64(15))
    mixed = ((rowid * np.uint64(0x9E3779B1)) + (pair * np.uint64(0x7FEB352D))) & M32
    h = _attn_mix(key ^ mixed)
    half = np.where(((k >> np.uint64(4)) & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return (half >= np.uint64(thr)).reshape(B, H, S, Sk)


def attention_drop_scale(p: float) -> float:
    """The kernels' 1/keep-probability for the realised 16-bit threshold."""
    if p <= 0:
        return 1.0
    thr = int(float(np.float32(p)) * 65536.0)
    return 65536.0 / (65536.0 - thr)
