"""`ttd.nn` — functional ops with autograd (tf.nn-shaped), SURVEY.md §2.2 T22-T25/T30 and
§7.5 ("mitrain.nn.*").

Every op runs a hand-written gfx950 kernel when its inputs live on the GPU (a
torch.autograd.Function whose backward is also a HIP kernel) and a plain fp32 PyTorch
implementation on CPU tensors (the "soft placement" CPU fallback of
ConfigProto(allow_soft_placement=True), reference distribute_training.py:201-202). There is no
silent GPU fallback to torch compute: a GPU input the kernels cannot take (dtype other than
fp32/bf16, an unsupported attention head size) raises InvalidArgumentError.

GPU precision: fp32 inputs stay fp32 for dense/matmul (exact-fp32 MFMA, gemm_f32.hip),
normalisation, pooling, depthwise convolution, embeddings, activations and losses (nn_generic.hip /
depthwise.hip / elementwise.hip / xent.hip); bf16 inputs use the bf16 MFMA engines. conv2d and attention compute in bf16 (fp32
accumulation) for either input dtype.

    ttd.nn.elu(x); ttd.nn.dropout(x, rate=0.01)
    ttd.nn.sparse_softmax_cross_entropy_with_logits(labels=y, logits=z)
    ttd.nn.in_top_k(z, y, 1); ttd.nn.layer_norm(x, gamma, beta)
    ttd.nn.dense(x, kernel, bias, activation="relu")      # kernel [in, out] (TF layout)
    ttd.nn.conv2d(x, kernel, strides, padding)            # NHWC, kernel [R, S, C, K]
    ttd.nn.depthwise_conv2d(x, kernel, strides, padding, dilations)   # kernel [R, S, C, M], R, S <= 7
    ttd.nn.separable_conv2d(x, depthwise_kernel, pointwise_kernel)    # depthwise, then the 1x1 GEMM
    ttd.nn.attention(q, k, v, num_heads, dropout_rate)    # [B, S, H*64] token-major
    ttd.nn.attention(q, k, v, 16, num_kv_heads=4)         # grouped-query: k, v [B, Sk, 4*64]
    ttd.nn.rotary_embedding(q, 16, offset=0)              # RoPE on q / k before attention
    ttd.nn.rms_norm(x, gamma); ttd.nn.swiglu(x)           # RMSNorm; silu(x[..., :I]) * x[..., I:]
    ttd.nn.group_norm(x, gamma, beta, groups=32)          # [N, *spatial, C], per-sample group statistics
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .utils.errors import InvalidArgumentError

_ACT_CODES = {None: 0, "linear": 0, "relu": 1, "gelu": 2, "tanh": 3}  # GEMM epilogue codes
_EW_ACT = {None: 0, "linear": 0, "relu": 1, "gelu": 2, "elu": 3}       # elementwise kernel codes


def _on_gpu(*ts):
    if not (all(t is None or t.is_cuda for t in ts) and any(t is not None for t in ts)):
        return False
    for t in ts:
        if t is not None and t.is_floating_point() and t.dtype not in (torch.float32, torch.bfloat16):
            raise InvalidArgumentError("ttd.nn GPU kernels take float32/bfloat16 tensors, got %s" % t.dtype)
    return True


def _f32(t):
    """fp32 contiguous view/copy of a (small) parameter vector, or None."""
    return None if t is None else t.float().contiguous()


class _Rng:
    """Host-side Philox (seed, offset) stream for eager-mode dropout."""
    seed = 0x5EED
    offset = 0

    @classmethod
    def next(cls, n):
        off = cls.offset
        cls.offset += (n + 3) // 4 + 1
        return cls.seed, off


def set_random_seed(seed: int):
    _Rng.seed = int(seed)
    _Rng.offset = 0
    torch.manual_seed(seed)


# ------------------------------------------------------------------ activations
def _act_ref(x, act):
    if act in (None, "linear"):
        return x
    if act == "relu":
        return F.relu(x)
    if act == "elu":
        return F.elu(x)
    if act == "gelu":
        return F.gelu(x, approximate="tanh")
    if act == "tanh":
        return torch.tanh(x)
    raise ValueError("unknown activation %r" % act)


class _BiasActDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, act, rate):
        from .ops import kernels as K
        xb = x.contiguous()
        seed, off = _Rng.next(xb.numel()) if rate > 0 else (0, 0)
        code = _EW_ACT[act]
        b = bias.float().contiguous() if bias is not None else None
        y = K.bias_act_dropout(xb, b, act=code, rate=rate, seed=seed, offset=off)
        ctx.save_for_backward(xb, b)
        ctx.cfg = (code, rate, seed, off, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        xb, b = ctx.saved_tensors
        code, rate, seed, off, has_b = ctx.cfg
        dz = K.bias_act_dropout_bwd(dy.contiguous().to(xb.dtype), xb, b, act=code, rate=rate, seed=seed, offset=off)
        db = None
        if has_b:
            db = K.colsum(dz.reshape(-1, dz.shape[-1]))
        return dz, db, None, None


def _bias_act_dropout(x, bias, act, rate):
    if _on_gpu(x) and x.dtype in (torch.float32, torch.bfloat16) and (act in _EW_ACT):
        return _BiasActDropout.apply(x, bias, act, float(rate))
    y = x + bias if bias is not None else x
    y = _act_ref(y, act)
    if rate > 0:
        y = F.dropout(y, rate, training=True)
    return y


def elu(x):
    return _bias_act_dropout(x, None, "elu", 0.0)


def relu(x):
    return _bias_act_dropout(x, None, "relu", 0.0)


def gelu(x):
    return _bias_act_dropout(x, None, "gelu", 0.0)


class _Unary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, op):
        from .ops import kernels as K
        y = K.unary(x.contiguous(), op)
        ctx.save_for_backward(y)
        ctx.op = op
        return y

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        (y,) = ctx.saved_tensors
        return K.unary_bwd(dy.contiguous().to(y.dtype), y, ctx.op), None


def tanh(x):
    if _on_gpu(x):
        return _Unary.apply(x, 0)
    return torch.tanh(x)


def sigmoid(x):
    if _on_gpu(x):
        return _Unary.apply(x, 1)
    return torch.sigmoid(x)


def bias_add(x, bias):
    return _bias_act_dropout(x, bias, None, 0.0)


def dropout(x, rate: float = 0.5, training: bool = True):
    """tf.nn.dropout / tf.layers.dropout: keep with probability 1-rate, scale by 1/(1-rate)."""
    if not training or rate <= 0:
        return x
    return _bias_act_dropout(x, None, None, rate)


# ------------------------------------------------------------------ dense (GEMM + epilogue)
class _Dense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, bias, act):
        from .ops import gemm as G
        shp = x.shape
        xb = x.reshape(-1, shp[-1]).to(torch.bfloat16).contiguous()
        wb = kernel.to(torch.bfloat16).contiguous()          # [in, out]
        b = bias.float().contiguous() if bias is not None else None
        code = _ACT_CODES.get(act, None)
        pre = None
        if act in ("gelu", "tanh", "relu"):
            pre = torch.empty((xb.shape[0], wb.shape[1]), dtype=torch.bfloat16, device=x.device)
        y = G.gemm(xb, wb, bias=b, act=code or 0, aux=pre)
        if act == "elu":
            from .ops import kernels as K
            pre = y
            y = K.bias_act_dropout(y, None, act=_EW_ACT["elu"])
        ctx.save_for_backward(xb, wb, pre, y if act == "tanh" else None)
        ctx.cfg = (act, bias is not None, shp, x.dtype, kernel.dtype)
        return y.reshape(*shp[:-1], wb.shape[1]).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        from .ops import gemm as G
        from .ops import kernels as K
        from .ops import transformer as T
        xb, wb, pre, y = ctx.saved_tensors
        act, has_b, shp, xdt, wdt = ctx.cfg
        d = dy.reshape(-1, wb.shape[1]).to(torch.bfloat16).contiguous()
        if act == "gelu":
            d = T.dact(d, pre, 0)
        elif act == "tanh":
            d = T.dact(d, y, 1)
        elif act in ("relu", "elu"):
            d = K.bias_act_dropout_bwd(d, pre, None, act=_EW_ACT[act])
        dw = torch.empty(wb.shape, dtype=torch.float32, device=d.device)
        G.gemm(xb, d, trans_a=True, out=dw, splits=G.gemm_wgrad_splits(wb.shape[0], wb.shape[1], xb.shape[0]))
        db = K.colsum(d) if has_b else None
        dx = G.gemm(d, wb, trans_b=True) if ctx.needs_input_grad[0] else None
        return (dx.reshape(shp).to(xdt) if dx is not None else None), dw.to(wdt), db, None


class _DenseF32(torch.autograd.Function):
    """Exact-fp32 dense layer: f32-MFMA GEMMs (gemm_f32.hip) + fp32 element-wise kernels."""

    @staticmethod
    def forward(ctx, x, kernel, bias, act):
        from .ops import gemm as G
        from .ops import kernels as K
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        w = kernel.contiguous()
        y = G.gemm_f32(x2, w, bias=_f32(bias))
        pre = None
        if act in ("relu", "gelu", "elu"):
            pre = y
            y = K.bias_act_dropout(y, None, act=_EW_ACT[act])
        elif act == "tanh":
            y = K.unary(y, K.UNARY_TANH)
        elif act not in (None, "linear"):
            raise InvalidArgumentError("unknown dense activation %r" % (act,))
        ctx.save_for_backward(x2, w, pre, y if act == "tanh" else None)
        ctx.cfg = (act, bias is not None, shp)
        return y.reshape(*shp[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, dy):
        from .ops import gemm as G
        from .ops import kernels as K
        x2, w, pre, y = ctx.saved_tensors
        act, has_b, shp = ctx.cfg
        d = dy.reshape(-1, w.shape[1]).contiguous()
        if act in ("relu", "gelu", "elu"):
            d = K.bias_act_dropout_bwd(d, pre, None, act=_EW_ACT[act])
        elif act == "tanh":
            d = K.unary_bwd(d, y, K.UNARY_TANH)
        dw = G.gemm_f32(x2, d, trans_a=True) if ctx.needs_input_grad[1] else None
        db = K.colsum(d) if has_b and ctx.needs_input_grad[2] else None
        dx = G.gemm_f32(d, w, trans_b=True).reshape(shp) if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


def dense(x, kernel, bias=None, activation=None):
    """y = activation(x @ kernel + bias); kernel [in, out] (tf.layers.dense layout)."""
    if _on_gpu(x, kernel):
        if x.dtype == torch.float32 and kernel.dtype == torch.float32:
            return _DenseF32.apply(x, kernel, bias, activation)
        return _Dense.apply(x, kernel, bias, activation)
    y = x @ kernel
    if bias is not None:
        y = y + bias
    return _act_ref(y, activation)


class _MatMul(torch.autograd.Function):
    """[..., M, K] @ [..., K, N] with identical leading (batch) shapes: ONE strided-batched GEMM
    launch per product (ops.gemm.gemm_batched: batch index on the grid), forward and backward.
    fp32 operands stay exact fp32 (f32 MFMA); otherwise bf16 operands with fp32 accumulation."""

    @staticmethod
    def _bmm(a, b, ta=False, tb=False):
        from .ops import gemm as G
        if a.dtype == torch.float32 and b.dtype == torch.float32:
            return G.gemm_batched(a, b, trans_a=ta, trans_b=tb)
        return G.gemm_batched(a.to(torch.bfloat16), b.to(torch.bfloat16), trans_a=ta, trans_b=tb,
                              out_dtype=torch.float32)

    @staticmethod
    def forward(ctx, a, b):
        a3 = a.reshape(-1, a.shape[-2], a.shape[-1]).contiguous()
        b3 = b.reshape(-1, b.shape[-2], b.shape[-1]).contiguous()
        out = _MatMul._bmm(a3, b3)
        ctx.save_for_backward(a3, b3)
        ctx.shapes = (a.shape, b.shape, a.dtype, b.dtype)
        return out.reshape(*a.shape[:-1], b.shape[-1]).to(a.dtype)

    @staticmethod
    def backward(ctx, dy):
        a3, b3 = ctx.saved_tensors
        sa, sb, da_t, db_t = ctx.shapes
        d3 = dy.reshape(a3.shape[0], a3.shape[1], b3.shape[2]).contiguous()
        if d3.dtype != a3.dtype and a3.dtype == torch.float32:
            d3 = d3.float()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = _MatMul._bmm(d3, b3, tb=True).reshape(sa).to(da_t)
        if ctx.needs_input_grad[1]:
            db = _MatMul._bmm(a3, d3, ta=True).reshape(sb).to(db_t)
        return da, db


def matmul(a, b, transpose_a=False, transpose_b=False):
    a2 = a.transpose(-1, -2) if transpose_a else a
    b2 = b.transpose(-1, -2) if transpose_b else b
    if _on_gpu(a, b):
        if a2.dim() == 2 and b2.dim() == 2:
            return dense(a2.contiguous(), b2.contiguous())
        if a2.shape[:-2] != b2.shape[:-2]:
            raise InvalidArgumentError("ttd.nn.matmul on GPU needs equal batch shapes, got %s and %s"
                                       % (tuple(a2.shape), tuple(b2.shape)))
        return _MatMul.apply(a2, b2)
    return a2 @ b2


# ------------------------------------------------------------------ losses / metrics
class _SparseXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        from .ops import kernels as K
        z = logits.contiguous()
        if z.dtype not in (torch.float32, torch.bfloat16):
            z = z.float()
        _, dl, rows, _ = K.sparse_xent(z, labels.contiguous(), grad_scale=1.0, want_rows=True)
        ctx.save_for_backward(dl)
        ctx.dt = logits.dtype
        return rows

    @staticmethod
    def backward(ctx, g):
        from .ops import kernels as K
        (dl,) = ctx.saved_tensors
        d = K.row_scale(dl, g.float().contiguous())
        return (d if d.dtype == ctx.dt else d.to(ctx.dt)), None


def sparse_softmax_cross_entropy_with_logits(labels=None, logits=None):
    """Per-example loss [N] (tf.nn.sparse_softmax_cross_entropy_with_logits)."""
    if _on_gpu(logits) and logits.dim() == 2:
        return _SparseXent.apply(logits, labels)
    return F.cross_entropy(logits.float(), labels.long(), reduction="none")


def in_top_k(predictions, targets, k: int = 1):
    """TF semantics: correct iff fewer than k classes have a STRICTLY greater logit than the
    target's; a non-finite target logit is never correct."""
    if _on_gpu(predictions) and predictions.dim() == 2:
        from .ops import kernels as K
        t = targets if targets.dtype in (torch.int32, torch.int64) else targets.long()
        return K.in_top_k(predictions.contiguous(), t.contiguous(), int(k)).bool()
    z = predictions.float()
    t = targets.long()
    zt = z.gather(1, t[:, None])
    greater = (z > zt).sum(1)
    return (greater < k) & torch.isfinite(zt[:, 0])


class _Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from .ops import kernels as K
        xc = x.contiguous()
        ctx.shape, ctx.dt = x.shape, x.dtype
        return K.sum_all(xc, 1.0 / max(1, xc.numel()))

    @staticmethod
    def backward(ctx, g):
        from .ops import kernels as K
        n = 1
        for d in ctx.shape:
            n *= d
        return K.fill_scaled(ctx.shape, g.to(ctx.dt).contiguous(), 1.0 / max(1, n), ctx.dt)


def reduce_mean(x):
    """tf.reduce_mean over all elements (0-d result)."""
    if _on_gpu(x):
        return _Mean.apply(x)
    return x.mean()


def l1_loss(w):
    return w.abs().sum()


def l2_loss(w):
    return 0.5 * (w * w).sum()


# ------------------------------------------------------------------ normalisation
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        from .ops import transformer as T
        shp = x.shape
        xb = x.reshape(-1, shp[-1]).to(torch.bfloat16).contiguous()
        g, b = gamma.float().contiguous(), beta.float().contiguous()
        y, s, mean, rstd = T.layernorm_fwd(xb, g, b, eps=eps)
        ctx.save_for_backward(s, mean, rstd, g)
        ctx.cfg = (shp, x.dtype, gamma.dtype)
        return y.reshape(shp).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        from .ops import transformer as T
        s, mean, rstd, g = ctx.saved_tensors
        shp, xdt, gdt = ctx.cfg
        H = shp[-1]
        dg = torch.empty(H, dtype=torch.float32, device=dy.device)
        db = torch.empty(H, dtype=torch.float32, device=dy.device)
        ds, _ = T.layernorm_bwd(dy.reshape(-1, H).to(torch.bfloat16).contiguous(), s, mean, rstd, g, dg, db)
        return ds.reshape(shp).to(xdt), dg.to(gdt), db.to(gdt), None


class _LayerNormGeneric(torch.autograd.Function):
    """Any width, fp32 or bf16 (nn_generic.hip): wave-per-row statistics, deterministic
    column-partial dgamma/dbeta."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        from .ops import kernels as K
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        g, b = _f32(gamma), _f32(beta)
        y, mean, rstd = K.ln_generic_fwd(x2, g, b, eps)
        ctx.save_for_backward(x2, g, mean, rstd)
        ctx.cfg = (shp, gamma.dtype, beta.dtype)
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        x2, g, mean, rstd = ctx.saved_tensors
        shp, gdt, bdt = ctx.cfg
        H = shp[-1]
        dg = torch.empty(H, dtype=torch.float32, device=dy.device)
        db = torch.empty(H, dtype=torch.float32, device=dy.device)
        d2 = dy.reshape(-1, H).contiguous().to(x2.dtype)
        dx = K.ln_generic_bwd(d2, x2, g, mean, rstd, dg, db, want_dx=ctx.needs_input_grad[0])
        return (dx.reshape(shp) if dx is not None else None), dg.to(gdt), db.to(bdt), None


_LN_FAST_WIDTHS = (512, 1024, 1536, 2048, 4096)


def layer_norm(x, gamma, beta, eps: float = 1e-12):
    if _on_gpu(x):
        if x.dtype == torch.bfloat16 and x.shape[-1] in _LN_FAST_WIDTHS:
            return _LayerNorm.apply(x, gamma, beta, float(eps))   # vectorised BERT kernel
        return _LayerNormGeneric.apply(x, gamma, beta, float(eps))
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


class _RMSNorm(torch.autograd.Function):
    """bf16 at a fast width (rmsnorm_glu.hip): wave per row, the row in registers."""

    @staticmethod
    def forward(ctx, x, gamma, eps):
        from .ops import transformer as T
        shp = x.shape
        xb = x.reshape(-1, shp[-1]).contiguous()
        g = _f32(gamma)
        y, s, rstd = T.rmsnorm_fwd(xb, g, eps=eps)
        ctx.save_for_backward(s, rstd, g)
        ctx.cfg = (shp, gamma.dtype)
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        from .ops import transformer as T
        s, rstd, g = ctx.saved_tensors
        shp, gdt = ctx.cfg
        H = shp[-1]
        dg = torch.empty(H, dtype=torch.float32, device=dy.device)
        ds, _ = T.rmsnorm_bwd(dy.reshape(-1, H).to(torch.bfloat16).contiguous(), s, rstd, g, dg)
        return ds.reshape(shp), dg.to(gdt), None


class _RMSNormGeneric(torch.autograd.Function):
    """Any width, fp32 or bf16 (rmsnorm_glu.hip): wave-per-row statistic, deterministic
    column-partial dgamma."""

    @staticmethod
    def forward(ctx, x, gamma, eps):
        from .ops import kernels as K
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        g = _f32(gamma)
        y, rstd = K.rms_generic_fwd(x2, g, eps)
        ctx.save_for_backward(x2, g, rstd)
        ctx.cfg = (shp, gamma.dtype)
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        x2, g, rstd = ctx.saved_tensors
        shp, gdt = ctx.cfg
        H = shp[-1]
        dg = torch.empty(H, dtype=torch.float32, device=dy.device)
        d2 = dy.reshape(-1, H).contiguous().to(x2.dtype)
        dx = K.rms_generic_bwd(d2, x2, g, rstd, dg, want_dx=ctx.needs_input_grad[0])
        return (dx.reshape(shp) if dx is not None else None), dg.to(gdt), None


def rms_norm(x, gamma, eps: float = 1e-6):
    """y = x * rsqrt(mean(x^2, -1) + eps) * gamma over the last axis (RMSNorm; statistic in fp32).
    GPU: bf16 at a LayerNorm fast width runs the vectorised kernel, any other width or fp32 the
    generic one (fp32 stays fp32). CPU: the fp32 formula in torch ops."""
    if x.dim() < 1 or x.shape[-1] < 1 or gamma.dim() != 1 or gamma.shape[0] != x.shape[-1]:
        raise InvalidArgumentError("ttd.nn.rms_norm: gamma must be [%s] for x %s, got %s"
                                   % (x.shape[-1] if x.dim() else "?", tuple(x.shape), tuple(gamma.shape)))
    if _on_gpu(x):
        if x.numel() == 0:
            raise InvalidArgumentError("ttd.nn.rms_norm: empty input %s" % (tuple(x.shape),))
        if x.dtype == torch.bfloat16 and x.shape[-1] in _LN_FAST_WIDTHS:
            return _RMSNorm.apply(x, gamma, float(eps))
        return _RMSNormGeneric.apply(x, gamma, float(eps))
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()
    return y.to(x.dtype)


class _GroupNorm(torch.autograd.Function):
    """Any [N, *spatial, C], fp32 or bf16 (groupnorm.hip): slab partial sums folded in a fixed
    order, per-(n, c) coefficient rows for the two apply kernels."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps):
        from .ops import kernels as K
        shp = x.shape
        x3 = x.reshape(shp[0], -1, shp[-1]).contiguous()
        g = _f32(gamma)
        y, mean, rstd = K.group_norm_fwd(x3, g, _f32(beta), groups, eps)
        ctx.save_for_backward(x3, g, mean, rstd)
        ctx.cfg = (shp, None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return y.reshape(shp)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        x3, g, mean, rstd = ctx.saved_tensors
        shp, gdt, bdt = ctx.cfg
        C = shp[-1]
        need = ctx.needs_input_grad
        dg = torch.empty(C, dtype=torch.float32, device=dy.device) if gdt is not None and need[1] else None
        db = torch.empty(C, dtype=torch.float32, device=dy.device) if bdt is not None and need[2] else None
        d3 = dy.reshape(x3.shape).contiguous().to(x3.dtype)
        dx = K.group_norm_bwd(d3, x3, g, mean, rstd, dg, db, want_dx=need[0])
        return ((dx.reshape(shp) if dx is not None else None), (dg.to(gdt) if dg is not None else None),
                (db.to(bdt) if db is not None else None), None, None)


def group_norm(x, gamma, beta, groups: int = 32, eps: float = 1e-3):
    """Group normalisation over the last (channel) axis of x [N, *spatial, C] (Keras
    GroupNormalization(axis=-1)): mean and biased variance over the spatial positions and the
    C / groups consecutive channels of each group, per sample; y = (x - mean) * rsqrt(var + eps)
    * gamma + beta with gamma / beta [C] or None. Statistics in fp32. GPU: groupnorm.hip, bf16
    with C % 8 == 0 on the vectorised form, anything else (fp32 stays fp32) on the generic one.
    CPU: the fp32 formula in torch ops."""
    groups = int(groups)
    if x.dim() < 2:
        raise InvalidArgumentError("ttd.nn.group_norm: x must be [N, ..., C] of rank >= 2, got %s" % (tuple(x.shape),))
    C = x.shape[-1]
    if groups < 1 or C < 1 or C % groups:
        raise InvalidArgumentError("ttd.nn.group_norm: groups = %d must be positive and divide the %d channels"
                                   % (groups, C))
    for name, v in (("gamma", gamma), ("beta", beta)):
        if v is not None and (v.dim() != 1 or v.shape[0] != C):
            raise InvalidArgumentError("ttd.nn.group_norm: %s must be [%d] for x %s, got %s"
                                       % (name, C, tuple(x.shape), tuple(v.shape)))
        if v is not None and v.device != x.device:
            raise InvalidArgumentError("ttd.nn.group_norm: %s is on %s, x on %s" % (name, v.device, x.device))
    if _on_gpu(x, gamma, beta):
        if x.numel() == 0:
            raise InvalidArgumentError("ttd.nn.group_norm: empty input %s" % (tuple(x.shape),))
        return _GroupNorm.apply(x, gamma, beta, groups, float(eps))
    shp = x.shape
    xf = x.float().reshape(shp[0], -1, groups, C // groups)
    mean = xf.mean((1, 3), keepdim=True)
    var = (xf - mean).pow(2).mean((1, 3), keepdim=True)
    y = ((xf - mean) * torch.rsqrt(var + eps)).reshape(shp)
    if gamma is not None:
        y = y * gamma.float()
    if beta is not None:
        y = y + beta.float()
    return y.to(x.dtype)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from .ops import transformer as T
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        h = T.swiglu_fwd(x2)
        ctx.save_for_backward(x2)
        ctx.shp = shp
        return h.reshape(shp[:-1] + (shp[-1] // 2,))

    @staticmethod
    def backward(ctx, dh):
        from .ops import transformer as T
        (x2,) = ctx.saved_tensors
        shp = ctx.shp
        d2 = dh.reshape(-1, shp[-1] // 2).contiguous().to(x2.dtype)
        return T.swiglu_bwd(d2, x2).reshape(shp)


def swiglu(x):
    """silu(a) * b for x = [a | b] split in halves along the last axis (gate first): the gated unit of
    a LLaMA-style feed-forward. GPU bf16 / fp32 run the SwiGLU kernel; CPU is F.silu(a) * b."""
    if x.dim() < 1 or x.shape[-1] % 2 or x.shape[-1] == 0:
        raise InvalidArgumentError("ttd.nn.swiglu: the last dimension must be even and non-zero, got %s"
                                   % (tuple(x.shape),))
    if _on_gpu(x):
        if x.numel() == 0:
            raise InvalidArgumentError("ttd.nn.swiglu: empty input %s" % (tuple(x.shape),))
        return _SwiGLU.apply(x)
    a, b = x.chunk(2, dim=-1)
    return F.silu(a) * b


class _BatchNorm(torch.autograd.Function):
    """NHWC BatchNorm over all but the channel axis on the GPU: column statistics
    (nn_generic.hip) folded by the ResNet engine's finalize kernel (batchnorm.hip: mean/rstd,
    scale/shift, TF moving-average update with the unbiased variance), one affine pass; the
    backward is (sum g, sum g*x) -> dgamma/dbeta + coefficients -> one affine pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_variance, training, momentum, eps):
        from .ops import kernels as K
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        M = x2.shape[0]
        g, b = _f32(gamma), _f32(beta)
        if training:
            part, T = K.col_stats(x2, mode=0)
            st = K.BNState(C, x.device)
            for t in (moving_mean, moving_variance):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                    raise InvalidArgumentError("batch_norm moving statistics must be contiguous fp32 GPU tensors")
            K.bn_fwd_stats(part, T, M, g, b, eps, momentum, moving_mean, moving_variance, st)
            y = K.col_affine(x2, st.scale, c2=st.shift)
            ctx.save_for_backward(x2, g, st.mean, st.rstd, None)
        else:
            if moving_mean is None or moving_variance is None:
                raise InvalidArgumentError("batch_norm(training=False) needs moving_mean/moving_variance")
            mm = moving_mean.float().contiguous()
            scale, shift, rstd = K.bn_infer_coef(mm, moving_variance.float().contiguous(), g, b, eps)
            y = K.col_affine(x2, scale, c2=shift)
            ctx.save_for_backward(x2, g, mm, rstd, scale)
        ctx.cfg = (training, x.shape, None if gamma is None else gamma.dtype, None if beta is None else beta.dtype)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        x2, g, mean, rstd, scale = ctx.saved_tensors
        training, shp, gdt, bdt = ctx.cfg
        M, C = x2.shape
        d2 = dy.reshape(-1, C).contiguous().to(x2.dtype)
        dgamma = torch.empty(C, dtype=torch.float32, device=dy.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=dy.device)
        part, T = K.col_stats(d2, x2, mode=1)
        if training:
            st = K.BNState(C, dy.device)
            st.mean, st.rstd = mean, rstd
            coef = K.bn_backward_coef(M, C, g, st, dgamma, dbeta, part, T, device=dy.device)
            dx = K.col_affine(d2, coef[0], b=x2, c1=coef[1], c2=coef[2])
        else:
            K.bn_infer_bwd(part, T, mean, rstd, dgamma, dbeta)
            dx = K.col_affine(d2, scale)
        dg = dgamma.to(gdt) if gdt is not None else None
        db = dbeta.to(bdt) if bdt is not None else None
        return dx.reshape(shp), dg, db, None, None, None, None, None


def batch_norm(x, gamma, beta, moving_mean=None, moving_variance=None, training=True, momentum=0.99,
               eps=1e-3):
    """NHWC batch normalisation over all but the last axis (tf.layers.batch_normalization);
    updates the moving statistics in place when training."""
    if _on_gpu(x):
        return _BatchNorm.apply(x, gamma, beta, moving_mean, moving_variance, bool(training), float(momentum),
                                float(eps))
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if training:
        mean = x2.float().mean(0)
        var = x2.float().var(0, unbiased=False)
        if moving_mean is not None:
            with torch.no_grad():
                n = x2.shape[0]
                moving_mean.mul_(momentum).add_((1 - momentum) * mean.detach())
                moving_variance.mul_(momentum).add_((1 - momentum) * var.detach() * n / max(1, n - 1))
    else:
        mean, var = moving_mean, moving_variance
    y = (x2.float() - mean) * torch.rsqrt(var + eps)
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return y.reshape(x.shape).to(x.dtype)


# ------------------------------------------------------------------ convolution
class _Conv2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, stride, padding):
        from .ops import gemm as G
        xb = x.to(torch.bfloat16).contiguous()
        wk = kernel.permute(3, 0, 1, 2).to(torch.bfloat16).contiguous()  # [R,S,C,K] -> [K,R,S,C]
        y = G.conv_fwd(xb, wk, stride, padding)
        ctx.save_for_backward(xb, wk)
        ctx.cfg = (stride, padding, x.dtype, kernel.dtype)
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        from .ops import gemm as G
        from .ops import kernels as K
        xb, wk = ctx.saved_tensors
        stride, padding, xdt, wdt = ctx.cfg
        d = dy.to(torch.bfloat16).contiguous()
        dw = G.conv_wgrad(xb, d, tuple(wk.shape), stride, padding)  # [K,R,S,C] fp32
        dx = None
        if ctx.needs_input_grad[0]:
            dx = G.conv_dgrad(d, K.krsc_to_crsk(wk), xb.shape, stride, padding).to(xdt)
        return dx, dw.permute(1, 2, 3, 0).to(wdt), None, None


def _same_pad(size, k, s):
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def conv2d(x, kernel, strides=(1, 1), padding="SAME"):
    """NHWC conv; kernel [R, S, C, K] (TF layout). padding 'SAME' | 'VALID' | (ph, pw)."""
    if isinstance(strides, int):
        strides = (strides, strides)
    R, S = kernel.shape[0], kernel.shape[1]
    if isinstance(padding, str):
        if padding.upper() == "VALID":
            pads = (0, 0)
            extra = None
        else:
            (ph0, ph1), (pw0, pw1) = _same_pad(x.shape[1], R, strides[0]), _same_pad(x.shape[2], S, strides[1])
            pads = (ph0, pw0)
            extra = (ph1 - ph0, pw1 - pw0)
            if extra != (0, 0):  # asymmetric SAME padding: pad explicitly (right/bottom)
                x = F.pad(x, (0, 0, 0, pw1 - pw0, 0, ph1 - ph0))
    else:
        pads = tuple(padding)
    if _on_gpu(x):
        C, K = x.shape[-1], kernel.shape[-1]
        Cp, Kp = -(-C // 8) * 8, -(-K // 8) * 8
        if Cp != C or Kp != K:  # the implicit-GEMM kernels want channel counts % 8: zero-pad
            x = F.pad(x, (0, Cp - C))
            kernel = F.pad(kernel, (0, Kp - K, 0, Cp - C))
        y = _Conv2D.apply(x, kernel, tuple(strides), pads)
        return y[..., :K] if Kp != K else y
    y = F.conv2d(x.permute(0, 3, 1, 2), kernel.permute(3, 2, 0, 1), stride=strides, padding=pads)
    return y.permute(0, 2, 3, 1)


def _pair(v):
    if isinstance(v, int):
        return v, v
    v = tuple(v)
    if len(v) == 4:  # TF NHWC [1, kh, kw, 1]
        return v[1], v[2]
    return v[0], v[1]


class _DepthwiseConv2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, geom):
        from .ops import kernels as K
        xc = x.contiguous()
        wf = kernel.float().contiguous()  # the kernels take the (tiny) filter as fp32
        y = K.dwconv_fwd(xc, wf, geom)
        ctx.save_for_backward(xc, wf)
        ctx.cfg = (geom, kernel.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        xc, wf = ctx.saved_tensors
        geom, wdt = ctx.cfg
        d = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = K.dwconv_wgrad(xc, d, tuple(wf.shape), geom).to(wdt)
        if ctx.needs_input_grad[0]:
            dx = K.dwconv_dgrad(d, wf, tuple(xc.shape), geom)
        return dx, dw, None


def _dw_geometry(H, W, R, S, strides, padding, dilations):
    """(sh, sw, ph, pw, dh, dw, P, Q) of a depthwise conv: TF 'SAME' (the extra row / column goes
    to the bottom / right) / 'VALID', or explicit symmetric (ph, pw)."""
    (sh, sw), (dh, dw) = strides, dilations
    Re, Se = (R - 1) * dh + 1, (S - 1) * dw + 1  # dilated filter extent
    if isinstance(padding, str):
        if padding.upper() == "VALID":
            ph, pw, P, Q = 0, 0, (H - Re) // sh + 1, (W - Se) // sw + 1
        elif padding.upper() == "SAME":
            P, Q = -(-H // sh), -(-W // sw)
            ph, pw = max((P - 1) * sh + Re - H, 0) // 2, max((Q - 1) * sw + Se - W, 0) // 2
        else:
            raise InvalidArgumentError("padding must be 'SAME', 'VALID' or (ph, pw), got %r" % (padding,))
    else:
        ph, pw = _pair(padding)
        P, Q = (H + 2 * ph - Re) // sh + 1, (W + 2 * pw - Se) // sw + 1
    if P <= 0 or Q <= 0 or min(sh, sw, dh, dw) <= 0 or ph < 0 or pw < 0:
        raise InvalidArgumentError("depthwise_conv2d: empty output or bad strides / dilations / padding "
                                   "(input %dx%d, filter %dx%d)" % (H, W, R, S))
    return sh, sw, ph, pw, dh, dw, P, Q


def depthwise_conv2d(x, kernel, strides=(1, 1), padding="SAME", dilations=(1, 1)):
    """tf.nn.depthwise_conv2d: NHWC x [N,H,W,C], kernel [R,S,C,M] (R, S <= 7), output [N,P,Q,C*M]
    where channel c*M+m is input channel c filtered by kernel[:, :, c, m]. padding 'SAME' | 'VALID'
    | (ph, pw); strides / dilations an int, a pair or TF's [1, a, b, 1]. On the GPU fp32 stays
    fp32, bf16 accumulates in fp32, and the kernel's gradient is bitwise reproducible."""
    if x.dim() != 4 or kernel.dim() != 4:
        raise InvalidArgumentError("depthwise_conv2d takes x [N,H,W,C] and kernel [R,S,C,M], got %s and %s"
                                   % (tuple(x.shape), tuple(kernel.shape)))
    R, S, C, M = kernel.shape
    if C != x.shape[3]:
        raise InvalidArgumentError("depthwise_conv2d: kernel has %d input channels, x has %d" % (C, x.shape[3]))
    if R > 7 or S > 7:
        raise InvalidArgumentError("depthwise_conv2d: filters up to 7x7, got %dx%d" % (R, S))
    geom = _dw_geometry(x.shape[1], x.shape[2], R, S, _pair(strides), padding, _pair(dilations))
    if _on_gpu(x, kernel):
        return _DepthwiseConv2D.apply(x, kernel, geom)
    sh, sw, ph, pw, dh, dw, P, Q = geom
    # explicit zero padding (covers SAME's extra bottom / right row) then an unpadded grouped conv
    eh = max((P - 1) * sh + (R - 1) * dh + 1 - x.shape[1] - ph, 0)
    ew = max((Q - 1) * sw + (S - 1) * dw + 1 - x.shape[2] - pw, 0)
    xp = F.pad(x.float().permute(0, 3, 1, 2), (pw, ew, ph, eh))
    wk = kernel.float().permute(2, 3, 0, 1).reshape(C * M, 1, R, S)
    y = F.conv2d(xp, wk, stride=(sh, sw), dilation=(dh, dw), groups=C)
    return y[:, :, :P, :Q].permute(0, 2, 3, 1).to(x.dtype)


def separable_conv2d(x, depthwise_kernel, pointwise_kernel, strides=(1, 1), padding="SAME", dilations=(1, 1)):
    """tf.nn.separable_conv2d: depthwise_conv2d with depthwise_kernel [R,S,C,M], then conv2d with
    pointwise_kernel [1,1,C*M,K] (a plain GEMM)."""
    if pointwise_kernel.dim() != 4 or tuple(pointwise_kernel.shape[:2]) != (1, 1):
        raise InvalidArgumentError("separable_conv2d: pointwise_kernel must be [1,1,C*M,K], got %s"
                                   % (tuple(pointwise_kernel.shape),))
    y = depthwise_conv2d(x, depthwise_kernel, strides, padding, dilations)
    if pointwise_kernel.shape[2] != y.shape[3]:
        raise InvalidArgumentError("separable_conv2d: pointwise_kernel takes %d channels, the depthwise output has %d"
                                   % (pointwise_kernel.shape[2], y.shape[3]))
    return conv2d(y, pointwise_kernel, (1, 1), "VALID")


def _pool_geometry(H, W, k, s, padding):
    """(ph, pw, P, Q): TF 'SAME' / 'VALID' (SAME pads the extra row/column at the bottom/right)
    or explicit symmetric padding (int / pair)."""
    (R, S), (sh, sw) = k, s
    if isinstance(padding, str):
        if padding.upper() == "VALID":
            return 0, 0, (H - R) // sh + 1, (W - S) // sw + 1
        P, Q = -(-H // sh), -(-W // sw)
        return (max((P - 1) * sh + R - H, 0) // 2, max((Q - 1) * sw + S - W, 0) // 2, P, Q)
    ph, pw = _pair(padding)
    return ph, pw, (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, geo):
        from .ops import kernels as K
        xc = x.contiguous()
        (R, S), (sh, sw) = k, s
        ph, pw, P, Q = geo
        C = x.shape[-1]
        fast = (x.dtype == torch.bfloat16 and C % 8 == 0 and R == S and sh == sw and ph == pw
                and P == K.pool_out(x.shape[1], R, sh, ph) and Q == K.pool_out(x.shape[2], S, sw, pw))
        if fast:
            y, arg = K.maxpool_fwd(xc, R, sh, ph)
        else:
            y, arg = K.maxpool_generic_fwd(xc, R, S, sh, sw, ph, pw, P, Q)
        ctx.save_for_backward(arg)
        ctx.cfg = (fast, tuple(x.shape), k, s, geo)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        (arg,) = ctx.saved_tensors
        fast, xs, (R, S), (sh, sw), (ph, pw, _, _) = ctx.cfg
        d = dy.contiguous()
        if fast:
            return K.maxpool_bwd(d, arg, xs, R, sh, ph), None, None, None
        return K.maxpool_generic_bwd(d, arg, xs, R, S, sh, sw, ph, pw), None, None, None


def max_pool2d(x, ksize=3, strides=2, padding=1):
    """NHWC max pooling; ksize/strides int, pair or TF [1, k, k, 1]; padding 'SAME' | 'VALID'
    | int / pair (explicit, symmetric)."""
    k, s = _pair(ksize), _pair(strides)
    ph, pw, P, Q = _pool_geometry(x.shape[1], x.shape[2], k, s, padding)
    if _on_gpu(x):
        return _MaxPool.apply(x, k, s, (ph, pw, P, Q))
    # explicit -inf padding (covers TF SAME's extra bottom/right row) then an unpadded pool
    eh = max((P - 1) * s[0] + k[0] - x.shape[1] - 2 * ph, 0)
    ew = max((Q - 1) * s[1] + k[1] - x.shape[2] - 2 * pw, 0)
    xp = F.pad(x.permute(0, 3, 1, 2), (pw, pw + ew, ph, ph + eh), value=float("-inf"))
    y = F.max_pool2d(xp, k, s, 0)
    return y[:, :, :P, :Q].permute(0, 2, 3, 1)


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        from .ops import kernels as K
        xc = x.contiguous()
        fast = x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0
        ctx.cfg = (fast, tuple(x.shape))
        return K.avgpool_fwd(xc) if fast else K.gap_fwd(xc)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        fast, xs = ctx.cfg
        d = dy.contiguous()
        return K.avgpool_bwd(d, xs) if fast else K.gap_bwd(d, xs)


def global_avg_pool(x):
    if _on_gpu(x):
        return _GlobalAvgPool.apply(x)
    return x.mean(dim=(1, 2))


# ------------------------------------------------------------------ attention
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, num_heads, rate, seqlen, site, causal, num_kv_heads, band=None):
        from .ops import transformer as T
        B, S, D = q.shape
        Sk, Dk = k.shape[1], k.shape[2]  # Dk = num_kv_heads * 64: narrower than D when heads are grouped
        q2 = q.reshape(B * S, D).to(torch.bfloat16).contiguous()
        k2, v2 = [t.reshape(B * Sk, Dk).to(torch.bfloat16).contiguous() for t in (k, v)]
        o = torch.empty_like(q2)
        lse = torch.empty((B * num_heads, S), dtype=torch.float32, device=q.device)
        rng = None
        if rate > 0:
            rng = T.RngState(_Rng.seed, q.device)
            rng.t[1] = _Rng.offset
            _Rng.offset += 1
        if band is not None:  # seqlen and causal are in the table
            seqlen, causal = None, False
        T.attention_fwd(q2, k2, v2, o, lse, B, num_heads, S, Sk=Sk, Hk=num_kv_heads, seqlen=seqlen, p_drop=rate,
                        rng=rng, site=site, causal=causal, band=band)
        ctx.save_for_backward(q2, k2, v2, o, lse, seqlen, band)
        ctx.cfg = (B, S, Sk, D, Dk, num_heads, num_kv_heads, rate, rng, site, q.dtype, causal)
        return o.reshape(B, S, D).to(q.dtype)

    @staticmethod
    def backward(ctx, do):
        from .ops import transformer as T
        q2, k2, v2, o, lse, seqlen, band = ctx.saved_tensors
        B, S, Sk, D, Dk, nh, nkv, rate, rng, site, dt, causal = ctx.cfg
        d2 = do.reshape(B * S, D).to(torch.bfloat16).contiguous()
        dq, dk, dv = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2)
        T.attention_bwd(q2, k2, v2, o, d2, lse, dq, dk, dv, B, nh, S, Sk=Sk, Hk=nkv, seqlen=seqlen, p_drop=rate,
                        rng=rng, site=site, causal=causal, band=band)
        return (dq.reshape(B, S, D).to(dt), dk.reshape(B, Sk, Dk).to(dt), dv.reshape(B, Sk, Dk).to(dt),
                None, None, None, None, None, None, None)


def attention_band_mask(segment_ids, seqlen, window, causal, B, S, device):
    """Boolean [B, S(query), S(key)] mask of the banded attention (see attention): True where the
    query attends the key. The explicit form of the table the GPU kernels read."""
    ar = torch.arange(S, device=device)
    m = torch.ones((B, S, S), dtype=torch.bool, device=device)
    if segment_ids is not None:
        ids = segment_ids.to(device).long()
        start = torch.ones((B, S), dtype=torch.bool, device=device)
        start[:, 1:] = ids[:, 1:] != ids[:, :-1]
        run = start.long().cumsum(1)  # the number of the token's maximal run of equal ids
        valid = ids >= 0
        m = m & (run[:, :, None] == run[:, None, :]) & valid[:, :, None] & valid[:, None, :]
    if seqlen is not None:
        m = m & (ar[None, None, :] < seqlen.to(device).long()[:, None, None])
    left, right = (None, None) if window is None else window
    if causal:
        right = 0
    d = ar[None, :] - ar[:, None]  # key - query
    if left is not None:
        m = m & (d >= -int(left))[None]
    if right is not None:
        m = m & (d <= int(right))[None]
    return m


def attention(q, k, v, num_heads: int, dropout_rate: float = 0.0, seqlen=None, site: int = 0, causal: bool = False,
              num_kv_heads: Optional[int] = None, segment_ids=None, window=None):
    """Multi-head scaled dot-product attention, token-major inputs: q [B, S, num_heads*64], k and v
    [B, Sk, num_kv_heads*64]. Sk == S is self-attention; Sk != S is cross-attention over a memory of
    another length (a decoder's attention over the encoder's output): the result has the query's
    S rows, the gradients of k and v have Sk rows. Keys >= seqlen[b] are masked — seqlen is the
    keys' (the memory's) valid length, at most Sk; queries are never masked. causal=True also masks
    keys after the query (position s attends positions <= s: a left-to-right language model) and
    needs Sk == S. GPU: the flash kernels (head_dim 64, S % 128 == 0 and Sk % 128 == 0); their
    causal form skips the key tiles above the diagonal.
    num_kv_heads (None: num_heads) is grouped-query attention, num_kv_heads=1 multi-query attention:
    num_heads % num_kv_heads == 0 and query head h attends key/value head h // (num_heads //
    num_kv_heads) — the heads of a group are contiguous, as torch.repeat_interleave over the head
    axis lays them out. k and v are never repeated in memory, and their gradients come back
    num_kv_heads*64 wide, each key/value head the sum over the query heads of its group.
    Banded masks (self-attention only; they intersect with each other, with causal and with seqlen):
    segment_ids int32 [B, S] packs several documents into a row — a token attends the tokens of its
    own maximal run of equal ids (an id that reappears later in the row is another document); a
    negative id is padding: the token attends nothing and nothing attends it, its output row is
    exactly zero and so are its gradients. window=(left, right) is sliding-window attention,
    q - left <= k <= q + right, None on a side for no bound; causal=True clamps right to 0. A row
    whose intersection is empty behaves like a padding row. GPU: the table of
    ops.transformer.attention_band and the BAND kernels, which stream only the key tiles of each
    block's range; CPU: the same mask on the fp32 formulas (zero rows, not NaN). With
    segment_ids=None and no bound in window the call takes exactly the path it took without them."""
    from .ops import transformer as T
    B, S, D = q.shape
    wl, wr = T._band_window(window)
    banded = segment_ids is not None or wl >= 0 or wr >= 0
    Sk = k.shape[1]
    hd = D // num_heads
    nkv = int(num_heads) if num_kv_heads is None else int(num_kv_heads)
    if nkv <= 0 or num_heads % nkv:
        raise InvalidArgumentError(
            "ttd.nn.attention: num_heads must be a multiple of num_kv_heads (got num_heads %d, num_kv_heads %d)"
            % (num_heads, nkv))
    Dk = nkv * hd
    if tuple(k.shape) != (B, Sk, Dk) or tuple(v.shape) != (B, Sk, Dk):
        raise InvalidArgumentError(
            "ttd.nn.attention: k and v must both be [batch, key_len, num_kv_heads * head_dim = %d] with q's batch "
            "(got q %s, k %s, v %s, num_heads %d, num_kv_heads %d)"
            % (Dk, tuple(q.shape), tuple(k.shape), tuple(v.shape), num_heads, nkv))
    if causal and Sk != S:
        raise InvalidArgumentError(
            "ttd.nn.attention: causal=True needs as many keys as queries (got %d queries, %d keys)" % (S, Sk))
    if banded:
        if Sk != S:
            raise InvalidArgumentError(
                "ttd.nn.attention: segment_ids / window are self-attention masks (got %d queries, %d keys)" % (S, Sk))
        if segment_ids is not None and (tuple(segment_ids.shape) != (B, S) or segment_ids.dtype != torch.int32):
            raise InvalidArgumentError("ttd.nn.attention: segment_ids must be int32 [batch, seq_len] = [%d, %d], got "
                                       "%s %s" % (B, S, segment_ids.dtype, tuple(segment_ids.shape)))
    if _on_gpu(q, k, v):
        if hd != 64 or S % 128 != 0 or Sk % 128 != 0 or D % num_heads:
            raise InvalidArgumentError(
                "ttd.nn.attention on GPU runs the flash kernels for head_dim 64 and seq_len %% 128 == 0 "
                "(got head_dim %s, seq_len %d%s); pad the sequence (and mask it with seqlen) or use 64-wide heads"
                % (D / num_heads, S, "" if Sk == S else ", key seq_len %d" % Sk))
        sl = seqlen.to(torch.int32).contiguous() if seqlen is not None else None
        if banded:
            ids = segment_ids.to(q.device).contiguous() if segment_ids is not None else None
            band = T.attention_band(ids, sl.to(q.device) if sl is not None else None, window, causal, B, S,
                                    out=torch.empty(T.attention_band_ints(B, S), dtype=torch.int32, device=q.device))
            return _Attention.apply(q, k, v, num_heads, float(dropout_rate), None, int(site), False, nkv, band)
        return _Attention.apply(q, k, v, num_heads, float(dropout_rate), sl, int(site), bool(causal), nkv)
    qh = q.reshape(B, S, num_heads, hd).transpose(1, 2)
    kh = k.reshape(B, Sk, nkv, hd).transpose(1, 2)
    vh = v.reshape(B, Sk, nkv, hd).transpose(1, 2)
    if nkv != num_heads:
        # grouped heads: repeated inside the computation, so autograd sums each group's gradients
        kh = kh.repeat_interleave(num_heads // nkv, dim=1)
        vh = vh.repeat_interleave(num_heads // nkv, dim=1)
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    if seqlen is not None:
        m = torch.arange(Sk, device=q.device)[None, :] < seqlen[:, None].long()
        sc = sc.masked_fill(~m[:, None, None, :], float("-inf"))
    if causal:
        tri = torch.ones((S, S), dtype=torch.bool, device=q.device).tril()
        sc = sc.masked_fill(~tri, float("-inf"))
    if banded:
        m = attention_band_mask(segment_ids, seqlen, window, causal, B, S, q.device)
        sc = sc.masked_fill(~m[:, None], float("-inf"))
        dead = ~m.any(-1)[:, None, :, None]  # rows that attend nothing: zeros, not softmax's NaN
        sc = sc.masked_fill(dead, 0.0)
        p = sc.softmax(-1).masked_fill(dead, 0.0)
    else:
        p = sc.softmax(-1)
    if dropout_rate > 0:
        p = F.dropout(p, dropout_rate, training=True)
    return (p @ vh).transpose(1, 2).reshape(B, S, D)


# ------------------------------------------------------------------ rotary position embeddings
def _token_rows(t, B, S, D):
    """[B*S, D] view of t [B, S, D] that the rope kernel can take as it is (unit column stride,
    uniformly strided 16-byte aligned rows: a column slice of a fused projection is one), else of a
    contiguous copy."""
    es = t.element_size()
    ok = (t.stride(2) == 1 and t.stride(1) >= D and (B == 1 or t.stride(0) == S * t.stride(1))
          and (t.stride(1) * es) % 16 == 0 and t.data_ptr() % 16 == 0)
    if not ok:
        t = t.contiguous()
    return t.as_strided((B * S, D), (t.stride(1), 1))


class _Rotary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, num_heads, table, offset):
        from .ops import transformer as T
        B, S, D = x.shape
        y = torch.empty((B * S, D), dtype=x.dtype, device=x.device)
        T.rope(_token_rows(x, B, S, D), y, table, S, num_heads, pos0=offset)
        ctx.cfg = (num_heads, table, offset)
        return y.view(B, S, D)

    @staticmethod
    def backward(ctx, dy):
        from .ops import transformer as T
        num_heads, table, offset = ctx.cfg
        B, S, D = dy.shape
        dx = torch.empty((B * S, D), dtype=dy.dtype, device=dy.device)
        T.rope(_token_rows(dy, B, S, D), dx, table, S, num_heads, pos0=offset, inverse=True)
        return dx.view(B, S, D), None, None, None


def rotary_embedding(x, num_heads: int, base: float = 10000.0, offset: int = 0):
    """Rotary position embedding (RoPE) of x [B, S, num_heads*head_dim], half-split convention
    ("rotate_half", LLaMA / GPT-NeoX): in every head, with half = head_dim // 2, i in [0, half),
    theta_i = base**(-i/half) and p = offset + s the position of token s,
        y[i]        = x[i] * cos(p theta_i) - x[i + half] * sin(p theta_i)
        y[i + half] = x[i + half] * cos(p theta_i) + x[i] * sin(p theta_i).
    Apply it to q and k before attention (`offset`: the position of the first token, e.g. the
    length of a cached prefix). The result has x's shape and dtype; the backward is the inverse
    rotation of the incoming gradient (the rotation is orthogonal), the same kernel with -sin.
    GPU: head_dim 64 only, any S; bf16 stays bf16 and fp32 stays fp32 (rope.hip, cos / sin from a
    host-built table: ops.transformer.rope_table, offset + S rows rounded up to a power of two, at
    least 512). A view with unit column stride and uniformly strided rows — a column slice of a
    fused projection — is read through its row stride without a copy. CPU: the same convention in
    fp32 torch ops for any even head_dim."""
    if x.dim() != 3:
        raise InvalidArgumentError("ttd.nn.rotary_embedding: x must be [batch, seq_len, num_heads * head_dim] "
                                   "(got shape %s)" % (tuple(x.shape),))
    B, S, D = x.shape
    num_heads, offset = int(num_heads), int(offset)
    if num_heads <= 0 or D % num_heads:
        raise InvalidArgumentError(
            "ttd.nn.rotary_embedding: num_heads must divide the width (got width %d, num_heads %d)" % (D, num_heads))
    hd = D // num_heads
    if hd % 2:
        raise InvalidArgumentError(
            "ttd.nn.rotary_embedding: head_dim must be even, the rotation pairs column i with i + head_dim/2 "
            "(got head_dim %d)" % hd)
    if offset < 0:
        raise InvalidArgumentError("ttd.nn.rotary_embedding: offset must be >= 0 (got %d)" % offset)
    if _on_gpu(x):
        if hd != 64:
            raise InvalidArgumentError(
                "ttd.nn.rotary_embedding on GPU runs the rotary kernel for head_dim 64 (got head_dim %d); "
                "use 64-wide heads" % hd)
        from .ops import transformer as T
        rows = max(512, 1 << (offset + S - 1).bit_length())
        if B * S == 0:
            return x.clone()
        return _Rotary.apply(x, num_heads, T.rope_table(rows, base, x.device), offset)
    half = hd // 2
    pos = torch.arange(offset, offset + S, dtype=torch.float64)
    ang = pos[:, None] * float(base) ** (-torch.arange(half, dtype=torch.float64) / half)
    cos, sin = ang.cos().float()[None, :, None, :], ang.sin().float()[None, :, None, :]
    xh = x.float().reshape(B, S, num_heads, hd)
    lo, hi = xh[..., :half], xh[..., half:]
    y = torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], dim=-1)
    return y.reshape(B, S, D).to(x.dtype)


class _Embedding(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, ids):
        from .ops import kernels as K
        idc = ids.contiguous() if ids.dtype in (torch.int32, torch.int64) else ids.long().contiguous()
        ctx.save_for_backward(idc)
        ctx.cfg = (tuple(params.shape), params.dtype)
        return K.gather_generic(params.contiguous(), idc)

    @staticmethod
    def backward(ctx, dy):
        from .ops import kernels as K
        (idc,) = ctx.saved_tensors
        shp, dt = ctx.cfg
        dtable = K.zeros(shp, dtype=torch.float32, device=dy.device)
        K.scatter_add_generic(dy.reshape(-1, shp[1]).contiguous(), idc, dtable)
        return (dtable if dt == torch.float32 else dtable.to(dt)), None


def embedding_lookup(params, ids):
    """tf.nn.embedding_lookup (single table): rows of params [V, H] for ids of any shape; on GPU
    out-of-range ids give zero rows (tf.gather's GPU behaviour)."""
    if _on_gpu(params):
        return _Embedding.apply(params, ids)
    return F.embedding(ids.long(), params)
