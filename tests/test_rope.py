"""Rotary position embeddings (half-split convention, head size 64 on the GPU): the kernel of
rope.hip behind `ops.transformer.rope` / `rope_table`, `ttd.nn.rotary_embedding` (GPU kernel and CPU
path), `layers.MultiHeadAttention(rotary=True)` and the BERT engine (`BertConfig.rotary`).

The oracle is written here, independently of the package: float64 cos / sin of
p * base**(-i/half) and a float64 rotation of the inputs.

bf16 bars of the kernel tests: |got - want64| <= 2^-7 |want64| + 1e-5 (half a bf16 ulp of the final
rounding plus half an ulp for fp32 / FMA differences before it), and at least 99.9 % of the elements
bit-equal to want64 rounded to bf16. fp32 bar: |got - want64| <= 1e-6 (|x_lo| + |x_hi|) of the pair
that forms the element (a few fp32 ulps of the two products and of the fp32 table)."""
import math

import numpy as np
import pytest
import torch

from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.models.bert import BertConfig, BertPretraining, synthetic_batch
from tensorflow_train_distributed_amd.ops import transformer as T
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ float64 oracle
def _cos_sin64(positions, half=32, base=10000.0):
    """cos, sin float64 [len(positions), half]."""
    p = np.asarray(positions, dtype=np.float64)[:, None]
    ang = p * base ** (-np.arange(half, dtype=np.float64) / half)
    return np.cos(ang), np.sin(ang)


def _rot64(x, S, heads, pos0=0, inverse=False, base=10000.0):
    """float64 rotation of x [tokens, heads*hd] (torch, any float dtype), row r at position
    pos0 + r % S. Returns a float64 torch tensor."""
    x = x.detach().cpu().double().numpy()
    tokens, width = x.shape
    hd = width // heads
    half = hd // 2
    cos, sin = _cos_sin64(pos0 + np.arange(tokens) % S, half, base)
    if inverse:
        sin = -sin
    xh = x.reshape(tokens, heads, hd)
    lo, hi = xh[..., :half], xh[..., half:]
    c, s = cos[:, None, :], sin[:, None, :]
    y = np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1)
    return torch.from_numpy(y.reshape(tokens, width))


def _pair_scale(x, heads):
    """|x_lo| + |x_hi| of the pair behind every element, float64 [tokens, heads*64]."""
    a = x.detach().cpu().double().abs().reshape(x.shape[0], heads, 2, 32)
    s = a[:, :, 0] + a[:, :, 1]
    return torch.stack([s, s], dim=2).reshape(x.shape[0], heads * 64)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check_against_oracle(got, want64, x, heads):
    got = got.detach().cpu()
    err = (got.double() - want64).abs()
    if got.dtype == torch.bfloat16:
        bound = 2.0 ** -7 * want64.abs() + 1e-5
        worst = float((err / bound).max())
        share = float((_bits(got) == _bits(want64.bfloat16())).double().mean())
        print("bf16: worst error / bound %.3f, bit-equal share %.5f" % (worst, share))
        assert worst <= 1.0, worst
        assert share >= 0.999, share
    else:
        scale = _pair_scale(x, heads)
        worst = float((err / scale.clamp(min=1e-30)).max())
        print("fp32: worst error / (|x_lo| + |x_hi|) %.3g" % worst)
        assert bool((err <= 1e-6 * scale).all()), worst


# ------------------------------------------------------------------ CPU
def test_rope_table_is_the_float64_formula_and_cached():
    t = T.rope_table(300, device="cpu")
    cos, sin = _cos_sin64(np.arange(300))
    want = torch.from_numpy(np.stack([cos, sin], axis=1).astype(np.float32))
    assert t.shape == (300, 2, 32) and t.dtype == torch.float32
    assert torch.equal(t, want)
    assert T.rope_table(300, device="cpu") is t
    assert T.rope_table(300, base=500.0, device="cpu") is not t


@pytest.mark.parametrize("offset", [0, 57])
def test_nn_rotary_embedding_cpu_matches_oracle(offset):
    torch.manual_seed(0)
    B, S, H = 2, 70, 3
    x = torch.randn(B, S, H * 64)
    y = N.rotary_embedding(x, H, offset=offset)
    assert y.shape == x.shape and y.dtype == x.dtype
    want = _rot64(x.reshape(B * S, -1), S, H, pos0=offset).reshape(B, S, -1)
    torch.testing.assert_close(y.double(), want, atol=1e-5, rtol=1e-5)
    assert not torch.allclose(y, x, atol=1e-2)
    # another even head size and base on the CPU path
    x2 = torch.randn(B, S, 4 * 24)
    want2 = _rot64(x2.reshape(B * S, -1), S, 4, pos0=offset, base=500.0).reshape(B, S, -1)
    torch.testing.assert_close(N.rotary_embedding(x2, 4, base=500.0, offset=offset).double(), want2, atol=1e-5,
                               rtol=1e-5)


def test_nn_rotary_embedding_cpu_gradient_is_the_inverse_rotation():
    torch.manual_seed(1)
    B, S, H = 2, 70, 3
    x = torch.randn(B, S, H * 64, requires_grad=True)
    g = torch.randn(B, S, H * 64)
    N.rotary_embedding(x, H, offset=57).backward(g)
    want = _rot64(g.reshape(B * S, -1), S, H, pos0=57, inverse=True).reshape(B, S, -1)
    torch.testing.assert_close(x.grad.double(), want, atol=1e-5, rtol=1e-5)


def test_nn_rotary_embedding_refusals():
    x = torch.randn(2, 16, 192)
    with pytest.raises(InvalidArgumentError):
        N.rotary_embedding(x, 5)            # 5 does not divide 192
    with pytest.raises(InvalidArgumentError):
        N.rotary_embedding(x, 0)
    with pytest.raises(InvalidArgumentError):
        N.rotary_embedding(x, 64)           # head_dim 3: odd
    with pytest.raises(InvalidArgumentError):
        N.rotary_embedding(x, 3, offset=-1)


def _set_weights(layer, D, inner, ikv, seed):
    """O(1/sqrt(fan_in)) bf16-representable weights: q, k, v and the output are O(1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.qkv_kernel.copy_((torch.randn(D, inner + 2 * ikv, generator=g) / math.sqrt(D)).bfloat16().float())
        layer.qkv_bias.copy_((torch.randn(inner + 2 * ikv, generator=g) * 0.1).bfloat16().float())
        layer.out_kernel.copy_((torch.randn(inner, D, generator=g) / math.sqrt(inner)).bfloat16().float())
        layer.out_bias.copy_((torch.randn(D, generator=g) * 0.1).bfloat16().float())


def test_multi_head_attention_rotary_has_the_same_variables():
    L.reset_naming(0)
    x = torch.randn(2, 16, 96)
    a, b = L.MultiHeadAttention(4, num_kv_heads=2, rotary=True), L.MultiHeadAttention(4, num_kv_heads=2)
    with torch.no_grad():
        a(x), b(x)
    va = [(n.split("/", 1)[1], tuple(t.shape)) for n, t in a.named_variables()]
    vb = [(n.split("/", 1)[1], tuple(t.shape)) for n, t in b.named_variables()]
    assert va == vb and len(va) == 4


@pytest.mark.parametrize("mode", ["plain", "causal", "cross"])
def test_multi_head_attention_rotary_cpu_is_the_by_hand_composition(mode):
    torch.manual_seed(2)
    L.reset_naming(0)
    B, S, Sk, D, H, Hk = 2, 70, 45, 96, 4, 2
    inner, ikv = H * 64, Hk * 64
    x = torch.randn(B, S, D)
    mem = torch.randn(B, Sk, D) if mode == "cross" else None
    causal = mode == "causal"
    layer, plain = L.MultiHeadAttention(H, num_kv_heads=Hk, rotary=True), L.MultiHeadAttention(H, num_kv_heads=Hk)
    with torch.no_grad():
        layer(x), plain(x)
        _set_weights(layer, D, inner, ikv, 5)
        plain.load_state_dict(layer.state_dict())
        got = layer(x, value=mem, use_causal_mask=causal)
        if mem is None:
            qkv = N.dense(x, layer.qkv_kernel, layer.qkv_bias)
            q, k, v = qkv[..., :inner], qkv[..., inner:inner + ikv], qkv[..., inner + ikv:]
        else:
            q = N.dense(x, layer.qkv_kernel[:, :inner].contiguous(), layer.qkv_bias[:inner].contiguous())
            kv = N.dense(mem, layer.qkv_kernel[:, inner:].contiguous(), layer.qkv_bias[inner:].contiguous())
            k, v = kv[..., :ikv], kv[..., ikv:]
        q, k = N.rotary_embedding(q.contiguous(), H), N.rotary_embedding(k.contiguous(), Hk)
        a = N.attention(q, k, v.contiguous(), H, causal=causal, num_kv_heads=Hk)
        want = N.dense(a, layer.out_kernel, layer.out_bias)
        torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-4)
        assert not torch.allclose(got, plain(x, value=mem, use_causal_mask=causal), atol=1e-3)


def test_bert_config_rotary_defaults_off():
    assert BertConfig().rotary is False
    assert BertConfig().rotary_base == 10000.0


# ------------------------------------------------------------------ GPU kernel vs the oracle
def _run_case(dtype, inplace, inverse, pos0, B, S, heads, extra=192, lead=128):
    """x is a column view [B*S, heads*64] of a wider buffer (row stride != rotated width, the view
    starts `lead` columns in); out of place y is a whole sentinel-filled buffer of the same width."""
    torch.manual_seed(S + heads + pos0)
    W = heads * 64
    buf = torch.randn(B * S, W + extra, device="cuda").to(dtype)
    before = buf.clone()
    x = buf[:, lead:lead + W]
    table = T.rope_table(max(512, 1 << (pos0 + S - 1).bit_length()), device="cuda")
    want = _rot64(before[:, lead:lead + W], S, heads, pos0=pos0, inverse=inverse)
    if inplace:
        T.rope(x, x, table, S, heads, pos0=pos0, inverse=inverse)
        got = x
        assert torch.equal(_bits(buf[:, :lead]), _bits(before[:, :lead]))
        assert torch.equal(_bits(buf[:, lead + W:]), _bits(before[:, lead + W:]))
    else:
        ybuf = torch.full((B * S, W + extra), -77.0, device="cuda", dtype=dtype)
        T.rope(x, ybuf, table, S, heads, pos0=pos0, inverse=inverse)
        got = ybuf[:, :W]
        assert torch.equal(_bits(ybuf[:, W:]), _bits(torch.full_like(ybuf[:, W:], -77.0)))
        assert torch.equal(_bits(buf), _bits(before))
    _check_against_oracle(got, want, before[:, lead:lead + W], heads)


@gpu
@pytest.mark.parametrize("pos0", [0, 57])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_kernel_matches_oracle(dtype, inplace, inverse, pos0):
    _run_case(dtype, inplace, inverse, pos0, B=2, S=200, heads=5)


@gpu
def test_rope_kernel_grid_stride_coverage():
    """More work items (tokens * heads * 4 for bf16) than the capped grid has threads."""
    B, S, heads = 2, 2048, 40
    assert B * S * heads * 4 > T.rope_max_threads()
    _run_case(torch.bfloat16, True, False, 0, B=B, S=S, heads=heads, extra=64, lead=0)


@gpu
def test_rope_kernel_position_offset():
    torch.manual_seed(3)
    x = torch.randn(256, 128, device="cuda").bfloat16()
    table = T.rope_table(512, device="cuda")
    whole = T.rope(x, torch.empty_like(x), table, 256, 2)
    tail = T.rope(x[128:], torch.empty_like(x[128:]), table, 128, 2, pos0=128)
    assert torch.equal(whole[128:], tail)
    assert not torch.equal(whole[:128], tail)


@gpu
def test_rope_kernel_round_trip():
    torch.manual_seed(4)
    B, S, heads = 2, 200, 5
    x = torch.randn(B * S, heads * 64, device="cuda").bfloat16()
    table = T.rope_table(512, device="cuda")
    y = T.rope(x, torch.empty_like(x), table, S, heads, pos0=57)
    z = T.rope(y, torch.empty_like(x), table, S, heads, pos0=57, inverse=True)
    rel = float((z.double() - x.double()).norm() / x.double().norm())
    print("round trip relative L2 %.3g" % rel)
    assert rel <= math.sqrt(2.0) * 2.0 ** -8, rel


@gpu
def test_rope_kernel_adjoint():
    torch.manual_seed(5)
    B, S, heads = 2, 200, 5
    x = torch.randn(B * S, heads * 64)
    # g correlated with the rotated x, so that the inner product is not a near-cancelling sum
    g = (_rot64(x, S, heads, pos0=57).float() + torch.randn(B * S, heads * 64)).cuda()
    x = x.cuda()
    table = T.rope_table(512, device="cuda")
    rx = T.rope(x, torch.empty_like(x), table, S, heads, pos0=57)
    rg = T.rope(g, torch.empty_like(g), table, S, heads, pos0=57, inverse=True)
    lhs = float((rx.cpu().double() * g.cpu().double()).sum())
    rhs = float((x.cpu().double() * rg.cpu().double()).sum())
    print("adjoint: %.12g vs %.12g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@gpu
@pytest.mark.parametrize("m,n,t", [(5, 3, 100), (200, 17, 3000), (0, 383, 3700)])
def test_rope_kernel_scores_depend_on_relative_position(m, n, t):
    torch.manual_seed(6)
    rows, heads = 8, 2
    q, k = [torch.randn(rows, heads * 64, device="cuda") for _ in range(2)]
    table = T.rope_table(4096, device="cuda")

    def scores(pq, pk):
        rq = T.rope(q, torch.empty_like(q), table, 1, heads, pos0=pq).cpu().double()
        rk = T.rope(k, torch.empty_like(k), table, 1, heads, pos0=pk).cpu().double()
        return (rq * rk).reshape(rows, heads, 64).sum(-1)

    a, b = scores(m, n), scores(m + t, n + t)
    scale = (q.cpu().double().reshape(rows, heads, 64).norm(dim=-1)
             * k.cpu().double().reshape(rows, heads, 64).norm(dim=-1))
    worst = float(((a - b).abs() / scale).max())
    print("relative position: worst |diff| / (|q||k|) %.3g" % worst)
    assert worst <= 1e-5, worst
    assert float(((a - scores(m + 1, n)).abs() / scale).max()) > 1e-3  # and on nothing less


@gpu
def test_rope_kernel_refusals():
    """Host checks: every call returns hipErrorInvalidValue before any launch."""
    tokens, S, heads, rows = 400, 200, 5, 512
    x = torch.randn(tokens, 512, device="cuda").bfloat16()
    y = torch.zeros_like(x)
    before = x.clone()
    table = T.rope_table(rows, device="cuda")
    base = dict(x=x.data_ptr(), ldx=512, y=y.data_ptr(), ldy=512, dt=1, table=table.data_ptr(), rows=rows,
                tokens=tokens, S=S, heads=heads, pos0=0, inverse=0)

    def call(**kw):
        a = dict(base, **kw)
        T._lib.call("ttdk_rope", a["x"], a["ldx"], a["y"], a["ldy"], a["dt"], a["table"], a["rows"], a["tokens"],
                    a["S"], a["heads"], a["pos0"], a["inverse"], T._lib.stream())

    bad = [dict(heads=0), dict(heads=-1), dict(S=0), dict(tokens=-200), dict(tokens=399),
           dict(pos0=-1), dict(pos0=rows - S + 1), dict(rows=S - 1), dict(dt=2), dict(dt=-1),
           dict(ldx=heads * 64 - 8), dict(ldy=heads * 64 - 8),
           dict(x=x.data_ptr() + 2), dict(y=y.data_ptr() + 2),   # base pointer not a multiple of 16 bytes
           dict(ldx=heads * 64 + 4), dict(ldy=heads * 64 + 4),   # bf16 row stride % 8 != 0
           dict(table=None)]
    for kw in bad:
        with pytest.raises(T._lib.HipKernelError):
            call(**kw)
    call(tokens=0)  # nothing to do: no error, no launch
    with pytest.raises(T._lib.HipKernelError):  # the wrapper: mixed dtypes
        T.rope(x, y.float(), table, S, heads)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and float(y.float().abs().max()) == 0.0
    call()  # the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert float(y[:, :heads * 64].float().abs().max()) > 0


@gpu
def test_rope_kernel_in_hip_graph():
    torch.manual_seed(7)
    B, S, heads = 2, 200, 5
    x = torch.randn(B * S, heads * 64 + 64, device="cuda").bfloat16()
    out = torch.empty_like(x)
    table = T.rope_table(512, device="cuda")  # before the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.rope(x, out, table, S, heads, pos0=57)  # warm
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            T.rope(x, out, table, S, heads, pos0=57)
            with pytest.raises(RuntimeError):  # a table that is not cached yet: no copy inside a capture
                T.rope_table(512, base=1234.5, device="cuda")
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        x.copy_(torch.randn(x.shape, device="cuda").bfloat16())
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        eager = torch.full_like(out, -1.0)
        T.rope(x, eager, table, S, heads, pos0=57)
        assert torch.equal(_bits(out), _bits(eager))
        assert not torch.equal(out[:, :heads * 64], x[:, :heads * 64])


# ------------------------------------------------------------------ public surface on the GPU
@gpu
def test_nn_rotary_embedding_gpu_matches_cpu_path():
    torch.manual_seed(8)
    B, S, H = 2, 130, 3
    x = torch.randn(B, S, H * 64)
    g = torch.randn(B, S, H * 64)
    xc = x.clone().requires_grad_(True)
    yc = N.rotary_embedding(xc, H, offset=7)
    yc.backward(g)
    xg = x.cuda().requires_grad_(True)
    yg = N.rotary_embedding(xg, H, offset=7)
    yg.backward(g.cuda())
    assert yg.dtype == torch.float32 and yg.shape == x.shape
    torch.testing.assert_close(yg.detach().cpu(), yc.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(xg.grad.cpu(), xc.grad, atol=1e-5, rtol=1e-5)
    # a column slice of a wider projection goes in through its row stride
    wide = torch.randn(B, S, H * 64 + 128)
    ys = N.rotary_embedding(wide.cuda()[..., :H * 64], H, offset=7)
    torch.testing.assert_close(ys.cpu(), N.rotary_embedding(wide[..., :H * 64], H, offset=7), atol=1e-5, rtol=1e-5)
    yb = N.rotary_embedding(x.cuda().bfloat16(), H, offset=7)
    assert yb.dtype == torch.bfloat16
    torch.testing.assert_close(yb.float().cpu(), yc.detach(), atol=2e-2, rtol=2e-2)
    with pytest.raises(InvalidArgumentError):
        N.rotary_embedding(x.cuda(), 6)  # head_dim 32


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@gpu
def test_multi_head_attention_rotary_gpu_matches_cpu():
    """MultiHeadAttention(4, num_kv_heads=2, rotary=True) with a causal mask, at the bars and
    weights of test_attention_gqa.py's test_multi_head_attention_mqa_gpu_matches_cpu."""
    torch.manual_seed(6)
    L.reset_naming(0)
    B, S, D, H, Hk = 2, 128, 128, 4, 2
    inner, ikv = H * 64, Hk * 64
    x = torch.randn(B, S, D).bfloat16().float()
    dy = torch.randn(B, S, D)
    cpu = L.MultiHeadAttention(H, num_kv_heads=Hk, rotary=True)
    gpu_layer = L.MultiHeadAttention(H, num_kv_heads=Hk, rotary=True)
    with torch.no_grad():
        cpu(x)
        _set_weights(cpu, D, inner, ikv, 9)
        gpu_layer(x.cuda())
        gpu_layer.load_state_dict(cpu.state_dict())

    def run(layer, dev):
        xi = x.clone().to(dev).requires_grad_(True)
        y = layer(xi, use_causal_mask=True)
        y.backward(dy.to(dev))
        grads = {"x": xi.grad}
        for n, t in layer.named_variables():
            grads[n.split("/", 1)[1]] = t.grad
        return y.detach().cpu(), {n: g.cpu() for n, g in grads.items()}

    want, gw = run(cpu, "cpu")
    got, gg = run(gpu_layer, "cuda")
    print("max abs err", float((got - want).abs().max()), "rel L2", _rel(got, want))
    torch.testing.assert_close(got, want, atol=3e-2, rtol=3e-2)
    assert set(gg) == set(gw)
    rels = {n: _rel(gg[n], gw[n]) for n in gw}
    print("grad rel L2", rels)
    for n, rel in rels.items():
        assert rel < 2e-2, (n, rel)


def _small_cfg(**kw):
    return BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                      intermediate_size=1024, max_position_embeddings=256, **kw)


@gpu
def test_bert_engine_rotary_matches_reference():
    """The body and bars of test_attention_causal.py's test_bert_engine_causal_matches_reference
    with rotary embeddings in the engine and in the fp32 reference. One difference: under the
    rotation q.R.b_k varies over the keys, so the key/bias gradient is no longer exactly zero and
    is compared like every other tensor (measured relative error 0.013 in layer 1, 0.012 in
    layer 0, with |gradient| 3.1e-4 and 3.6e-4 beside a query/bias gradient of 4.1e-4 and 5.2e-4)."""
    torch.manual_seed(0)
    cfg = _small_cfg(causal=True, rotary=True)
    m = BertPretraining(cfg, device="cuda", seed=3, dropout=False)
    m.blaslt = 0
    batch = synthetic_batch(cfg, 2, 256, max_predictions=20, device="cuda", seed=1, full_length=False)
    sums = m.forward_backward(batch)
    torch.cuda.synchronize()
    P = m.params
    leaves = {n: P.c[n].float().detach().clone().requires_grad_(True) for n in P.names()}
    for n in P.names():  # fp32 params used directly by the kernels (biases, LayerNorm)
        if n.endswith("/bias") or "LayerNorm" in n or n.endswith("output_bias"):
            leaves[n] = P.var[n].detach().clone().requires_grad_(True)
    mlm, nsp = m.reference_loss(batch, leaves)
    assert abs(float(sums[0]) - float(mlm)) < 0.02 * float(mlm), (float(sums[0]), float(mlm.detach()))
    assert abs(float(sums[2]) - float(nsp)) < 0.02 * float(nsp) + 1e-3
    (mlm + nsp).backward()
    ge, gr = [], []
    bad = []
    for n in P.names():
        a = P.g[n].flatten()
        b = leaves[n].grad
        b = torch.zeros_like(a) if b is None else b.flatten()
        if "rows" in P.spec(n).meta:  # padded vocab rows: must be exactly zero
            rows = P.spec(n).meta["rows"]
            width = a.numel() // P.spec(n).shape[0]
            assert float(a[rows * width:].abs().sum()) == 0.0, n
        ge.append(a)
        gr.append(b)
        if b.norm() > 0:
            rel = float((a - b).norm() / b.norm())
            if n.endswith("key/bias"):
                qn = float(P.g[n.replace("key/bias", "query/bias")].norm())
                print("%s: relative error %.4f, |a - b| %.4g, |b| %.4g, |query/bias grad| %.4g"
                      % (n, rel, float((a - b).norm()), float(b.norm()), qn))
            if rel > 0.1:
                bad.append((n, rel))
    ge, gr = torch.cat(ge), torch.cat(gr)
    cos = float(torch.dot(ge, gr) / (ge.norm() * gr.norm()))
    assert cos > 0.99, (cos, bad[:10])
    assert not bad, bad[:10]


@gpu
def test_bert_engine_rotary_flag_is_live():
    """Dropout off: the rotary and the plain engine give different MLM losses on the same batch,
    and two rotary runs the same loss bit for bit.
    The batch has one predicted position per sequence, two in all. The engine adds each row's loss
    into the MLM sum with an fp32 atomic, in whatever order the rows' workgroups finish: a sum of
    two terms does not depend on that order (fp32 addition is commutative), a sum of more does
    (it is not associative). Measured with 20 predictions per sequence, five fresh engines each:
    the MLM loss took two values one ulp apart without rotary (7.0528598 / 7.0528593) and three
    with it (7.0528131 / 7.0528135 / 7.0528140), the two-row NSP loss one value in all ten runs.
    With two rows, bit equality tests the forward pass, the rotation included, and nothing else."""
    torch.manual_seed(0)
    batch = synthetic_batch(_small_cfg(), 2, 256, max_predictions=1, device="cuda", seed=1)

    def losses(rotary):
        m = BertPretraining(_small_cfg(rotary=rotary), device="cuda", seed=3, dropout=False)
        m.blaslt = 0
        s = m.forward_backward(batch)
        torch.cuda.synchronize()
        return float(s[0]), float(s[2])

    a, b, plain = losses(True), losses(True), losses(False)
    print("mlm / nsp loss: rotary %r, rotary again %r, plain %r" % (a, b, plain))
    assert a == b, (a, b)
    assert a[0] != plain[0], (a, plain)
