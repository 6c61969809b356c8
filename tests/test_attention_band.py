"""Banded attention masks on the GPU: packed documents (segment ids), sliding windows, causal and
key length, folded into one table (ops.transformer.attention_band) and run by the BAND
instantiations of the flash kernels. Checked against tests/attention_oracle.py's fp32 oracle with
the explicit [S, S] mask of tests/band_oracle.py on top, at the suite's bars (o: atol = rtol = 3e-2;
lse: atol 2e-2, rtol 1e-3; dq / dk / dv: relative L2 < 2e-2). Rows that attend nothing are exact:
o == 0, lse == -inf, dq == dk == dv == 0."""
import math

import numpy as np
import pytest
import torch

import attention_oracle as O
import band_oracle as BO
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.models.bert import BertConfig, BertPretraining, synthetic_batch
from tensorflow_train_distributed_amd.ops import transformer as T
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

gpu = pytest.mark.gpu
B = 2

DOCS_384 = np.stack([BO.runs([70, 58, 128, 100], 384), BO.runs([1, 383], 384)])
DOCS_256 = np.stack([BO.runs([40, 100, 88], 256), BO.runs([130, 126], 256)])  # row 0 ends in 28 padding tokens

# id -> (H, Hk, S, segment ids, window, causal, seqlen, p, fused_layout)
CASES = {
    "documents": (3, 3, 384, DOCS_384, None, False, None, 0.0, False),
    "window-40-0-causal": (3, 3, 384, None, (40, 0), True, None, 0.0, False),
    "window-100-30": (3, 3, 384, None, (100, 30), False, None, 0.0, False),
    "window-none-30": (3, 3, 384, None, (None, 30), False, None, 0.0, False),
    "window-200-none": (3, 3, 384, None, (200, None), False, None, 0.0, False),
    "window-0-0": (3, 3, 384, None, (0, 0), False, None, 0.0, False),
    "all-grouped": (4, 2, 256, DOCS_256, (90, 0), True, [256, 150], 0.1, True),
    "all-self": (3, 3, 256, DOCS_256, (90, 0), True, [256, 150], 0.1, True),
}


def _inputs(H, Hk, S, fused_layout, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, Dk = H * 64, Hk * 64
    if fused_layout:
        qkv = (torch.randn(B * S, D + 2 * Dk, device="cuda", generator=g) * 1.5).bfloat16()
        q, k, v = qkv[:, :D], qkv[:, D:D + Dk], qkv[:, D + Dk:]
        dqkv = torch.empty_like(qkv)
        grads = dqkv[:, :D], dqkv[:, D:D + Dk], dqkv[:, D + Dk:]
    else:
        q = (torch.randn(B * S, D, device="cuda", generator=g) * 1.5).bfloat16()
        kv = (torch.randn(B * S, 2 * Dk, device="cuda", generator=g) * 1.5).bfloat16()
        k, v = kv[:, :Dk], kv[:, Dk:]
        dkv = torch.empty_like(kv)
        grads = torch.empty_like(q), dkv[:, :Dk], dkv[:, Dk:]
    do = torch.randn(B * S, D, device="cuda", generator=g).bfloat16()
    return q, k, v, do, grads


def _table(ids, window, causal, seqlen, S):
    ids_t = torch.from_numpy(ids).cuda() if ids is not None else None
    sl_t = torch.tensor(seqlen, dtype=torch.int32, device="cuda") if seqlen is not None else None
    return T.attention_band(ids_t, sl_t, window, causal, B, S)


def _run(cid, q, k, v, do, grads, band=None):
    """(o, lse, dq, dk, dv, rng) of a case through attention_fwd / attention_bwd(band=)."""
    H, Hk, S, ids, window, causal, seqlen, p, _ = CASES[cid]
    if band is None:
        band = _table(ids, window, causal, seqlen, S)
    rng = None
    if p > 0:
        rng = T.RngState(99, "cuda")
        rng.advance()
    o = torch.empty(B * S, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H, S, dtype=torch.float32, device="cuda")
    kw = dict(Hk=Hk, p_drop=p, rng=rng, site=5, band=band)
    T.attention_fwd(q, k, v, o, lse, B, H, S, **kw)
    dq, dk, dv = grads
    T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, S, **kw)
    return o, lse, dq, dk, dv, rng


_oracle_cache = {}


def _oracle(cid, q, k, v, do, rng):
    """fp32 (o, lse2, dq, dk, dv, mask) of the case, computed once per case and left unchanged."""
    if cid in _oracle_cache:
        return _oracle_cache[cid]
    H, Hk, S, ids, window, causal, seqlen, p, _ = CASES[cid]
    mask = torch.from_numpy(BO.brute_mask(ids, seqlen, window, causal, B, S)).cuda()
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    sc = O.scores(qf, kf, B, H, Hk, S, S, None, False).masked_fill(~mask[:, None], float("-inf"))
    lse = (torch.logsumexp(sc.detach(), -1) / math.log(2)).reshape(B * H, S)
    dead = ~mask.any(-1)[:, None, :, None]  # softmax over a row of -inf is NaN: zero rows instead
    pr = sc.masked_fill(dead, 0.0).softmax(-1).masked_fill(dead, 0.0)
    if p > 0:
        seed, step = rng.host()
        keep = torch.from_numpy(T.attention_keep_mask(seed, step, 5, p, B, H, S)).float().cuda()
        pr = pr * (keep * mask[:, None]) * T.attention_drop_scale(p)
    want = (pr @ O.heads(vf, B, S, Hk, H)).transpose(1, 2).reshape(B * S, H * 64)
    want.backward(do.float())
    _oracle_cache[cid] = (want.detach(), lse, qf.grad, kf.grad, vf.grad, mask)
    return _oracle_cache[cid]


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_band_kernels_match_the_oracle(cid):
    H, Hk, S, ids, window, causal, seqlen, p, fused_layout = CASES[cid]
    q, k, v, do, grads = _inputs(H, Hk, S, fused_layout)
    o, lse, dq, dk, dv, rng = _run(cid, q, k, v, do, grads)
    want, lse_ref, gq, gk, gv, mask = _oracle(cid, q, k, v, do, rng)
    print("o max abs err", float((o.float() - want).abs().max()))
    torch.testing.assert_close(o.float(), want, atol=3e-2, rtol=3e-2)
    dead_q = ~mask.any(-1).reshape(B * S)       # queries that attend nothing
    dead_k = ~mask.any(-2).reshape(B * S)       # keys nothing attends
    dead_l = dead_q.reshape(B, 1, S).expand(B, H, S).reshape(B * H, S)
    assert bool((lse[dead_l] == float("-inf")).all())
    print("lse max abs err", float((lse[~dead_l] - lse_ref[~dead_l]).abs().max()))
    torch.testing.assert_close(lse[~dead_l], lse_ref[~dead_l], atol=2e-2, rtol=1e-3)
    if ids is not None:
        assert bool(dead_q.any()) and bool(dead_k.any())
    if bool(dead_q.any()):  # exact, not small
        assert float(o[dead_q].float().abs().max()) == 0.0 and float(dq[dead_q].float().abs().max()) == 0.0
    if bool(dead_k.any()):
        assert float(dk[dead_k].float().abs().max()) == 0.0 and float(dv[dead_k].float().abs().max()) == 0.0
    if cid == "window-0-0":
        # each token attends itself: P = 1, o = v to bf16 rounding, lse = its own score, and
        # dS = P (dP - delta) = 0 up to the fp32 summation order of two 64-term dot products of
        # O(1) values (~64 * 2^-24 * sum|dO v| < 1e-4), times |k| / 8 < 1: dq, dk below 1e-3
        torch.testing.assert_close(o.float(), v.float(), atol=0.0, rtol=2.0 ** -7)  # two bf16 ulps
        own = (q.float() * k.float()).reshape(B, S, H, 64).sum(-1).permute(0, 2, 1).reshape(B * H, S) / 8.0
        torch.testing.assert_close(lse, own / math.log(2), atol=2e-2, rtol=1e-3)
        assert float(dq.float().abs().max()) < 1e-3 and float(dk.float().abs().max()) < 1e-3
        assert O.rel(dv, gv) < 2e-2
        return
    rels = [(n, O.rel(got, g)) for n, got, g in (("dq", dq, gq), ("dk", dk, gk), ("dv", dv, gv))]
    print("rel L2", rels)
    for n, r in rels:
        assert r < 2e-2, (n, r)


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_band_table_equals_host_mirror(cid):
    _, _, S, ids, window, causal, seqlen, _, _ = CASES[cid]
    got = _table(ids, window, causal, seqlen, S).cpu().numpy()
    sl = np.asarray(seqlen, dtype=np.int32) if seqlen is not None else None
    want = T.attention_band_host(ids, sl, window, causal, B, S)
    assert got.dtype == want.dtype and np.array_equal(got, want)


@gpu
def test_tiles_outside_the_band_are_not_read():
    """Four documents of 128 at S = 512: NaN in document 2's k / v (and, for the backward, its q /
    do / o) must not reach documents 0, 1 and 3 — a masked but streamed tile would turn 0 * NaN
    into NaN. The boundaries lie on 128 so that a correct kernel passes."""
    H, S = 2, 512
    ids = np.stack([BO.runs([128] * 4, S)] * B)
    band = T.attention_band(torch.from_numpy(ids).cuda(), None, None, False, B, S)
    q, k, v, do, _ = _inputs(H, H, S, False, seed=3)

    def run(q, k, v, do, o_in=None):
        o = torch.empty_like(q)
        lse = torch.empty(B * H, S, dtype=torch.float32, device="cuda")
        T.attention_fwd(q, k, v, o, lse, B, H, S, band=band)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        T.attention_bwd(q, k, v, o if o_in is None else o_in, do, lse, dq, dk, dv, B, H, S, band=band)
        return o, lse, dq, dk, dv

    first = run(q, k, v, do)
    doc2 = (torch.arange(B * S, device="cuda") % S) // 128 == 2
    nan = float("nan")
    q2, k2, v2, do2, o2 = [t.clone().contiguous() for t in (q, k, v, do, first[0])]
    for t in (q2, k2, v2, do2, o2):
        t[doc2] = nan
    again = run(q2, k2, v2, do2, o_in=o2)
    fwd_only = torch.empty_like(q)
    T.attention_fwd(q, k2, v2, fwd_only, torch.empty_like(first[1]), B, H, S, band=band)
    assert torch.equal(fwd_only[~doc2], first[0][~doc2])
    assert bool(torch.isnan(again[0][doc2].float()).all())  # the poison is live
    for name, a, b in zip(("o", "dq", "dk", "dv"), (first[0],) + first[2:], (again[0],) + again[2:]):
        assert torch.equal(a[~doc2], b[~doc2]), name
    keep_l = (~doc2).reshape(B, 1, S).expand(B, H, S).reshape(B * H, S)
    assert torch.equal(first[1][keep_l], again[1][keep_l])


@gpu
def test_band_same_bits_twice():
    cid = "all-grouped"
    H, Hk, S = CASES[cid][:3]
    q, k, v, do, grads = _inputs(H, Hk, S, True)
    one = [t.clone() for t in _run(cid, q, k, v, do, grads)[:5]]
    two = _run(cid, q, k, v, do, grads)[:5]
    for name, a, b in zip(O.OUTPUTS, one, two):
        assert torch.equal(a, b), name


@gpu
def test_band_table_forward_backward_in_one_graph():
    """attention_band, the forward and the backward captured in one graph (a single chain of
    kernels, no parallel branches), replayed, against the eager run bit for bit."""
    cid = "all-grouped"
    H, Hk, S, ids, window, causal, seqlen, p, _ = CASES[cid]
    q, k, v, do, grads = _inputs(H, Hk, S, True)
    eager = [t.clone() for t in _run(cid, q, k, v, do, grads)[:5]]
    ids_t = torch.from_numpy(ids).cuda()
    sl_t = torch.tensor(seqlen, dtype=torch.int32, device="cuda")
    band = torch.zeros(T.attention_band_ints(B, S), dtype=torch.int32, device="cuda")
    rng = T.RngState(99, "cuda")
    rng.advance()
    o = torch.zeros(B * S, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(B * H, S, dtype=torch.float32, device="cuda")
    delta = torch.zeros_like(lse)
    dq, dk, dv = grads
    for t in grads:
        t.zero_()
    kw = dict(Hk=Hk, p_drop=p, rng=rng, site=5, band=band)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.attention_band(ids_t, sl_t, window, causal, B, S, out=band)
        T.attention_fwd(q, k, v, o, lse, B, H, S, **kw)
        T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, S, delta=delta, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(O.OUTPUTS, eager, (o, lse, dq, dk, dv)):
        assert torch.equal(a, b), name


@gpu
def test_band_refusals():
    H, S = 2, 256
    q, k, v, do, _ = _inputs(H, H, S, False)
    o = torch.empty_like(q)
    lse = torch.empty(B * H, S, dtype=torch.float32, device="cuda")
    band = T.attention_band(None, None, (10, 10), False, B, S)
    kv = torch.empty(B * 128, H * 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(InvalidArgumentError):
        T.attention_fwd(q, kv, kv, o, lse, B, H, S, Sk=128, band=band)
    with pytest.raises(InvalidArgumentError):
        T.attention_bwd(q, kv, kv, o, do, lse, q, kv, kv, B, H, S, Sk=128, band=band)
    with pytest.raises(InvalidArgumentError):
        T.attention_band(None, None, (-3, 10), False, B, S)
    ids = torch.zeros(B, S, dtype=torch.int32, device="cuda")
    with pytest.raises(InvalidArgumentError):
        T.attention_band(ids[:, :128], None, None, False, B, S)
    with pytest.raises(InvalidArgumentError):
        T.attention_band(ids.long(), None, None, False, B, S)
    with pytest.raises(InvalidArgumentError):
        T.attention_fwd(q, k, v, o, lse, B, H, S, band=band[:100])


# ------------------------------------------------------------------ ttd.nn.attention, layers
@gpu
def test_nn_attention_band_gpu_matches_cpu_path():
    torch.manual_seed(2)
    S, H, Hk = 256, 4, 2
    q, k, v = torch.randn(B, S, H * 64), torch.randn(B, S, Hk * 64), torch.randn(B, S, Hk * 64)
    q, k, v = [t.bfloat16().float() for t in (q, k, v)]
    dy = torch.randn(B, S, H * 64).bfloat16().float()
    ids = torch.from_numpy(DOCS_256)

    def run(dev):
        leaves = [t.clone().to(dev).requires_grad_(True) for t in (q, k, v)]
        out = N.attention(*leaves, H, num_kv_heads=Hk, causal=True, segment_ids=ids.to(dev), window=(70, 0))
        out.backward(dy.to(dev))
        return [out.detach().cpu()] + [t.grad.cpu() for t in leaves]

    want, got = run("cpu"), run("cuda")
    torch.testing.assert_close(got[0], want[0], atol=3e-2, rtol=3e-2)
    pad = (ids < 0)
    assert bool(pad.any()) and float(got[0][pad].abs().max()) == 0.0
    for n, a, b in zip(("dq", "dk", "dv"), got[1:], want[1:]):
        assert O.rel(a, b) < 2e-2, (n, O.rel(a, b))
        assert float(a[pad].abs().max()) == 0.0, n


def _set_weights(layer, D, inner, ikv, seed):
    """O(1/sqrt(fan_in)) bf16-representable weights: q, k, v and the output are O(1)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        layer.qkv_kernel.copy_((torch.randn(D, inner + 2 * ikv, generator=g) / math.sqrt(D)).bfloat16().float())
        layer.qkv_bias.copy_((torch.randn(inner + 2 * ikv, generator=g) * 0.1).bfloat16().float())
        layer.out_kernel.copy_((torch.randn(inner, D, generator=g) / math.sqrt(inner)).bfloat16().float())
        layer.out_bias.copy_((torch.randn(D, generator=g) * 0.1).bfloat16().float())


@gpu
def test_multi_head_attention_band_gpu_matches_cpu():
    """MultiHeadAttention(4, num_kv_heads=2, rotary=True, window=(70, 0)) on packed documents with a
    causal mask, at the bars of the layer's rotary / grouped GPU-against-CPU tests."""
    torch.manual_seed(6)
    L.reset_naming(0)
    S, D, H, Hk = 256, 128, 4, 2
    inner, ikv = H * 64, Hk * 64
    x = torch.randn(B, S, D).bfloat16().float()
    dy = torch.randn(B, S, D)
    ids = torch.from_numpy(np.stack([BO.runs([100, 156], S), BO.runs([256], S)]))
    cpu = L.MultiHeadAttention(H, num_kv_heads=Hk, rotary=True, window=(70, 0))
    gpu_layer = L.MultiHeadAttention(H, num_kv_heads=Hk, rotary=True, window=(70, 0))
    with torch.no_grad():
        cpu(x)
        _set_weights(cpu, D, inner, ikv, 9)
        gpu_layer(x.cuda())
        gpu_layer.load_state_dict(cpu.state_dict())

    def run(layer, dev):
        xi = x.clone().to(dev).requires_grad_(True)
        y = layer(xi, use_causal_mask=True, segment_ids=ids.to(dev))
        y.backward(dy.to(dev))
        grads = {"x": xi.grad}
        for n, t in layer.named_variables():
            grads[n.split("/", 1)[1]] = t.grad
        return y.detach().cpu(), {n: g.cpu() for n, g in grads.items()}

    want, gw = run(cpu, "cpu")
    got, gg = run(gpu_layer, "cuda")
    torch.testing.assert_close(got, want, atol=3e-2, rtol=3e-2)
    assert set(gg) == set(gw)
    for n in gw:
        assert O.rel(gg[n], gw[n]) < 2e-2, (n, O.rel(gg[n], gw[n]))


# ------------------------------------------------------------------ BERT engine
def _small_cfg(**kw):
    return BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                      intermediate_size=1024, max_position_embeddings=256, **kw)


@gpu
@pytest.mark.parametrize("causal", [False, True])
def test_bert_engine_attention_window_matches_reference(causal):
    """The body and bars of test_attention_causal.py's test_bert_engine_causal_matches_reference with
    attention_window=(40, 40) in the engine and the same mask in the fp32 reference; padded
    sequences, so the window also meets seqlen."""
    torch.manual_seed(0)
    cfg = _small_cfg(attention_window=(40, 40), causal=causal)
    m = BertPretraining(cfg, device="cuda", seed=3, dropout=False)
    m.blaslt = 0
    batch = synthetic_batch(cfg, 2, 256, max_predictions=20, device="cuda", seed=1, full_length=False)
    sums = m.forward_backward(batch)
    torch.cuda.synchronize()
    P = m.params
    plain = BertPretraining(_small_cfg(causal=causal), device="cuda", seed=3, dropout=False)
    assert P.names() == plain.params.names()  # the parameter set does not change
    leaves = {n: P.c[n].float().detach().clone().requires_grad_(True) for n in P.names()}
    for n in P.names():  # fp32 params used directly by the kernels (biases, LayerNorm)
        if n.endswith("/bias") or "LayerNorm" in n or n.endswith("output_bias"):
            leaves[n] = P.var[n].detach().clone().requires_grad_(True)
    mlm, nsp = m.reference_loss(batch, leaves)
    assert abs(float(sums[0]) - float(mlm)) < 0.02 * float(mlm), (float(sums[0]), float(mlm.detach()))
    assert abs(float(sums[2]) - float(nsp)) < 0.02 * float(nsp) + 1e-3
    (mlm + nsp).backward()
    ge, gr, bad = [], [], []
    for n in P.names():
        a = P.g[n].flatten()
        b = leaves[n].grad
        b = torch.zeros_like(a) if b is None else b.flatten()
        ge.append(a)
        gr.append(b)
        if n.endswith("key/bias"):
            # softmax is invariant to q.b_k (constant over keys): the exact gradient is 0
            qn = float(P.g[n.replace("key/bias", "query/bias")].norm())
            assert float(a.norm()) < 0.05 * qn, (n, float(a.norm()), qn)
        elif b.norm() > 0:
            rel = float((a - b).norm() / b.norm())
            if rel > 0.1:
                bad.append((n, rel))
    ge, gr = torch.cat(ge), torch.cat(gr)
    cos = float(torch.dot(ge, gr) / (ge.norm() * gr.norm()))
    assert cos > 0.99, (cos, bad[:10])
    assert not bad, bad[:10]
    # the flag is live: the full-attention engine gives another loss on the same batch
    plain.blaslt = 0
    assert abs(float(plain.forward_backward(batch)[0]) - float(sums[0])) > 1e-4
