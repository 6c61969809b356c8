"""Causal (left-to-right) attention: the `causal` flag of the flash kernels, of `ttd.nn.attention`
(GPU kernels and CPU path), `layers.MultiHeadAttention(use_causal_mask=True)` and the BERT engine
(`BertConfig.causal`). The kernels are checked against the fp32 autograd oracle of
tests/attention_oracle.py with its triangular mask, and for exactness: a masked key
contributes exact zeros, so outputs and gradients of positions <= t do not change by one bit
when keys / values after t do."""
import pytest
import torch

from attention_oracle import ref as _ref, run_case
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.models.bert import BertConfig, BertPretraining, synthetic_batch
from tensorflow_train_distributed_amd.ops import transformer as T

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("masked", [False, True])
def test_nn_attention_causal_cpu_matches_masked_softmax(masked):
    torch.manual_seed(0)
    B, H, S = 2, 3, 128
    seqlen = torch.tensor([128, 70]) if masked else None
    q, k, v = [torch.randn(B, S, H * 64).requires_grad_(True) for _ in range(3)]
    o = N.attention(q, k, v, H, seqlen=seqlen, causal=True)
    do = torch.randn_like(o)
    o.backward(do)
    qr, kr, vr = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    ref = _ref(qr.view(B * S, -1), kr.view(B * S, -1), vr.view(B * S, -1), B, H, H, S, S, seqlen,
               True).view(B, S, -1)
    ref.backward(do)
    torch.testing.assert_close(o, ref, atol=1e-5, rtol=1e-5)
    for a, b in ((q, qr), (k, kr), (v, vr)):
        torch.testing.assert_close(a.grad, b.grad, atol=1e-5, rtol=1e-5)
    # and it is not the bidirectional result
    assert not torch.allclose(o, N.attention(q, k, v, H, seqlen=seqlen), atol=1e-3)


def test_multi_head_attention_use_causal_mask_cpu():
    torch.manual_seed(1)
    L.reset_naming(0)
    layer = L.MultiHeadAttention(2)
    x = torch.randn(2, 128, 96)
    t = 77
    x2 = x.clone()
    x2[:, t + 1:] = torch.randn(2, 128 - t - 1, 96)
    with torch.no_grad():
        a, b = layer(x, use_causal_mask=True), layer(x2, use_causal_mask=True)
        assert torch.equal(a[:, :t + 1], b[:, :t + 1])
        assert not torch.equal(a[:, t + 1:], b[:, t + 1:])
        c, d = layer(x), layer(x2)
        assert not torch.equal(c[:, :t + 1], d[:, :t + 1])


# ------------------------------------------------------------------ GPU kernels vs fp32 oracle
@gpu
@pytest.mark.parametrize("S,seqlen,p", [
    (128, None, 0.0),         # one block: diagonal tiles only
    (256, None, 0.1),         # + a full below-diagonal block, a skipped block, dropout
    (384, [384, 214], 0.1),   # odd block count; bwd_kv starts at tiles 0, 2, 4; len inside a diagonal tile
    (256, [256, 37], 0.0),    # len inside the first tile: query rows >= len see only keys < len
])
def test_causal_attention_fwd_bwd_matches_reference(S, seqlen, p):
    run_case(3, 3, S, S, True, seqlen, p, fused_layout=True)


@gpu
def test_causal_backward_ignores_fused_switch():
    """The fused single-kernel backward has no causal form: with the switch on, a causal
    backward still runs the split kernels and meets the same bars."""
    run_case(3, 3, 256, 256, True, None, 0.1, fused=True, fused_layout=True)


# ------------------------------------------------------------------ exactness on the GPU
@gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_attention_is_exact_about_later_keys(p):
    torch.manual_seed(3)
    B, H, S, t = 2, 3, 256, 150
    D = H * 64
    dev = "cuda"
    qkv = (torch.randn(B * S, 3 * D, device=dev) * 1.5).bfloat16()
    qkv2 = qkv.clone()
    late = (torch.arange(B * S, device=dev) % S) > t
    qkv2[late, D:] = (torch.randn(int(late.sum()), 2 * D, device=dev) * 1.5).bfloat16()
    rng = T.RngState(5, dev) if p > 0 else None
    do = torch.randn(B * S, D, device=dev).bfloat16()
    do[late] = 0

    def run(x, causal):
        q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:]
        o = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B * H, S, dtype=torch.float32, device=dev)
        T.attention_fwd(q, k, v, o, lse, B, H, S, p_drop=p, rng=rng, site=2, causal=causal)
        dx = torch.empty_like(x)
        T.attention_bwd(q, k, v, o, do, lse, dx[:, :D], dx[:, D:2 * D], dx[:, 2 * D:], B, H, S, p_drop=p, rng=rng,
                        site=2, causal=causal)
        return o, lse, dx

    early = ~late
    o1, l1, d1 = run(qkv, True)
    o2, l2, d2 = run(qkv2, True)
    assert torch.equal(o1[early], o2[early])
    assert torch.equal(l1[:, :t + 1], l2[:, :t + 1])
    assert not torch.equal(o1[late], o2[late])
    for d in (d1, d2):  # no query with a gradient attends keys > t
        assert float(d[late][:, D:].float().abs().max()) == 0.0
    assert torch.equal(d1[early][:, :D], d2[early][:, :D])
    assert float(d1[early][:, :D].float().abs().max()) > 0
    # the bidirectional kernels do see the later keys
    o3, l3, _ = run(qkv, False)
    o4, l4, _ = run(qkv2, False)
    assert not torch.equal(o3[early], o4[early])
    assert not torch.equal(l3[:, :t + 1], l4[:, :t + 1])


# ------------------------------------------------------------------ ttd.nn.attention on the GPU
@gpu
def test_nn_attention_causal_gpu_matches_cpu_path():
    torch.manual_seed(2)
    q = torch.randn(2, 128, 128)
    seqlen = torch.tensor([128, 70])
    qc = q.clone().requires_grad_(True)
    oc = N.attention(qc, qc, qc, 2, seqlen=seqlen, causal=True)
    oc.sum().backward()
    qg = q.cuda().requires_grad_(True)
    og = N.attention(qg, qg, qg, 2, seqlen=seqlen.cuda(), causal=True)
    og.sum().backward()
    assert float((og.detach().cpu() - oc.detach()).norm() / oc.detach().norm()) < 3e-2
    assert float((qg.grad.cpu() - qc.grad).norm() / qc.grad.norm()) < 3e-2


# ------------------------------------------------------------------ BERT engine
def _small_cfg(**kw):
    return BertConfig(vocab_size=1000, hidden_size=512, num_hidden_layers=2, num_attention_heads=8,
                      intermediate_size=1024, max_position_embeddings=256, **kw)


@gpu
@pytest.mark.parametrize("full_length", [True, False])
def test_bert_engine_causal_matches_reference(full_length):
    """tests/test_bert.py test_bert_engine_matches_reference's body (own GEMMs) with causal
    attention in the engine and the triangular mask in the fp32 reference."""
    torch.manual_seed(0)
    cfg = _small_cfg(causal=True)
    m = BertPretraining(cfg, device="cuda", seed=3, dropout=False)
    m.blaslt = 0
    batch = synthetic_batch(cfg, 2, 256, max_predictions=20, device="cuda", seed=1, full_length=full_length)
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


@gpu
def test_bert_engine_causal_flag_is_live():
    """Dropout off, every predicted position < 128: tokens at positions >= 128 cannot reach the
    causal engine's MLM loss (nor the NSP loss, pooled from position 0). fp32 summation order is
    the only freedom (1e-5); a leak through attention moves the loss orders of magnitude more,
    as the bidirectional engine shows."""
    torch.manual_seed(0)
    batch = synthetic_batch(_small_cfg(), 2, 256, max_predictions=20, device="cuda", seed=1)
    g = torch.Generator().manual_seed(7)
    batch.masked_lm_positions = torch.stack(
        [torch.randperm(127, generator=g)[:20] + 1 for _ in range(2)]).sort(1).values.to(torch.int32).cuda()
    ids2 = batch.input_ids.clone()
    ids2[:, 128:] = torch.randint(500, 1000, (2, 128), generator=g, dtype=torch.int32).cuda()
    assert not torch.equal(ids2, batch.input_ids)

    def losses(causal, ids):
        m = BertPretraining(_small_cfg(causal=causal), device="cuda", seed=3, dropout=False)
        m.blaslt = 0
        b = type(batch)(ids, batch.token_type_ids, batch.masked_lm_positions, batch.masked_lm_ids,
                        batch.next_sentence_labels, None)
        s = m.forward_backward(b)
        torch.cuda.synchronize()
        return float(s[0]), float(s[2])

    mlm_a, nsp_a = losses(True, batch.input_ids)
    mlm_b, nsp_b = losses(True, ids2)
    assert abs(mlm_a - mlm_b) <= 1e-5 * abs(mlm_a), (mlm_a, mlm_b)
    assert abs(nsp_a - nsp_b) <= 1e-5 * abs(nsp_a), (nsp_a, nsp_b)
    mlm_c, _ = losses(False, batch.input_ids)
    mlm_d, _ = losses(False, ids2)
    assert abs(mlm_c - mlm_d) > 1e-4 * abs(mlm_c), (mlm_c, mlm_d)
