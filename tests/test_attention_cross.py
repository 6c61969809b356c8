"""Cross-attention: a key length `Sk` apart from the query length in the flash kernels
(`ttdk_attn_fwd` / `ttdk_attn_bwd` with Sk != Sq), `ops.transformer.attention_fwd / _bwd(Sk=)`,
`attention_keep_mask(Sk=)`, `ttd.nn.attention` with k / v of another length (GPU kernels and CPU
path) and `layers.MultiHeadAttention(x, value=mem)`.

The kernels are checked against the fp32 autograd oracle of tests/attention_oracle.py with
separate query and key lengths, at its bars (o: atol = rtol = 3e-2; lse: atol 2e-2, rtol
1e-3; dq / dk / dv: relative L2 error < 2e-2), and for exactness: keys past the memory's length
add exact zeros, query blocks do not see each other, and the general argument list at Sk == S
gives the self-attention bits."""
import math

import pytest
import torch

from attention_oracle import assert_explicit_entry_is_self_attention, ref as _ref, rel as _rel, run_case
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import transformer as T
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("Sq,Sk,seqlen", [(40, 72, None), (72, 40, [40, 23]), (128, 256, [256, 70])])
def test_nn_attention_cross_cpu_matches_masked_softmax(Sq, Sk, seqlen):
    torch.manual_seed(0)
    B, H = 2, 3
    seqlen = torch.tensor(seqlen) if seqlen is not None else None
    q = torch.randn(B, Sq, H * 64).requires_grad_(True)
    k, v = [torch.randn(B, Sk, H * 64).requires_grad_(True) for _ in range(2)]
    o = N.attention(q, k, v, H, seqlen=seqlen)
    assert o.shape == (B, Sq, H * 64)
    do = torch.randn_like(o)
    o.backward(do)
    qr, kr, vr = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    ref = _ref(qr.view(B * Sq, -1), kr.view(B * Sk, -1), vr.view(B * Sk, -1), B, H, H, Sq, Sk, seqlen).view(B, Sq, -1)
    ref.backward(do)
    torch.testing.assert_close(o, ref, atol=1e-5, rtol=1e-5)
    assert k.grad.shape == (B, Sk, H * 64) and v.grad.shape == (B, Sk, H * 64)
    for a, b in ((q, qr), (k, kr), (v, vr)):
        torch.testing.assert_close(a.grad, b.grad, atol=1e-5, rtol=1e-5)
    if seqlen is not None:  # masked keys get no gradient
        n = int(seqlen[1])
        assert float(k.grad[1, n:].abs().max()) == 0.0 and float(v.grad[1, n:].abs().max()) == 0.0


def test_attention_keep_mask_key_length():
    B, H = 2, 3
    wide = T.attention_keep_mask(7, 3, 5, 0.1, B, H, 128, Sk=256)
    assert wide.shape == (B, H, 128, 256)
    square = T.attention_keep_mask(7, 3, 5, 0.1, B, H, 128, Sk=128)
    assert (wide[..., :128] == square).all()
    assert (square == T.attention_keep_mask(7, 3, 5, 0.1, B, H, 128)).all()
    assert 0.85 < wide[..., 128:].mean() < 0.95  # the new columns are a mask of their own, not a constant
    tall = T.attention_keep_mask(7, 3, 5, 0.1, B, H, 256, Sk=128)
    assert tall.shape == (B, H, 256, 128)
    assert (tall == T.attention_keep_mask(7, 3, 5, 0.1, B, H, 256)[..., :128]).all()


def test_nn_attention_causal_cross_raises_cpu():
    q, m = torch.randn(2, 128, 128), torch.randn(2, 256, 128)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, m, m, 2, causal=True)
    N.attention(q, q, q, 2, causal=True)  # Sk == S stays allowed


def test_multi_head_attention_value_cpu():
    torch.manual_seed(1)
    L.reset_naming(0)
    B, S, Sk, D, H = 2, 24, 40, 96, 2
    inner = H * 64
    x, mem = torch.randn(B, S, D), torch.randn(B, Sk, D)
    seqlen = torch.tensor([40, 17])
    self_layer = L.MultiHeadAttention(H)
    with torch.no_grad():
        self_layer(x)
    self_names = {n.split("/", 1)[1] for n, _ in self_layer.named_variables()}
    layer = L.MultiHeadAttention(H)
    with torch.no_grad():
        y = layer(x, value=mem, seqlen=seqlen)
        assert {n.split("/", 1)[1] for n, _ in layer.named_variables()} == self_names
        assert len(layer.variables) == len(self_layer.variables) == 4
        # non-trivial biases, so the bias split is checked too
        layer.qkv_bias.copy_(torch.randn(3 * inner) * 0.1)
        layer.out_bias.copy_(torch.randn(D) * 0.1)
        y = layer(x, value=mem, seqlen=seqlen)
        W, b = layer.qkv_kernel, layer.qkv_bias
        q = x @ W[:, :inner] + b[:inner]
        k = mem @ W[:, inner:2 * inner] + b[inner:2 * inner]
        v = mem @ W[:, 2 * inner:] + b[2 * inner:]
        a = _ref(q.reshape(B * S, inner), k.reshape(B * Sk, inner), v.reshape(B * Sk, inner), B, H, H, S, Sk, seqlen)
        want = a.view(B, S, inner) @ layer.out_kernel + layer.out_bias
        assert y.shape == (B, S, D)
        torch.testing.assert_close(y, want, atol=1e-5, rtol=1e-4)
        # value = x is self-attention through the split projections
        torch.testing.assert_close(layer(x, value=x), layer(x), atol=1e-5, rtol=1e-4)
        with pytest.raises(InvalidArgumentError):
            layer(x, value=torch.randn(B, Sk, D + 32))


# ------------------------------------------------------------------ GPU kernels vs fp32 oracle
@gpu
@pytest.mark.parametrize("Sq,Sk,seqlen,p", [
    (128, 256, None, 0.0),          # more key blocks than query blocks: bwd_kv's grid is the larger
    (256, 128, None, 0.1),          # more query blocks: lse / delta / hash rows stride by Sq, not Sk
    (128, 384, [384, 70], 0.1),     # odd key-block count, len inside a tile; whole key blocks past len
    (384, 128, [37, 128], 0.0),     # odd query-block count; len inside the first tile
])
def test_cross_attention_fwd_bwd_matches_reference(Sq, Sk, seqlen, p):
    run_case(3, 3, Sq, Sk, False, seqlen, p)


@gpu
def test_cross_backward_ignores_fused_switch():
    """The fused single-kernel backward is a self-attention kernel: with the switch on, a backward
    with Sq != Sk still runs the split kernels and meets the same bars."""
    run_case(3, 3, 256, 128, False, None, 0.1, fused=True)


# ------------------------------------------------------------------ exactness on the GPU
def _run(q, k, v, do, B, H, Sq, Sk, *, seqlen=None, p=0.0, rng=None, site=2, cross=True):
    """Forward + split backward into fresh buffers; cross=False goes through the call without Sk
    (the wrapper fills in Sk = Sq)."""
    D = H * 64
    dev = q.device
    o = torch.empty(B * Sq, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H, Sq, dtype=torch.float32, device=dev)
    dq = torch.empty(B * Sq, D, dtype=torch.bfloat16, device=dev)
    dk = torch.empty(B * Sk, D, dtype=torch.bfloat16, device=dev)
    dv = torch.empty(B * Sk, D, dtype=torch.bfloat16, device=dev)
    kw = dict(seqlen=seqlen, p_drop=p, rng=rng, site=site)
    if cross:
        kw["Sk"] = Sk
    T.attention_fwd(q, k, v, o, lse, B, H, Sq, **kw)
    T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, Sq, **kw)
    return o, lse, dq, dk, dv


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_keys_past_len_add_nothing(p):
    torch.manual_seed(3)
    B, H, S = 2, 3, 128
    D = H * 64
    dev = "cuda"
    q, ka, va, do = [(torch.randn(B * S, D, device=dev) * 1.5).bfloat16() for _ in range(4)]
    kb, vb = [(torch.randn(B, 2 * S, D, device=dev) * 1.5).bfloat16() for _ in range(2)]
    kb[:, :S] = ka.view(B, S, D)
    vb[:, :S] = va.view(B, S, D)
    kb, vb = kb.view(B * 2 * S, D), vb.view(B * 2 * S, D)
    rng = T.RngState(5, dev) if p > 0 else None
    seqlen = torch.tensor([S, S], dtype=torch.int32, device=dev)
    oa, la, dqa, dka, dva = _run(q, ka, va, do, B, H, S, S, p=p, rng=rng, cross=False)
    ob, lb, dqb, dkb, dvb = _run(q, kb, vb, do, B, H, S, 2 * S, seqlen=seqlen, p=p, rng=rng)
    assert torch.equal(oa, ob) and torch.equal(la, lb) and torch.equal(dqa, dqb)
    assert float(dqa.float().abs().max()) > 0
    dkb, dvb = dkb.view(B, 2 * S, D), dvb.view(B, 2 * S, D)
    assert torch.equal(dka.view(B, S, D), dkb[:, :S]) and torch.equal(dva.view(B, S, D), dvb[:, :S])
    assert float(dkb[:, S:].float().abs().max()) == 0.0 and float(dvb[:, S:].float().abs().max()) == 0.0
    # without the length the extra keys are seen
    oc = _run(q, kb, vb, do, B, H, S, 2 * S, p=p, rng=rng)[0]
    assert not torch.equal(oa, oc)


@gpu
def test_query_blocks_are_independent():
    torch.manual_seed(4)
    B, H, Sq, Sk = 2, 3, 256, 128
    D = H * 64
    dev = "cuda"
    q, do = [(torch.randn(B * Sq, D, device=dev) * 1.5).bfloat16() for _ in range(2)]
    k, v = [(torch.randn(B * Sk, D, device=dev) * 1.5).bfloat16() for _ in range(2)]
    o, lse, dq, _, _ = _run(q, k, v, do, B, H, Sq, Sk)
    second = (torch.arange(B * Sq, device=dev) % Sq) >= 128
    o2, lse2, dq2, _, _ = _run(q[second].contiguous(), k, v, do[second].contiguous(), B, H, 128, Sk)
    assert torch.equal(o[second], o2)
    assert torch.equal(lse[:, 128:], lse2)
    assert torch.equal(dq[second], dq2)
    assert not torch.equal(o[~second], o2)


@gpu
def test_cross_entry_equals_self_entry_at_equal_lengths():
    """One entry pair takes Sq and Sk, so there is no second symbol to compare with: the general
    argument list at Sk == Sq must give the bits of the wrapper call without Sk, and the bits the
    self-attention entry points gave before the merge (tests/golden/attention_parent_bits.json)."""
    for cid in ("self-p0.1-full", "self-p0.1-causal"):
        assert_explicit_entry_is_self_attention(cid)


@gpu
def test_cross_entries_refuse_bad_lengths():
    B, H = 2, 3
    D = H * 64
    dev = "cuda"
    x = torch.zeros(B * 256, D, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(B * H, 256, dtype=torch.float32, device=dev)
    for Sq, Sk, causal in ((100, 128, False), (128, 100, False), (128, 256, True)):
        with pytest.raises(T._lib.HipKernelError):
            T.attention_fwd(x, x, x, x.clone(), lse, B, H, Sq, Sk=Sk, causal=causal)
        with pytest.raises(T._lib.HipKernelError):
            T.attention_bwd(x, x, x, x, x, lse, x.clone(), x.clone(), x.clone(), B, H, Sq, Sk=Sk, causal=causal)


# ------------------------------------------------------------------ public surface on the GPU
@gpu
def test_nn_attention_cross_gpu_matches_cpu_path():
    """fp32 tensors holding bf16-representable values, so both paths start from the same numbers
    (the kernels compute in bf16 by design)."""
    torch.manual_seed(2)
    B, H, S, Sk = 2, 3, 128, 256
    q = torch.randn(B, S, H * 64).bfloat16().float()
    k, v = [torch.randn(B, Sk, H * 64).bfloat16().float() for _ in range(2)]
    do = torch.randn(B, S, H * 64).bfloat16().float()
    seqlen = torch.tensor([256, 70])
    cpu = [t.clone().requires_grad_(True) for t in (q, k, v)]
    oc = N.attention(*cpu, H, seqlen=seqlen)
    oc.backward(do)
    dev = [t.cuda().requires_grad_(True) for t in (q, k, v)]
    og = N.attention(*dev, H, seqlen=seqlen.cuda())
    og.backward(do.cuda())
    assert og.shape == (B, S, H * 64) and dev[1].grad.shape == (B, Sk, H * 64)
    torch.testing.assert_close(og.detach().cpu(), oc.detach(), atol=3e-2, rtol=3e-2)
    for name, g, c in zip("qkv", dev, cpu):
        rel = _rel(g.grad.cpu(), c.grad)
        print("d" + name, rel)
        assert rel < 2e-2, (name, rel)


@gpu
def test_nn_attention_cross_gpu_refusals():
    q = torch.randn(2, 128, 128, device="cuda")
    with pytest.raises(InvalidArgumentError):
        N.attention(q, torch.randn(2, 100, 128, device="cuda"), torch.randn(2, 100, 128, device="cuda"), 2)
    m = torch.randn(2, 256, 128, device="cuda")
    with pytest.raises(InvalidArgumentError):
        N.attention(q, m, m, 2, causal=True)


@gpu
def test_multi_head_attention_value_gpu_matches_cpu():
    """Weights of O(1/sqrt(fan_in)) so that q, k, v and the output are O(1), the scale the output
    bar (atol = rtol = 3e-2) was set for."""
    torch.manual_seed(6)
    L.reset_naming(0)
    B, S, Sk, D, H = 2, 128, 256, 128, 2
    inner = H * 64
    x = torch.randn(B, S, D).bfloat16().float()
    mem = torch.randn(B, Sk, D).bfloat16().float()
    seqlen = torch.tensor([256, 101])
    cpu = L.MultiHeadAttention(H)
    gpu_layer = L.MultiHeadAttention(H)
    with torch.no_grad():
        cpu(x, value=mem)
        cpu.qkv_kernel.copy_((torch.randn(D, 3 * inner) / math.sqrt(D)).bfloat16().float())
        cpu.qkv_bias.copy_((torch.randn(3 * inner) * 0.1).bfloat16().float())
        cpu.out_kernel.copy_((torch.randn(inner, D) / math.sqrt(inner)).bfloat16().float())
        cpu.out_bias.copy_((torch.randn(D) * 0.1).bfloat16().float())
        want = cpu(x, value=mem, seqlen=seqlen)
        gpu_layer(x.cuda(), value=mem.cuda())
        gpu_layer.load_state_dict(cpu.state_dict())
        got = gpu_layer(x.cuda(), value=mem.cuda(), seqlen=seqlen.cuda())
    assert got.is_cuda and got.shape == (B, S, D)
    print("max abs err", float((got.cpu() - want).abs().max()), "rel L2", _rel(got.cpu(), want))
    torch.testing.assert_close(got.cpu(), want, atol=3e-2, rtol=3e-2)
