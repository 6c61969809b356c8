"""Grouped-query attention (GQA; one key/value head: multi-query attention): H query heads over
Hk < H key/value heads in the flash kernels (`ttdk_attn_fwd` / `ttdk_attn_bwd` with Hk != H),
`ops.transformer.attention_fwd / _bwd(Hk=)`, `ttd.nn.attention(num_kv_heads=)` (GPU kernels and
CPU path) and `layers.MultiHeadAttention(num_kv_heads=)`. Query head h uses key/value head
h // (H // Hk): the layout of `repeat_interleave` over the head axis.

The kernels are checked against the fp32 autograd oracle of tests/attention_oracle.py, which
repeats the key/value heads explicitly, at its bars
(o: atol = rtol = 3e-2; lse: atol 2e-2, rtol 1e-3; dq / dk / dv: relative L2 error < 2e-2), and
for exactness: o, lse and dq equal a self-attention run over repeated heads bit for bit, the
general argument list at Hk == H gives the self-attention bits, groups do not see each other, and
dk / dv (summed over a group's heads in registers, in head order) are deterministic."""
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
@pytest.mark.parametrize("H,Hk,S,Sk,seqlen,causal", [
    (4, 2, 40, 40, None, False),
    (6, 2, 72, 72, [72, 23], False),
    (4, 1, 40, 40, None, True),
    (6, 2, 40, 40, [40, 17], True),
    (4, 1, 72, 72, [33, 72], False),
    (4, 2, 40, 72, [72, 40], False),   # Sk != S
])
def test_nn_attention_gqa_cpu_matches_masked_softmax(H, Hk, S, Sk, seqlen, causal):
    torch.manual_seed(0)
    B = 2
    seqlen = torch.tensor(seqlen) if seqlen is not None else None
    q = torch.randn(B, S, H * 64).requires_grad_(True)
    k, v = [torch.randn(B, Sk, Hk * 64).requires_grad_(True) for _ in range(2)]
    o = N.attention(q, k, v, H, seqlen=seqlen, causal=causal, num_kv_heads=Hk)
    assert o.shape == (B, S, H * 64)
    do = torch.randn_like(o)
    o.backward(do)
    qr, kr, vr = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    ref = _ref(qr.view(B * S, -1), kr.view(B * Sk, -1), vr.view(B * Sk, -1), B, H, Hk, S, Sk, seqlen,
               causal).view(B, S, -1)
    ref.backward(do)
    torch.testing.assert_close(o, ref, atol=1e-5, rtol=1e-5)
    assert k.grad.shape == (B, Sk, Hk * 64) and v.grad.shape == (B, Sk, Hk * 64)
    for a, b in ((q, qr), (k, kr), (v, vr)):
        torch.testing.assert_close(a.grad, b.grad, atol=1e-5, rtol=1e-5)
    if seqlen is not None:  # masked keys get no gradient
        for b in range(B):
            n = int(seqlen[b])
            if n < Sk:
                assert float(k.grad[b, n:].abs().max()) == 0.0 and float(v.grad[b, n:].abs().max()) == 0.0
        assert int(seqlen.min()) < Sk


def test_nn_attention_gqa_refusals_and_default_cpu():
    torch.manual_seed(1)
    B, S, H = 2, 24, 4
    q = torch.randn(B, S, H * 64)
    kv2 = torch.randn(B, S, 2 * 64)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, torch.randn(B, S, 3 * 64), torch.randn(B, S, 3 * 64), 4, num_kv_heads=3)
    with pytest.raises(InvalidArgumentError):  # k / v as wide as q, two key/value heads asked for
        N.attention(q, q, q, 4, num_kv_heads=2)
    with pytest.raises(InvalidArgumentError):  # v of another width than k
        N.attention(q, kv2, q, 4, num_kv_heads=2)
    with pytest.raises(InvalidArgumentError):  # grouped k / v without saying so
        N.attention(q, kv2, kv2, 4)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, kv2, kv2, 4, num_kv_heads=0)
    old = N.attention(q, q, q, 4)
    assert torch.equal(N.attention(q, q, q, 4, num_kv_heads=None), old)
    assert torch.equal(N.attention(q, q, q, 4, num_kv_heads=4), old)


def test_multi_head_attention_num_kv_heads_cpu():
    torch.manual_seed(2)
    L.reset_naming(0)
    B, S, Sk, D, H, Hk = 2, 24, 40, 96, 4, 2
    inner, ikv = H * 64, Hk * 64
    x, mem = torch.randn(B, S, D), torch.randn(B, Sk, D)
    seqlen = torch.tensor([40, 17])
    default = L.MultiHeadAttention(H)
    layer = L.MultiHeadAttention(H, num_kv_heads=Hk)
    with torch.no_grad():
        default(x)
        layer(x)

        def shapes(l):
            return {n.split("/", 1)[1]: tuple(t.shape) for n, t in l.named_variables()}

        assert shapes(default) == {"qkv/kernel": (D, 3 * inner), "qkv/bias": (3 * inner,),
                                   "output/kernel": (inner, D), "output/bias": (D,)}
        assert shapes(layer) == {"qkv/kernel": (D, inner + 2 * ikv), "qkv/bias": (inner + 2 * ikv,),
                                 "output/kernel": (inner, D), "output/bias": (D,)}
        assert len(layer.variables) == len(default.variables) == 4
        # non-trivial biases, so the bias split is checked too
        layer.qkv_bias.copy_(torch.randn(inner + 2 * ikv) * 0.1)
        layer.out_bias.copy_(torch.randn(D) * 0.1)
        W, b = layer.qkv_kernel, layer.qkv_bias

        def by_hand(src, Sm, **kw):
            q = x @ W[:, :inner] + b[:inner]
            k = src @ W[:, inner:inner + ikv] + b[inner:inner + ikv]
            v = src @ W[:, inner + ikv:] + b[inner + ikv:]
            assert k.shape == (B, Sm, ikv)
            a = N.attention(q, k, v, H, num_kv_heads=Hk, **kw)
            return a @ layer.out_kernel + layer.out_bias

        torch.testing.assert_close(layer(x), by_hand(x, S), atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(layer(x, use_causal_mask=True), by_hand(x, S, causal=True), atol=1e-5, rtol=1e-4)
        y = layer(x, value=mem, seqlen=seqlen)
        assert y.shape == (B, S, D)
        torch.testing.assert_close(y, by_hand(mem, Sk, seqlen=seqlen), atol=1e-5, rtol=1e-4)
        assert not torch.allclose(y, layer(x, value=mem), atol=1e-3)
    with pytest.raises(InvalidArgumentError):
        L.MultiHeadAttention(4, num_kv_heads=3)


# ------------------------------------------------------------------ GPU kernels vs fp32 oracle
@gpu
@pytest.mark.parametrize("H,Hk,Sq,Sk,causal,seqlen,p", [
    # two groups; two query blocks, so a group's second head reads lse / delta rows at another bh*S
    (4, 2, 256, 256, False, None, 0.0),
    # G = 3 (odd, more than one two-tile trip per head); cross lengths; whole key blocks past len
    (6, 2, 128, 384, False, [384, 70], 0.1),
    # MQA; the diagonal trip restarts for each of 4 heads; odd block count
    (4, 1, 384, 384, True, [384, 150], 0.1),
    # causal without dropout
    (4, 2, 256, 256, True, None, 0.0),
])
def test_gqa_fwd_bwd_matches_reference(H, Hk, Sq, Sk, causal, seqlen, p):
    run_case(H, Hk, Sq, Sk, causal, seqlen, p)


@gpu
def test_gqa_backward_ignores_fused_switch():
    """The fused single-kernel backward is an Hk == H kernel: with the switch on, a grouped
    backward still runs the split kernels and meets the same bars."""
    run_case(4, 2, 256, 256, False, None, 0.1, fused=True)


# ------------------------------------------------------------------ exactness on the GPU
def _run(q, k, v, do, B, H, S, *, Hk=None, seqlen=None, p=0.0, rng=None, site=2, causal=False):
    """Forward + split backward into fresh buffers; Hk=None goes through the call without Hk (the
    wrapper fills in Hk = H)."""
    dev = q.device
    o = torch.empty(B * S, H * 64, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H, S, dtype=torch.float32, device=dev)
    dq = torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    kw = dict(seqlen=seqlen, p_drop=p, rng=rng, site=site, causal=causal)
    if Hk is not None:
        kw["Hk"] = Hk
    T.attention_fwd(q, k, v, o, lse, B, H, S, **kw)
    T.attention_bwd(q, k, v, o, do, lse, dq, dk, dv, B, H, S, **kw)
    return o, lse, dq, dk, dv


def _repeat(t, Hk, G):
    """Token-major [rows, Hk*64] -> [rows, Hk*G*64], head j of the result = head j // G of t."""
    return t.view(-1, Hk, 1, 64).expand(-1, Hk, G, 64).reshape(-1, Hk * G * 64).contiguous()


@gpu
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_equals_repeated_heads_bitwise(causal):
    """The per-head arithmetic and the dropout hash (row id (b*H + h)*S + q) do not depend on where
    K and V come from: o, lse and dq equal the self-attention entry's over repeated heads. (dk / dv
    are not compared: the repeated run rounds each head to bf16 before the sum.)"""
    torch.manual_seed(7)
    B, H, Hk, S, p = 2, 4, 2, 256, 0.1
    dev = "cuda"
    q, do = [(torch.randn(B * S, H * 64, device=dev) * 1.5).bfloat16() for _ in range(2)]
    k, v = [(torch.randn(B * S, Hk * 64, device=dev) * 1.5).bfloat16() for _ in range(2)]
    rng = T.RngState(13, dev)
    seqlen = torch.tensor([S, 150], dtype=torch.int32, device=dev)
    o, lse, dq, dk, dv = _run(q, k, v, do, B, H, S, Hk=Hk, seqlen=seqlen, p=p, rng=rng, causal=causal)
    kr, vr = _repeat(k, Hk, H // Hk), _repeat(v, Hk, H // Hk)
    assert torch.equal(kr[:, 64:128], k[:, :64]) and torch.equal(kr[:, 128:192], k[:, 64:])
    o2, lse2, dq2, dk2, dv2 = _run(q, kr, vr, do, B, H, S, seqlen=seqlen, p=p, rng=rng, causal=causal)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(dq, dq2)
    assert float(dq.float().abs().max()) > 0
    # the group sums agree with the bf16-rounded per-head results to their rounding
    for name, got, rep in (("dk", dk, dk2), ("dv", dv, dv2)):
        want = rep.float().view(-1, Hk, H // Hk, 64).sum(2).reshape(-1, Hk * 64)
        rel = _rel(got, want)
        print(name, "vs summed repeated run: rel L2", rel)
        assert rel < 2e-2, (name, rel)


@gpu
def test_gqa_entry_equals_self_entry_at_equal_heads():
    """One entry pair takes Hk, so there is no second symbol to compare with: the general argument
    list at Hk == H must give the bits of the wrapper call without Hk, and the bits the
    self-attention entry points gave before the merge (tests/golden/attention_parent_bits.json)."""
    for cid in ("self-p0.1-full", "self-p0.1-causal"):
        assert_explicit_entry_is_self_attention(cid)


@gpu
def test_gqa_groups_are_independent_and_deterministic():
    torch.manual_seed(4)
    B, H, Hk, S, p = 2, 4, 2, 256, 0.1
    dev = "cuda"
    q, do = [(torch.randn(B * S, H * 64, device=dev) * 1.5).bfloat16() for _ in range(2)]
    k, v = [(torch.randn(B * S, Hk * 64, device=dev) * 1.5).bfloat16() for _ in range(2)]
    rng = T.RngState(17, dev)
    a = _run(q, k, v, do, B, H, S, Hk=Hk, p=p, rng=rng)
    b = _run(q, k, v, do, B, H, S, Hk=Hk, p=p, rng=rng)
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])  # two runs, the same bits
    # other Q and dO in the heads of group 1 (query heads 2, 3)
    q2, do2 = q.clone(), do.clone()
    q2[:, 128:] = (torch.randn(B * S, 128, device=dev) * 1.5).bfloat16()
    do2[:, 128:] = (torch.randn(B * S, 128, device=dev) * 1.5).bfloat16()
    c = _run(q2, k, v, do2, B, H, S, Hk=Hk, p=p, rng=rng)
    for name, x, y in (("dk", a[3], c[3]), ("dv", a[4], c[4])):
        assert torch.equal(x[:, :64], y[:, :64]), name
        assert not torch.equal(x[:, 64:], y[:, 64:]), name
    assert float(a[3][:, :64].float().abs().max()) > 0


@gpu
def test_gqa_entries_refuse_bad_arguments():
    B, H = 2, 4
    dev = "cuda"
    x = torch.zeros(B * 256, H * 64, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(B * H, 256, dtype=torch.float32, device=dev)
    for Hk, Sq, Sk, causal in ((3, 128, 128, False), (0, 128, 128, False), (2, 100, 128, False),
                               (2, 128, 100, False), (2, 128, 256, True)):
        with pytest.raises(T._lib.HipKernelError):
            T.attention_fwd(x, x, x, x.clone(), lse, B, H, Sq, Sk=Sk, Hk=Hk, causal=causal)
        with pytest.raises(T._lib.HipKernelError):
            T.attention_bwd(x, x, x, x, x, lse, x.clone(), x.clone(), x.clone(), B, H, Sq, Sk=Sk, Hk=Hk,
                            causal=causal)


# ------------------------------------------------------------------ public surface on the GPU
@gpu
@pytest.mark.parametrize("causal", [False, True])
def test_nn_attention_gqa_gpu_matches_cpu_path(causal):
    """fp32 tensors holding bf16-representable values, so both paths start from the same numbers
    (the kernels compute in bf16 by design)."""
    torch.manual_seed(2)
    B, H, Hk, S = 2, 4, 2, 256
    q = torch.randn(B, S, H * 64).bfloat16().float()
    k, v = [torch.randn(B, S, Hk * 64).bfloat16().float() for _ in range(2)]
    do = torch.randn(B, S, H * 64).bfloat16().float()
    seqlen = torch.tensor([256, 70])
    cpu = [t.clone().requires_grad_(True) for t in (q, k, v)]
    oc = N.attention(*cpu, H, seqlen=seqlen, causal=causal, num_kv_heads=Hk)
    oc.backward(do)
    dev = [t.cuda().requires_grad_(True) for t in (q, k, v)]
    og = N.attention(*dev, H, seqlen=seqlen.cuda(), causal=causal, num_kv_heads=Hk)
    og.backward(do.cuda())
    assert og.shape == (B, S, H * 64) and dev[1].grad.shape == (B, S, Hk * 64) == dev[2].grad.shape
    torch.testing.assert_close(og.detach().cpu(), oc.detach(), atol=3e-2, rtol=3e-2)
    for name, g, c in zip("qkv", dev, cpu):
        rel = _rel(g.grad.cpu(), c.grad)
        print("d" + name, rel)
        assert rel < 2e-2, (name, rel)


@gpu
def test_nn_attention_gqa_gpu_refusals():
    q = torch.randn(2, 128, 256, device="cuda")
    kv = torch.randn(2, 128, 128, device="cuda")
    with pytest.raises(InvalidArgumentError):
        N.attention(q, kv, kv, 4, num_kv_heads=3)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, kv, kv, 4, num_kv_heads=1)
    with pytest.raises(InvalidArgumentError):  # head size 32
        N.attention(q, kv, kv, 8, num_kv_heads=4)


@gpu
@pytest.mark.parametrize("cross", [False, True])
def test_multi_head_attention_mqa_gpu_matches_cpu(cross):
    """Forward and gradients of MultiHeadAttention(4, num_kv_heads=1). Weights of O(1/sqrt(fan_in))
    so that q, k, v and the output are O(1), the scale the output bar (atol = rtol = 3e-2) was set
    for. The projections around the attention kernels are fp32 on both devices (fp32 inputs take
    the exact-fp32 GEMM), i.e. linear maps of the kernel's dq / dk / dv and output, so the
    gradients are held to the kernel's own gradient bar, relative L2 < 2e-2; output/bias's gradient
    does not pass through the attention at all."""
    torch.manual_seed(6)
    L.reset_naming(0)
    B, S, Sk, D, H, Hk = 2, 128, 256, 128, 4, 1
    inner, ikv = H * 64, Hk * 64
    x = torch.randn(B, S, D).bfloat16().float()
    mem = torch.randn(B, Sk, D).bfloat16().float() if cross else None
    dy = torch.randn(B, S, D)
    seqlen = torch.tensor([256, 101] if cross else [128, 77])
    cpu = L.MultiHeadAttention(H, num_kv_heads=Hk)
    gpu_layer = L.MultiHeadAttention(H, num_kv_heads=Hk)
    with torch.no_grad():
        cpu(x)
        cpu.qkv_kernel.copy_((torch.randn(D, inner + 2 * ikv) / math.sqrt(D)).bfloat16().float())
        cpu.qkv_bias.copy_((torch.randn(inner + 2 * ikv) * 0.1).bfloat16().float())
        cpu.out_kernel.copy_((torch.randn(inner, D) / math.sqrt(inner)).bfloat16().float())
        cpu.out_bias.copy_((torch.randn(D) * 0.1).bfloat16().float())
        gpu_layer(x.cuda())
        gpu_layer.load_state_dict(cpu.state_dict())

    def run(layer, dev):
        xi = x.clone().to(dev).requires_grad_(True)
        mi = mem.clone().to(dev).requires_grad_(True) if cross else None
        y = layer(xi, value=mi, seqlen=seqlen.to(dev))
        y.backward(dy.to(dev))
        grads = {"x": xi.grad}
        if cross:
            grads["value"] = mi.grad
        for n, t in layer.named_variables():
            grads[n.split("/", 1)[1]] = t.grad
        return y.detach().cpu(), {n: g.cpu() for n, g in grads.items()}

    want, gw = run(cpu, "cpu")
    got, gg = run(gpu_layer, "cuda")
    assert got.shape == (B, S, D)
    print("max abs err", float((got - want).abs().max()), "rel L2", _rel(got, want))
    torch.testing.assert_close(got, want, atol=3e-2, rtol=3e-2)
    assert set(gg) == set(gw) and gg["qkv/kernel"].shape == (D, inner + 2 * ikv)
    rels = {n: _rel(gg[n], gw[n]) for n in gw}
    print("grad rel L2", rels)
    for n, rel in rels.items():
        assert rel < 2e-2, (n, rel)
