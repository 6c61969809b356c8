"""CPU paths of the grouped matmul and the mixture-of-experts layer against plain references:
`ttd.nn.grouped_matmul` against a float64 loop over the groups under autograd, and
`layers.MixtureOfExperts` against a per-token dense reference (for every token the sum over its
top_k experts of gate * ffn_e(x)), with `aux_loss` against its formula."""
import pytest
import torch
import torch.nn.functional as F

from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError


def test_grouped_matmul_against_float64_loop():
    g = torch.Generator().manual_seed(0)
    sizes = [0, 3, 1, 0, 5]                       # 9 rows in groups, 2 rows in none
    x = torch.randn(11, 6, generator=g, requires_grad=True)
    w = torch.randn(5, 6, 4, generator=g, requires_grad=True)
    dy = torch.randn(11, 4, generator=g)
    y = N.grouped_matmul(x, w, torch.tensor(sizes))
    y.backward(dy)
    xd, wd = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    ref, r = torch.zeros(11, 4, dtype=torch.float64), 0
    for e, m in enumerate(sizes):
        ref = ref + F.pad(xd[r:r + m] @ wd[e], (0, 0, r, 11 - r - m))
        r += m
    ref.backward(dy.double())
    for got, want in ((y, ref), (x.grad, xd.grad), (w.grad, wd.grad)):
        torch.testing.assert_close(got.double(), want.detach(), rtol=1e-5, atol=1e-5)
    assert not y[9:].any() and not x.grad[9:].any()


@pytest.mark.parametrize("gated", [True, False])
def test_mixture_of_experts_against_per_token_reference(gated):
    L.reset_naming(seed=3)
    E, k, T, D = 4, 2, 24, 8
    layer = L.MixtureOfExperts(E, k, 16, gated=gated)
    x = torch.randn(2, T // 2, D, generator=torch.Generator().manual_seed(1))
    y = layer(x)
    assert [n for n, _ in layer.named_variables()] == ["mixture_of_experts/" + s + "/kernel"
                                                       for s in ("router", "experts_in", "experts_out")]
    router, w_in, w_out = (v.detach().double() for v in layer.variables)
    xd = x.reshape(T, D).double()
    probs = torch.softmax(xd @ router, -1)
    ref = torch.zeros(T, D, dtype=torch.float64)
    counts = torch.zeros(E, dtype=torch.float64)
    for t in range(T):
        top = torch.topk(probs[t], k)
        for p, e in zip(top.values / top.values.sum(), top.indices.tolist()):
            h = xd[t] @ w_in[e]
            h = F.silu(h[:16]) * h[16:] if gated else F.gelu(h, approximate="tanh")
            ref[t] += p * (h @ w_out[e])
            counts[e] += 1
    torch.testing.assert_close(y.reshape(T, D).double(), ref, rtol=1e-5, atol=1e-5)
    aux = E * torch.sum(counts / (T * k) * probs.mean(0))
    torch.testing.assert_close(layer.aux_loss.double(), aux, rtol=1e-5, atol=1e-6)


def test_refusals():
    x, w = torch.randn(4, 8), torch.randn(3, 8, 8)
    with pytest.raises(InvalidArgumentError):
        N.grouped_matmul(x, w, torch.tensor([1, 1, 1, 1]))           # E mismatch
    with pytest.raises(InvalidArgumentError):
        N.grouped_matmul(x, w, torch.tensor([1.0, 1.0, 1.0]))        # non-integer sizes
    with pytest.raises(InvalidArgumentError):
        L.MixtureOfExperts(4, 5, 16)                                 # top_k > E
