"""CPU paths of `ttd.nn.moe_route` / `moe_dispatch` / `moe_combine`: against float64 statements,
and, gradients included, against the formula `layers.MixtureOfExperts` used before they existed,
written out inline; refusals that need no GPU; the layer's variables."""
import pytest
import torch

from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

T, E, K, D = 13, 5, 2, 6


def _inputs(dtype):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(s, generator=g).to(dtype).requires_grad_() for s in ((T, E), (T, D), (E, D, D))]


def _previous_formula(logits, x, w):
    """MixtureOfExperts.call before ttd.nn.moe_*, with one grouped matmul as the expert."""
    probs = torch.softmax(logits, dim=-1)
    gate, expert = torch.topk(probs, K, dim=-1)
    gate = gate / gate.sum(-1, keepdim=True)
    slots = expert.reshape(-1)
    order = torch.argsort(slots, stable=True)
    inv = torch.argsort(order)
    sizes = torch.bincount(slots, minlength=E)
    h = N.grouped_matmul(x[order // K], w, sizes)
    return (h[inv].reshape(T, K, -1).to(gate.dtype) * gate.unsqueeze(-1)).sum(1), probs


def test_cpu_paths_against_the_previous_formula_in_float64():
    outs, dtype, tol = [], torch.float32, 1e-5
    for new in (True, False):
        logits, x, w = _inputs(dtype)
        if new:
            gate, expert, probs = N.moe_route(logits, K)
            xs, sizes, plan = N.moe_dispatch(x, expert, E)
            assert int(sizes.sum()) == T * K and plan.k == K
            y = N.moe_combine(N.grouped_matmul(xs, w, sizes), gate, plan)
        else:
            lg, xd, wd = (v.detach().double().requires_grad_() for v in (logits, x, w))
            y, probs = _previous_formula(lg, xd, wd)
            logits, x, w = lg, xd, wd
        (y.sum() + (probs * torch.arange(E)).sum()).backward()      # gradients through gate and through probs
        outs.append([y.detach(), logits.grad, x.grad, w.grad])
    for got, ref in zip(*outs):
        torch.testing.assert_close(got.double(), ref, rtol=tol, atol=tol)


def test_offsets_stand_in_for_group_sizes():
    x, w = torch.randn(7, 4), torch.randn(3, 4, 2)
    sizes = torch.tensor([2, 0, 4])
    offsets = torch.tensor([0, 2, 2, 6], dtype=torch.int32)
    assert torch.equal(N.grouped_matmul(x, w, offsets=offsets), N.grouped_matmul(x, w, sizes))


def test_refusals():
    logits, x = torch.randn(4, 3), torch.randn(4, 8)
    gate, expert, _ = N.moe_route(logits, 2)
    _, sizes, plan = N.moe_dispatch(x, expert, 3)
    for call in (lambda: N.moe_route(logits, 4),                                   # top_k > E
                 lambda: N.moe_route(logits[0], 1),                                # not [T, E]
                 lambda: N.moe_dispatch(x, expert.float(), 3),                     # ids not integers
                 lambda: N.moe_dispatch(x[:3], expert, 3),                         # rows differ
                 lambda: N.moe_combine(torch.randn(7, 8), gate, plan),             # not T * k rows
                 lambda: N.moe_combine(torch.randn(8, 8), gate[:, :1], plan),      # gate not [T, k]
                 lambda: N.grouped_matmul(torch.randn(8, 8), torch.randn(3, 8, 8), sizes, offsets=sizes.int()),
                 lambda: N.grouped_matmul(torch.randn(8, 8), torch.randn(3, 8, 8))):
        with pytest.raises(InvalidArgumentError):
            call()


def test_layer_builds_the_same_three_variables():
    L.reset_naming(seed=1)
    layer = L.MixtureOfExperts(4, 2, 16)
    layer(torch.randn(3, 8))
    assert [(n, tuple(v.shape)) for n, v in layer.named_variables()] == [
        ("mixture_of_experts/router/kernel", (8, 4)), ("mixture_of_experts/experts_in/kernel", (4, 8, 32)),
        ("mixture_of_experts/experts_out/kernel", (4, 16, 8))]
    assert layer.aux_loss is not None and layer.aux_loss.dim() == 0
