"""`ttd.nn.linear_cross_entropy` on CPU tensors (the fp32 torch formula) against the float64 formula
with autograd, ignored labels included: loss and the gradients of x, weights and bias."""
import pytest
import torch

import tensorflow_train_distributed_amd.nn as ttd_nn
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError


@pytest.mark.parametrize("bias", [True, False])
def test_cpu_against_float64_autograd(bias):
    gen = torch.Generator().manual_seed(3)
    V = 24
    x, w, b = (torch.randn(s, generator=gen, requires_grad=True) for s in ((2, 5, 16), (V, 16), (V,)))
    lab = torch.randint(0, V, (2, 5), generator=gen)
    lab[0, 1], lab[1, 3] = -1, V
    loss = ttd_nn.linear_cross_entropy(x, w, lab, b if bias else None)
    coef = torch.randn(2, 5, generator=gen)
    (loss * coef).sum().backward()
    xd, wd, bd = (t.detach().double().requires_grad_() for t in (x, w, b))
    z = xd @ wd.T + (bd if bias else 0)
    valid = (lab >= 0) & (lab < V)
    ref = (torch.logsumexp(z, -1) - z.gather(-1, lab.clamp(0, V - 1)[..., None])[..., 0]) * valid
    (ref * coef.double()).sum().backward()
    assert loss.dtype == torch.float32 and not loss[~valid].any()
    assert not x.grad[~valid].any(), "an ignored example has no gradient"
    pairs = [(loss, ref), (x.grad, xd.grad), (w.grad, wd.grad)] + ([(b.grad, bd.grad)] if bias else [])
    for got, want in pairs:
        torch.testing.assert_close(got.double(), want.detach(), atol=2e-5, rtol=2e-5)


def test_cpu_refuses_mismatched_shapes():
    with pytest.raises(InvalidArgumentError):
        ttd_nn.linear_cross_entropy(torch.zeros(4, 16), torch.zeros(24, 8), torch.zeros(4, dtype=torch.long))
