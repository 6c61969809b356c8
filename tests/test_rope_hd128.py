"""Rotary embedding at head size 128 (rope.hip, ttdk_rope_hd) against a float64 rotation."""
import numpy as np
import pytest
import torch

from tensorflow_train_distributed_amd.ops import transformer as T

HD, HALF = 128, 64


def test_rope_table_head_dim():
    t = T.rope_table(300, device="cpu")
    assert T.rope_table(300, device="cpu", head_dim=64) is t  # same cache entry, default unchanged
    w = T.rope_table(300, device="cpu", head_dim=HD)
    assert w.shape == (300, 2, HALF) and w.dtype == torch.float32
    ang = np.arange(300.0)[:, None] * 10000.0 ** (-np.arange(HALF) / HALF)
    np.testing.assert_array_equal(w.numpy(), np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 192])
@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 2e-2)])
def test_rope_hd128_against_float64(dtype, tol, in_place, S):
    torch.manual_seed(S)
    Bn, heads, pos0 = 2, 3, 7  # q and k heads of a [q | k | v] projection; v (128 more columns) stays
    width = heads * HD
    buf = torch.randn(Bn * S, width + HD, device="cuda").to(dtype)
    x0 = buf.clone()
    table = T.rope_table(512, device="cuda", head_dim=HD)
    x = buf[:, :width]
    y = x if in_place else torch.full_like(buf, 3.0)[:, :width]
    T.rope(x, y, table, S, heads, pos0=pos0, head_dim=HD)

    xd = x0[:, :width].double().reshape(Bn, S, heads, HD).cpu()
    ang = (pos0 + torch.arange(S, dtype=torch.float64))[:, None] * 10000.0 ** (
        -torch.arange(HALF, dtype=torch.float64) / HALF)
    cos, sin = ang.cos()[None, :, None, :], ang.sin()[None, :, None, :]
    lo, hi = xd[..., :HALF], xd[..., HALF:]
    want = torch.cat([lo * cos - hi * sin, hi * cos + lo * sin], -1).reshape(Bn * S, width)
    torch.testing.assert_close(y.double().cpu(), want, atol=tol, rtol=tol)
    # columns past heads*128 are untouched (in place: v; out of place: the fill)
    tail = y.as_strided((Bn * S, HD), (y.stride(0), 1), y.storage_offset() + width)
    assert torch.equal(tail, x0[:, width:] if in_place else torch.full_like(tail, 3.0))
    back = T.rope(y, torch.empty_like(x0[:, :width]), table, S, heads, pos0=pos0, inverse=True, head_dim=HD)
    torch.testing.assert_close(back.double().cpu(), x0[:, :width].double().cpu(), atol=2 * tol, rtol=2 * tol)
