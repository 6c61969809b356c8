"""Banded attention masks without a GPU: the host mirror of the band table against the mask built
from the definitions, and the CPU paths of ttd.nn.attention(segment_ids=, window=) and
layers.MultiHeadAttention(window=) / call(segment_ids=) against an explicit masked softmax."""
import math

import numpy as np
import pytest
import torch

import band_oracle as BO
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import transformer as T
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError


def _random_case(rng, B, S):
    ids = None
    if rng.random() < 0.8:
        ids = np.zeros((B, S), dtype=np.int32)
        for b in range(B):
            at, doc = 0, 0
            while at < S:
                n = int(rng.integers(1, S // 2))
                # an id may reappear later (another document); some runs are padding
                ids[b, at:at + n] = -1 if rng.random() < 0.2 else doc % 3
                at, doc = at + n, doc + 1
    seqlen = rng.integers(0, S + 1, B).astype(np.int32) if rng.random() < 0.6 else None
    side = lambda: None if rng.random() < 0.4 else int(rng.integers(0, S // 2))  # noqa: E731
    window = None if rng.random() < 0.3 else (side(), side())
    return ids, seqlen, window, bool(rng.random() < 0.4)


def _check_table(tab, mask, B, S):
    tok = tab[:4 * B * S].reshape(B, S, 4)
    blk = tab[4 * B * S:].reshape(B, S // 128, 4)
    ar = np.arange(S)
    for b in range(B):
        for s in range(S):
            klo, khi, qlo, qhi = tok[b, s]
            assert np.array_equal(mask[b, s], (ar >= klo) & (ar < khi)), ("row", b, s, tok[b, s])
            assert np.array_equal(mask[b, :, s], (ar >= qlo) & (ar < qhi)), ("column", b, s, tok[b, s])
        for j in range(S // 128):
            kt0, kt1, qt0, qt1 = blk[b, j]
            assert 0 <= kt0 <= kt1 <= S // 64 and 0 <= qt0 <= qt1 <= S // 64
            assert qt0 % 2 == 0 and qt1 % 2 == 0  # bwd_kv consumes two tiles per trip
            rows = mask[b, j * 128:(j + 1) * 128]
            assert not rows[:, :kt0 * 64].any() and not rows[:, kt1 * 64:].any()
            cols = mask[b, :, j * 128:(j + 1) * 128]
            assert not cols[:qt0 * 64].any() and not cols[qt1 * 64:].any()
            # tight: the first and the last tile hold something (up to the even rounding)
            if rows.any():
                assert rows[:, kt0 * 64:kt0 * 64 + 64].any() and rows[:, kt1 * 64 - 64:kt1 * 64].any()
            else:
                assert kt0 == kt1
            if cols.any():
                assert cols[qt0 * 64:qt0 * 64 + 128].any() and cols[qt1 * 64 - 128:qt1 * 64].any()
            else:
                assert qt0 == qt1


def test_band_host_matches_the_definitions_on_random_cases():
    rng = np.random.default_rng(0)
    B, S = 2, 256
    for _ in range(12):
        ids, seqlen, window, causal = _random_case(rng, B, S)
        tab = T.attention_band_host(ids, seqlen, window, causal, B, S)
        assert tab.dtype == np.int32 and tab.shape == (T.attention_band_ints(B, S),)
        _check_table(tab, BO.brute_mask(ids, seqlen, window, causal, B, S), B, S)


def test_band_host_named_cases():
    B, S = 2, 384
    ids = np.stack([BO.runs([70, 58, 128, 100], S), BO.runs([1, 383], S)])
    for window, causal, seqlen in ((None, False, None), ((40, 0), True, None), ((100, 30), False, None),
                                   ((None, 30), False, None), ((200, None), False, None), ((0, 0), False, None),
                                   ((90, 0), True, np.array([384, 150], dtype=np.int32))):
        for use_ids in (ids, None):
            tab = T.attention_band_host(use_ids, seqlen, window, causal, B, S)
            _check_table(tab, BO.brute_mask(use_ids, seqlen, window, causal, B, S), B, S)
    # the padded tail: (S, 0) records, nothing streamed by a block that is all padding
    tok = T.attention_band_host(ids, None, None, False, B, S)[:4 * B * S].reshape(B, S, 4)
    assert (tok[0, 356:] == np.array([S, 0, S, 0])).all()
    assert tuple(tok[1, 0]) == (0, 1, 0, 1) and tuple(tok[1, 1]) == (1, 384, 1, 384)


def test_band_host_refuses_malformed_input():
    ids = np.zeros((2, 256), dtype=np.int32)
    with pytest.raises(InvalidArgumentError):
        T.attention_band_host(ids, None, (-1, 0), False, 2, 256)
    with pytest.raises(InvalidArgumentError):
        T.attention_band_host(ids[:, :128], None, None, False, 2, 256)
    with pytest.raises(InvalidArgumentError):
        T.attention_band_host(ids.astype(np.int64), None, None, False, 2, 256)
    with pytest.raises(InvalidArgumentError):
        T.attention_band_host(None, None, (1, 2, 3), False, 2, 256)
    with pytest.raises(InvalidArgumentError):
        T.attention_band_host(None, None, None, False, 2, 200)


def _explicit(q, k, v, H, Hk, mask):
    """Masked softmax attention written out: [B, S, H*hd]; rows that attend nothing are zero."""
    B, S, D = q.shape
    hd = D // H
    qh = q.reshape(B, S, H, hd).transpose(1, 2)
    kh = k.reshape(B, S, Hk, hd).transpose(1, 2).repeat_interleave(H // Hk, dim=1)
    vh = v.reshape(B, S, Hk, hd).transpose(1, 2).repeat_interleave(H // Hk, dim=1)
    sc = qh @ kh.transpose(-1, -2) / math.sqrt(hd)
    out = torch.zeros(B, H, S, hd)
    for b in range(B):
        for s in range(S):
            sel = mask[b, s]
            if sel.any():
                out[b, :, s] = (sc[b, :, s][:, sel].softmax(-1)[:, None] @ vh[b][:, sel])[:, 0]
    return out.transpose(1, 2).reshape(B, S, D)


def test_nn_attention_cpu_band_matches_explicit_softmax():
    torch.manual_seed(0)
    B, S, H, Hk, hd = 2, 48, 4, 2, 16
    q = torch.randn(B, S, H * hd, requires_grad=True)
    k, v = torch.randn(B, S, Hk * hd), torch.randn(B, S, Hk * hd)
    ids = np.stack([BO.runs([10, 7, 20], S), BO.runs([1, 47], S)])
    seqlen = np.array([48, 30], dtype=np.int32)
    for window, causal in (((5, 2), False), ((None, 3), False), (None, True), ((6, None), True)):
        mask = torch.from_numpy(BO.brute_mask(ids, seqlen, window, causal, B, S))
        got = N.attention(q, k, v, H, seqlen=torch.from_numpy(seqlen), causal=causal, num_kv_heads=Hk,
                          segment_ids=torch.from_numpy(ids), window=window)
        torch.testing.assert_close(got, _explicit(q, k, v, H, Hk, mask), atol=1e-5, rtol=1e-4)
        dead = ~mask.any(-1)
        assert bool(dead.any())
        assert float(got.detach()[dead].abs().max()) == 0.0  # padding rows: zeros, not NaN
        g, = torch.autograd.grad(got.sum(), q)
        assert bool(torch.isfinite(g).all()) and float(g[dead].abs().max()) == 0.0


def test_nn_attention_without_a_band_is_todays_call():
    torch.manual_seed(1)
    q, k, v = [torch.randn(2, 32, 64) for _ in range(3)]
    seqlen = torch.tensor([32, 20])
    want = N.attention(q, k, v, 4, seqlen=seqlen, causal=True)
    assert torch.equal(N.attention(q, k, v, 4, seqlen=seqlen, causal=True, segment_ids=None, window=None), want)
    assert torch.equal(N.attention(q, k, v, 4, seqlen=seqlen, causal=True, window=(None, None)), want)


def test_nn_attention_band_refusals():
    q = torch.randn(2, 32, 64)
    m = torch.randn(2, 16, 64)
    ids = torch.zeros(2, 32, dtype=torch.int32)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, m, m, 4, window=(3, 3))
    with pytest.raises(InvalidArgumentError):
        N.attention(q, m, m, 4, segment_ids=ids)
    with pytest.raises(InvalidArgumentError):
        N.attention(q, q, q, 4, window=(-1, 3))
    with pytest.raises(InvalidArgumentError):
        N.attention(q, q, q, 4, segment_ids=ids[:, :16])
    with pytest.raises(InvalidArgumentError):
        N.attention(q, q, q, 4, segment_ids=ids.long())
    with pytest.raises(InvalidArgumentError):
        L.MultiHeadAttention(4, window=(2, -5))


def test_multi_head_attention_window_and_segments_cpu():
    torch.manual_seed(2)
    L.reset_naming(0)
    B, S, D, H, Hk = 2, 40, 48, 4, 2
    x = torch.randn(B, S, D)
    ids = np.stack([BO.runs([12, 20], S), BO.runs([40], S)])
    layer, plain = L.MultiHeadAttention(H, key_dim=16, num_kv_heads=Hk, window=(6, 1)), \
        L.MultiHeadAttention(H, key_dim=16, num_kv_heads=Hk)
    with torch.no_grad():
        plain(x)
        layer(x)
    assert [n.split("/", 1)[1] for n, _ in layer.named_variables()] == \
        [n.split("/", 1)[1] for n, _ in plain.named_variables()]  # no new variables
    layer.load_state_dict(plain.state_dict())
    inner, ikv = H * 16, Hk * 16
    with torch.no_grad():
        qkv = x @ plain.qkv_kernel + plain.qkv_bias
        mask = torch.from_numpy(BO.brute_mask(ids, None, (6, 1), True, B, S))
        a = _explicit(qkv[..., :inner], qkv[..., inner:inner + ikv], qkv[..., inner + ikv:], H, Hk, mask)
        want = a @ plain.out_kernel + plain.out_bias
        got = layer(x, segment_ids=torch.from_numpy(ids), use_causal_mask=True, training=False)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-4)
    with torch.no_grad():  # the window alone is live
        assert not torch.allclose(layer(x, training=False), plain(x, training=False))
