"""What the banded-attention test files share (a plain module, imported by them): the boolean
[B, S, S] mask built straight from the definitions — query q attends key k iff both lie in the same
maximal run of equal segment ids, neither id is negative, q - left <= k <= q + right (causal:
right = 0) and k < seqlen[b] — one query row at a time, with no interval arithmetic to share a
mistake with the table builders it checks."""
import numpy as np


def brute_mask(ids, seqlen, window, causal, B, S):
    left, right = (None, None) if window is None else window
    if causal:
        right = 0
    k = np.arange(S)
    m = np.zeros((B, S, S), dtype=bool)
    for b in range(B):
        run = np.zeros(S, dtype=np.int64)
        if ids is not None:
            for s in range(1, S):
                run[s] = run[s - 1] + (ids[b][s] != ids[b][s - 1])
        n = S if seqlen is None else int(seqlen[b])
        for q in range(S):
            ok = (run == run[q]) & (k < n)
            if ids is not None:
                ok &= (np.asarray(ids[b]) >= 0) & (ids[b][q] >= 0)
            if left is not None:
                ok &= k >= q - left
            if right is not None:
                ok &= k <= q + right
            m[b, q] = ok
    return m


def runs(lengths, S, pad_id=-1):
    """int32 [S] ids of consecutive documents of these lengths (ids 0, 1, ...), the rest padding."""
    out = np.full(S, pad_id, dtype=np.int32)
    at = 0
    for i, n in enumerate(lengths):
        out[at:at + n] = i
        at += n
    assert at <= S
    return out
