#!/usr/bin/env python3
"""Time the fused attention kernels at BERT-Large shapes (B=32, H=16, S=512, D=64) with and
without attention dropout; the backward on the single-kernel path and on the split dQ / dK-dV
kernels. --causal times the causal kernels (split backward only: the fused kernel has no causal
form); TTD_ATTN_CAUSAL_ORDER=natural selects their natural block order for the A/B.
--kv-seq N times cross-attention: S = 512 queries over a memory of N keys (forward and the split
backward — the fused and causal kernels are self-attention only); FLOPs 4 B H Sq Sk 64.
--kv-heads N times grouped-query attention: the 16 query heads over N key/value heads (N = 1:
multi-query), K / V column slices of a fused [B*S, (16 + 2*N)*64] buffer, forward and the split
backward, with --causal as well; N = 16 is self-attention through the same buffers. The FLOPs
do not depend on N.
--window L,R times the BAND kernels with a sliding window (q - L <= k <= q + R; "none" on a side
for no bound), --segments N with N equal documents per row (N = 1: the band form with nothing
masked, against the plain kernels); both combine with each other, --causal and --kv-heads. The
line then also gives the time of the table kernel (ttdk_attn_band) and the share of the dense
64 x 64 tiles the forward streams; TF/s stay dense-equivalent. --seq S sets the sequence length.
usage: python tools/attn_bench.py [B] [--causal | --kv-seq N] [--kv-heads N] [--window L,R] [--segments N] [--seq S]"""
import sys

import torch

sys.path.insert(0, ".")
from tensorflow_train_distributed_amd.ops import transformer as T  # noqa: E402


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


argv = sys.argv[1:]
Sk = None
if "--kv-seq" in argv:
    i = argv.index("--kv-seq")
    Sk = int(argv[i + 1])
    del argv[i:i + 2]
Hk = None
if "--kv-heads" in argv:
    i = argv.index("--kv-heads")
    Hk = int(argv[i + 1])
    del argv[i:i + 2]
window = segments = None
S_arg = 512
if "--window" in argv:
    i = argv.index("--window")
    window = tuple(None if x == "none" else int(x) for x in argv[i + 1].split(","))
    del argv[i:i + 2]
if "--segments" in argv:
    i = argv.index("--segments")
    segments = int(argv[i + 1])
    del argv[i:i + 2]
if "--seq" in argv:
    i = argv.index("--seq")
    S_arg = int(argv[i + 1])
    del argv[i:i + 2]
banded = window is not None or segments is not None
if banded and Sk is not None:
    sys.exit("--window / --segments and --kv-seq exclude each other: a band is a self-attention mask")
args = [a for a in argv if not a.startswith("--")]
causal = "--causal" in argv
if causal and Sk is not None:
    sys.exit("--causal and --kv-seq exclude each other: the causal kernels need Sk == S")
if Hk is not None and Sk is not None:
    sys.exit("--kv-heads and --kv-seq exclude each other")
B, H, S, D = (int(args[0]) if args else 32), 16, S_arg, 64
if Hk is not None and (Hk <= 0 or H % Hk):
    sys.exit("--kv-heads must divide %d" % H)
# one label, one buffer layout per mode; everything below is shared
if Sk is not None:
    label = "cross Sq=%d Sk=%d " % (S, Sk)
elif Hk is not None:
    label = "%skv-heads %2d " % ("causal " if causal else "", Hk)
else:
    label = "causal " if causal else ""
if banded:
    label += "band%s%s " % ("" if window is None else " window %s,%s" % window,
                            "" if segments is None else " %d docs" % segments)
Hkv, Skv = H if Hk is None else Hk, S if Sk is None else Sk
# Q / K / V column views of one fused [B*S, (H + 2*Hkv)*D] projection, dQ / dK / dV of another
qkv = (torch.randn(B * S, (H + 2 * Hkv) * D, device="cuda") * 0.5).bfloat16()
dqkv = torch.empty_like(qkv)
(q, k, v), (dq, dk, dv) = [(t[:, :H * D], t[:, H * D:(H + Hkv) * D], t[:, (H + Hkv) * D:]) for t in (qkv, dqkv)]
out = torch.empty(B * S, H * D, device="cuda", dtype=torch.bfloat16)
lse = torch.empty(B * H, S, device="cuda")
delta = torch.empty_like(lse)
dout = torch.randn_like(out)
rng = T.RngState(7, "cuda")
if Sk is not None:
    # the memory: K / V out of a fused [B*Sk, 2*H*D] projection, dK / dV into one; Q / dQ stay
    # views of the [B*S, 3*H*D] buffers
    kvm = (torch.randn(B * Sk, 2 * H * D, device="cuda") * 0.5).bfloat16()
    (k, v), (dk, dv) = [(t[:, :H * D], t[:, H * D:]) for t in (kvm, torch.empty_like(kvm))]
# FLOPs 4 B H Sq Sk D; the backward counted as the algorithm's 5 products (2.5x the forward's 2);
# TF/s of the causal runs are in dense-equivalent FLOPs (the skipped tiles counted), for comparison
fl = 4.0 * B * H * S * Skv * D
band, band_note = None, ""
if banded:
    ids = None
    if segments is not None:
        ids = (torch.arange(S, dtype=torch.int32, device="cuda") // -(-S // segments)).repeat(B, 1).contiguous()
    band = torch.empty(T.attention_band_ints(B, S), dtype=torch.int32, device="cuda")
    tband = timeit(lambda: T.attention_band(ids, None, window, causal, B, S, out=band))
    blk = band[4 * B * S:].reshape(B, S // 128, 4).cpu()
    share = float((blk[..., 1] - blk[..., 0]).sum()) / (B * (S // 128) * (S // 64))
    band_note = "   table %5.1f us, fwd streams %4.1f %% of the tiles" % (tband, 100 * share)
for p in (0.0, 0.1):
    kw = dict(Sk=Sk, Hk=Hk, p_drop=p, rng=rng, causal=causal)
    if banded:  # causal is in the table
        kw = dict(Hk=Hk, p_drop=p, rng=rng, band=band)
    tf = timeit(lambda: T.attention_fwd(q, k, v, out, lse, B, H, S, **kw))
    line = "%sp=%.1f  fwd %6.1f us %5.0f TF/s   bwd" % (label, p, tf, fl / tf / 1e6)
    # the fused backward has a self-attention, non-causal form only
    for fused in ((True, False) if label == "" else (False,)):
        T.set_fused_attention_bwd(fused)
        tb = timeit(lambda: T.attention_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, S, delta=delta, **kw))
        line += " %s %6.1f us %5.0f TF/s  " % ("fused" if fused else "split", tb, 2.5 * fl / tb / 1e6)
    T.set_fused_attention_bwd(False)
    print(line.rstrip() + band_note)
