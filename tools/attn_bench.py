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
usage: python tools/attn_bench.py [B] [--causal | --kv-seq N] [--kv-heads N]"""
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
args = [a for a in argv if not a.startswith("--")]
causal = "--causal" in argv
if causal and Sk is not None:
    sys.exit("--causal and --kv-seq exclude each other: the causal kernels need Sk == S")
if Hk is not None and Sk is not None:
    sys.exit("--kv-heads and --kv-seq exclude each other")
B, H, S, D = (int(args[0]) if args else 32), 16, 512, 64
if Hk is not None:
    if Hk <= 0 or H % Hk:
        sys.exit("--kv-heads must divide %d" % H)
    gqkv = (torch.randn(B * S, (H + 2 * Hk) * D, device="cuda") * 0.5).bfloat16()
    gq, gk, gv = gqkv[:, :H * D], gqkv[:, H * D:(H + Hk) * D], gqkv[:, (H + Hk) * D:]
    gd = torch.empty_like(gqkv)
    gdq, gdk, gdv = gd[:, :H * D], gd[:, H * D:(H + Hk) * D], gd[:, (H + Hk) * D:]
    gout = torch.empty(B * S, H * D, device="cuda", dtype=torch.bfloat16)
    glse = torch.empty(B * H, S, device="cuda")
    gdout = torch.randn_like(gout)
    grng = T.RngState(7, "cuda")
    fl_g = 4.0 * B * H * S * S * D
    T.set_fused_attention_bwd(False)
    for p in (0.0, 0.1):
        kw = dict(Hk=Hk, p_drop=p, rng=grng, causal=causal)
        tf = timeit(lambda: T.attention_fwd(gq, gk, gv, gout, glse, B, H, S, **kw))
        tb = timeit(lambda: T.attention_bwd(gq, gk, gv, gout, gdout, glse, gdq, gdk, gdv, B, H, S, **kw))
        print("%skv-heads %2d p=%.1f  fwd %6.1f us %5.0f TF/s   bwd split %6.1f us %5.0f TF/s"
              % ("causal " if causal else "", Hk, p, tf, fl_g / tf / 1e6, tb, 2.5 * fl_g / tb / 1e6))
    sys.exit(0)
qkv = (torch.randn(B * S, 3 * H * D, device="cuda") * 0.5).bfloat16()
q, k, v = qkv[:, :H * D], qkv[:, H * D:2 * H * D], qkv[:, 2 * H * D:]
out = torch.empty(B * S, H * D, device="cuda", dtype=torch.bfloat16)
lse = torch.empty(B * H, S, device="cuda")
dout = torch.randn_like(out)
dqkv = torch.empty_like(qkv)
rng = T.RngState(7, "cuda")
if Sk is not None:
    # the memory: K / V out of a fused [B*Sk, 2*H*D] projection, dK / dV into one; Q / dQ stay
    # views of the [B*S, 3*H*D] buffer. Goes through the cross entry points even at Sk == S.
    kvm = (torch.randn(B * Sk, 2 * H * D, device="cuda") * 0.5).bfloat16()
    dkvm = torch.empty_like(kvm)
    km, vm = kvm[:, :H * D], kvm[:, H * D:]
    fl_x = 4.0 * B * H * S * Sk * D
    st = T._lib.stream

    def xfwd(p):
        T._lib.call("ttdk_attn_fwd_cross", q.data_ptr(), q.stride(0), km.data_ptr(), km.stride(0), vm.data_ptr(),
                    vm.stride(0), out.data_ptr(), out.stride(0), lse.data_ptr(), None, B, H, S, Sk, p,
                    rng.t.data_ptr(), 0, 0, st())

    def xbwd(p):
        T._lib.call("ttdk_attn_bwd_cross", q.data_ptr(), q.stride(0), km.data_ptr(), km.stride(0), vm.data_ptr(),
                    vm.stride(0), out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(),
                    delta.data_ptr(), dqkv.data_ptr(), dqkv.stride(0), dkvm.data_ptr(), dkvm.stride(0),
                    dkvm[:, H * D:].data_ptr(), dkvm.stride(0), None, B, H, S, Sk, p, rng.t.data_ptr(), 0, 0, st())

    delta = torch.empty_like(lse)
    T.set_fused_attention_bwd(False)
    for p in (0.0, 0.1):
        tf = timeit(lambda: xfwd(p))
        tb = timeit(lambda: xbwd(p))
        print("cross Sq=%d Sk=%d p=%.1f  fwd %6.1f us %5.0f TF/s   bwd split %6.1f us %5.0f TF/s"
              % (S, Sk, p, tf, fl_x / tf / 1e6, tb, 2.5 * fl_x / tb / 1e6))
    sys.exit(0)
fl_f = 4.0 * B * H * S * S * D
kw = {"causal": True} if causal else {}
for p in (0.0, 0.1):
    tf = timeit(lambda: T.attention_fwd(q, k, v, out, lse, B, H, S, p_drop=p, rng=rng, **kw))
    res = {}
    for fused in ((False,) if causal else (True, False)):
        T.set_fused_attention_bwd(fused)
        res[fused] = timeit(lambda: T.attention_bwd(q, k, v, out, dout, lse, dqkv[:, :H * D], dqkv[:, H * D:2 * H * D],
                                                    dqkv[:, 2 * H * D:], B, H, S, p_drop=p, rng=rng, **kw))
    T.set_fused_attention_bwd(False)
    # backward FLOPs counted as the algorithm's 5 products (2.5x the forward's 2); TF/s of the
    # causal runs are in dense-equivalent FLOPs (the skipped tiles counted), for comparison
    if causal:
        print("causal p=%.1f  fwd %6.1f us %5.0f TF/s   bwd split %6.1f us %5.0f TF/s"
              % (p, tf, fl_f / tf / 1e6, res[False], 2.5 * fl_f / res[False] / 1e6))
    else:
        print("p=%.1f  fwd %6.1f us %5.0f TF/s   bwd fused %6.1f us %5.0f TF/s   split %6.1f us %5.0f TF/s"
              % (p, tf, fl_f / tf / 1e6, res[True], 2.5 * fl_f / res[True] / 1e6, res[False],
                 2.5 * fl_f / res[False] / 1e6))
