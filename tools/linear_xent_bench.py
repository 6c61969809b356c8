#!/usr/bin/env python3
"""The fused LM-head cross-entropy (linear_xent.hip through ops.transformer.linear_xent_fwd / _bwd)
against the unfused path the masked-LM head of models/bert.py uses, with a label on every row:

  fused    fwd: linear_xent_fwd (no logits)            bwd: linear_xent_bwd (chunks of the default size)
  unfused  fwd: logits = gemm(h, w^T) + bias (bf16 [T, V]), xent_vocab over them
           bwd: xent_vocab writes the gradient over the logits, dh = gemm(dlogits, w),
                dw = gemm(dlogits^T, h) in fp32, dbias = colsum(dlogits)

Time per call: HIP events around a window of eager calls on one stream, after 5 warm-up calls and a
probe that sizes the window; the two sides alternate in every repeat; best of the repeats, with the
spread (worst - best). Peak memory: torch.cuda.max_memory_allocated over one call, less what was
allocated before it (the operands), beside the size of a bf16 [T, V] tensor. The two sides' summed
loss and dh are compared at the timed shape. FLOP counted: what the algorithm needs, 2 T V H for the
forward and 6 T V H for forward + backward on both sides (the fused path's second pass over the logits
is its own cost, not useful work). Where a bf16 [T, V] tensor would reach 2 GiB only the fused side runs: it
holds no such tensor and every GEMM operand it hands to ops.gemm stays below 2 GiB, while the unfused
side's logits would be a GEMM operand of a size those kernels are not tested at (neither listed shape
reaches it: the second one's logits are 2004 MiB).
usage: python tools/linear_xent_bench.py [--repeats 3] [--window-ms 400] [--shapes 0,1]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16384, 1024, 30528), (8192, 4096, 128256)]  # T, H, V


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def compare(name, variants, flop, repeats, window_ms):
    iters = {}
    for label, fn in variants:
        for _ in range(5):
            fn()
        iters[label] = max(3, int(math.ceil(window_ms / max(timed(fn, 2), 1e-3))))
    ms = {label: [] for label, _ in variants}
    for _ in range(repeats):
        for label, fn in variants:
            ms[label].append(timed(fn, iters[label]))
    best = {k: min(v) for k, v in ms.items()}
    for label, fn in variants:
        print("%-9s %-8s %9.3f ms (spread %6.3f ms, %4d calls)  %6.1f TFLOP/s of %5.2f TFLOP  peak %9.1f MiB"
              % (name, label, best[label], max(ms[label]) - best[label], iters[label],
                 flop[label] / best[label] / 1e9, flop[label] / 1e12, peak_mib(fn)))
    if "unfused" in best:
        print("%-9s fused / unfused time %.3f" % (name, best["fused"] / best["unfused"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--shapes", default="0,1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("linear_xent_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd.ops import gemm as G
    from tensorflow_train_distributed_amd.ops import kernels as K
    from tensorflow_train_distributed_amd.ops import transformer as X
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    print("eager calls on one stream, %d alternating repeats, windows of about %.0f ms after 5 warm-up calls and a "
          "probe; best of the repeats" % (args.repeats, args.window_ms))
    for T, H, V in (SHAPES[int(i)] for i in args.shapes.split(",")):
        print("T = %d, H = %d, V = %d: a bf16 [T, V] tensor is %.1f MiB, the fused backward's chunk %d rows (%.1f MiB)"
              % (T, H, V, T * V * 2 / 2 ** 20, X.linear_xent_chunk_rows(V), X.linear_xent_chunk_rows(V) * V * 2 / 2 ** 20))
        g = torch.Generator(device=dev).manual_seed(0)
        h = torch.randn(T, H, device=dev, generator=g).to(bf)
        w = (torch.randn(V, H, device=dev, generator=g) * H ** -0.5).to(bf)
        bias = torch.randn(V, device=dev, generator=g)
        labels = torch.randint(0, V, (T,), device=dev, generator=g, dtype=torch.int32)
        dloss = torch.full((T,), 1.0 / T, device=dev)
        gsc = torch.full((1,), 1.0 / T, device=dev)
        sums = torch.zeros(2, device=dev)

        def fused_fwd():
            return X.linear_xent_fwd(h, w, labels, bias)

        def fused_all():
            loss, lse, _ = X.linear_xent_fwd(h, w, labels, bias)
            return (loss,) + X.linear_xent_bwd(h, w, labels, lse, dloss, bias)

        def unfused_fwd():
            logits = G.gemm(h, w, trans_b=True, bias=bias)
            X.xent_vocab(logits, V, labels, gsc, sums=sums)
            return sums

        def unfused_all():
            logits = G.gemm(h, w, trans_b=True, bias=bias)
            X.xent_vocab(logits, V, labels, gsc, dlogits=logits, sums=sums)
            return (sums, G.gemm(logits, w), G.gemm(logits, h, trans_a=True, out_dtype=torch.float32), K.colsum(logits))

        f = 2.0 * T * V * H
        sides = [("fused", fused_fwd, fused_all)]
        if T * V * 2 < 2 ** 31:
            sides.append(("unfused", unfused_fwd, unfused_all))
            sums.zero_()
            ours, ref = fused_all(), unfused_all()
            torch.cuda.synchronize()
            print("summed loss: fused %.6e, unfused (from bf16 logits) %.6e; dh: largest |fused - unfused| %.3e of "
                  "largest |dh| %.3e" % (float(ours[0].double().sum()), float(ref[0][0]),
                                         float((ours[1].float() - ref[1].float()).abs().max()),
                                         float(ref[1].float().abs().max())))
            del ours, ref
        else:
            print("unfused: not run (its bf16 logits are a %.2f GiB GEMM operand)" % (T * V * 2 / 2 ** 30))
        compare("fwd", [(n, a) for n, a, _ in sides], {n: f for n, _, _ in sides}, args.repeats, args.window_ms)
        compare("fwd+bwd", [(n, b) for n, _, b in sides], {n: 3 * f for n, _, _ in sides}, args.repeats, args.window_ms)


if __name__ == "__main__":
    main()
