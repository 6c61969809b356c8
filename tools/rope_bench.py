#!/usr/bin/env python3
"""Standalone rotary-embedding kernel (rope.hip), in place on the [q | k] columns of a fused
[tokens, width] QKV buffer as the BERT engine and MultiHeadAttention(rotary=True) call it:
time per call (HIP events after warm-up) and achieved bytes/s, counting the rotated columns read
once and written once (the 2 x 256 B of cos / sin per row chunk come from a table that stays in
cache and are not counted).

Yardstick on the same view: torch's in-place mul_(1.0) over the same columns. It moves the same
bytes through the same strided rows and is not the code under test.

Shapes: BERT-Large b128 (65536 tokens, S 512, H = 1024: 32 rotated heads of a 3072-wide bf16
buffer), forward and inverse; a grouped-query shape (32 query + 8 key heads rotated of a
(32 + 2*8)*64 = 3072-wide buffer); the BERT shape in fp32.
usage: python tools/rope_bench.py [--tokens 65536] [--seq 512] [--iters 200] [--repeats 3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rope_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    tokens, S = args.tokens, args.seq
    table = T.rope_table(S, device=dev)
    cases = [
        ("bert-large b128 bf16 fwd", torch.bfloat16, 3072, 32, False),
        ("bert-large b128 bf16 inverse", torch.bfloat16, 3072, 32, True),
        ("grouped H=32 Hk=8 bf16 fwd", torch.bfloat16, 3072, 40, False),
        ("bert-large b128 fp32 fwd", torch.float32, 3072, 32, False),
    ]
    print("tokens %d, S %d, %d timed launches per figure after 10 warm-up launches, %d alternating repeats"
          % (tokens, S, args.iters, args.repeats))
    for name, dt, width, heads, inverse in cases:
        qkv = torch.randn(tokens, width, device=dev).to(dt)
        view = qkv[:, :heads * 64]
        nbytes = 2 * tokens * heads * 64 * qkv.element_size()
        rope_us, mul_us = [], []
        for _ in range(args.repeats):
            rope_us.append(timed(lambda: T.rope(qkv, qkv, table, S, heads, inverse=inverse), args.iters))
            mul_us.append(timed(lambda: view.mul_(1.0), args.iters))
        for r, (a, b) in enumerate(zip(rope_us, mul_us)):
            print("%-30s run %d  rope %8.1f us %6.2f TB/s   torch mul_(1.0) %8.1f us %6.2f TB/s"
                  % (name, r + 1, a, nbytes / a / 1e6, b, nbytes / b / 1e6))
        a, b = min(rope_us), min(mul_us)
        print("%-30s best   rope %8.1f us %6.2f TB/s   torch mul_(1.0) %8.1f us %6.2f TB/s   "
              "rope rate / yardstick rate %.2f   (%.0f MB per call)"
              % (name, a, nbytes / a / 1e6, b, nbytes / b / 1e6, b / a, nbytes / 1e6))
        del qkv, view


if __name__ == "__main__":
    main()
