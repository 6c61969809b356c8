#!/usr/bin/env python3
"""Standalone RMSNorm and SwiGLU kernels (rmsnorm_glu.hip) at the BERT-Large b128 sizes, as the
engine calls them under BertConfig(rms_norm=True, gated_ffn=True): time per call (HIP events after
warm-up) and achieved bytes/s from the bytes each kernel must move.

Bytes (bf16, 2 B per element; the per-row statistics and gamma are not counted):
  norm forward, residual form    x, res read; s, y written            4 * tokens * H * 2
  norm forward, plain            x read; y written                    2 * tokens * H * 2
  norm backward with dx          dy, s read; ds, dx written           4 * tokens * H * 2
  norm backward, ds only         dy, s read; ds written               3 * tokens * H * 2
  SwiGLU forward                 x2 [tokens, 2I] read; h written      3 * tokens * I * 2
  SwiGLU backward                dh, x2 read; dx2 [tokens, 2I] written  5 * tokens * I * 2

Yardsticks, neither of them the code under test:
  RMSNorm     this project's LayerNorm forward / backward at the same shape and dropout settings (it
              moves the same activation bytes, with a second reduction and the mean / beta traffic);
  SwiGLU fwd  torch.add(a, b, out=h) over the gate / value / output views: the forward's bytes;
  SwiGLU bwd  torch.add(x2 as [tokens, 2, I], dh as [tokens, 1, I], out=dx2 as [tokens, 2, I]): the
              backward's writes and reads, except that dh is read once per half (the second read of
              a row can hit in cache).
The [tokens, I] and [tokens, 2I] operands are row-padded column views, as in the engine.
usage: python tools/norm_glu_bench.py [--tokens 65536] [--hidden 1024] [--inter 4096] [--pad 256]
                                      [--iters 200] [--repeats 3] [--only all|norm|swiglu]"""
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


def compare(name, nbytes, ours, ours_fn, yard, yard_fn, iters, repeats):
    a_us, b_us = [], []
    for _ in range(repeats):
        a_us.append(timed(ours_fn, iters))
        b_us.append(timed(yard_fn, iters))
    for r, (a, b) in enumerate(zip(a_us, b_us)):
        print("%-34s run %d  %s %8.1f us %6.2f TB/s   %s %8.1f us %6.2f TB/s"
              % (name, r + 1, ours, a, nbytes / a / 1e6, yard, b, nbytes / b / 1e6))
    a, b = min(a_us), min(b_us)
    print("%-34s best   %s %8.1f us %6.2f TB/s   %s %8.1f us %6.2f TB/s   rate / yardstick rate %.2f   "
          "spread %.1f / %.1f us   (%.0f MB per call)"
          % (name, ours, a, nbytes / a / 1e6, yard, b, nbytes / b / 1e6, b / a, max(a_us) - a, max(b_us) - b,
             nbytes / 1e6))


def bench_norms(T, args, dev):
    rows, H, bf = args.tokens, args.hidden, torch.bfloat16
    x, res, dy = [torch.randn(rows, H, device=dev).to(bf) for _ in range(3)]
    gamma, beta = torch.randn(H, device=dev) * 0.5 + 1, torch.randn(H, device=dev) * 0.1
    rng = T.RngState(7, dev)
    y, s, ds, dx = [torch.empty_like(x) for _ in range(4)]
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    dg, db = torch.empty(H, device=dev), torch.empty(H, device=dev)
    ln_work, rms_work = T.ln_bwd_workspace(rows, H, dev), T.rmsnorm_bwd_workspace(rows, H, dev)
    act = rows * H * 2
    for label, kw, fwd_n, bwd_n in [("residual + p_in 0.1", dict(p_in=0.1, site_in=3, rng=rng), 4, 4),
                                    ("plain", dict(), 2, 3)]:
        r = res if kw else None
        want_dx = bool(kw)
        compare("norm fwd, " + label, fwd_n * act, "rms",
                lambda: T.rmsnorm_fwd(x, gamma, res=r, out=y, s_out=s if kw else None, rstd=rstd, **kw), "layernorm",
                lambda: T.layernorm_fwd(x, gamma, beta, res=r, out=y, s_out=s if kw else None, mean=mean, rstd=rstd,
                                        **kw), args.iters, args.repeats)
        sv = s if kw else x
        T.layernorm_fwd(x, gamma, beta, res=r, out=y, s_out=s if kw else None, mean=mean, rstd=rstd, **kw)
        compare("norm bwd, " + label, bwd_n * act, "rms",
                lambda: T.rmsnorm_bwd(dy, sv, rstd, gamma, dg, ds_out=ds, want_dx=want_dx, dx_out=dx, work=rms_work,
                                      **kw), "layernorm",
                lambda: T.layernorm_bwd(dy, sv, mean, rstd, gamma, dg, db, ds_out=ds, want_dx=want_dx, dx_out=dx,
                                        work=ln_work, **kw), args.iters, args.repeats)


def bench_swiglu(T, args, dev):
    rows, I, pad, bf = args.tokens, args.inter, args.pad, torch.bfloat16

    def padded(width):
        buf = torch.randn(rows, width + pad, device=dev).to(bf)
        return buf[:, :width] if pad else buf

    x2, dx2, h, dh = padded(2 * I), padded(2 * I), padded(I), padded(I)
    a, b = x2[:, :I], x2[:, I:]
    esz = 2
    compare("swiglu fwd", 3 * rows * I * esz, "swiglu", lambda: T.swiglu_fwd(x2, out=h), "torch.add",
            lambda: torch.add(a, b, out=h), args.iters, args.repeats)
    x3, d3, o3 = x2.unflatten(1, (2, I)), dh.unsqueeze(1), dx2.unflatten(1, (2, I))
    compare("swiglu bwd", 5 * rows * I * esz, "swiglu", lambda: T.swiglu_bwd(dh, x2, out=dx2), "torch.add",
            lambda: torch.add(x3, d3, out=o3), args.iters, args.repeats)
    # in place over the forward's input, as the engine calls it: repeated passes over their own
    # output change the values, not the bytes moved
    compare("swiglu bwd in place", 5 * rows * I * esz, "swiglu", lambda: T.swiglu_bwd(dh, x2, out=x2), "torch.add_",
            lambda: x3.add_(d3), args.iters, args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--inter", type=int, default=4096)
    ap.add_argument("--pad", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="all", choices=["all", "norm", "swiglu"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("norm_glu_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    rows, H, I, pad = args.tokens, args.hidden, args.inter, args.pad
    print("tokens %d, H %d, I %d (row pad %d), %d timed launches per figure after 10 warm-up launches, "
          "%d alternating repeats" % (rows, H, I, pad, args.iters, args.repeats))

    if args.only in ("all", "norm"):
        bench_norms(T, args, dev)
    if args.only in ("all", "swiglu"):
        bench_swiglu(T, args, dev)


if __name__ == "__main__":
    main()
