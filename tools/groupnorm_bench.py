#!/usr/bin/env python3
"""Standalone group normalisation kernels (groupnorm.hip), bf16, G = 32, at the normalisation sites of
ResNet-50-GN at batch 32 and at two diffusion-UNet shapes: time per call (HIP events around replays of a
hipGraph of 10 recorded calls, after warm-up; a variant that cannot be captured is timed eagerly and
marked) and the share it reaches of the rate a torch.add over the same bytes gets on the same GPU.

Bytes (bf16, 2 B per element; the fp32 statistics, parameters and partial rows are not counted):
  forward   x read twice (statistics, apply), y written once          3 * N*M*C * 2
  backward  dy and x read twice (sums, apply), dx written once        5 * N*M*C * 2

Columns:
  fast     this project's kernels as dispatched (form="auto": the fast form at every shape here)
  generic  this project's kernels under form="generic"
  torch    F.group_norm on a channels_last bf16 tensor (logical NCHW over the same NHWC bytes) and
           autograd's backward of it for all three gradients
  copy     torch.add(a, 1, out=b) over bytes / 4 bf16 elements: the same bytes, half read and half
           written — the bandwidth yardstick
Neither yardstick is the code under test. The variants alternate inside every repeat.
usage: python tools/groupnorm_bench.py [--batch 32] [--repeats 3] [--window-ms 5] [--only fwd,bwd]"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (H = W, C): ResNet-50-GN, then the UNet shapes
SHAPES = [(56, 64), (56, 256), (28, 512), (14, 1024), (7, 2048), (64, 320), (32, 640)]
GROUPS = 32
EPS = 1e-3


GRAPH_CALLS = 10  # calls recorded into one hipGraph


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def graphed(fn):
    """A replay of GRAPH_CALLS recorded calls of fn, so that what is timed is the kernels and not
    the Python and ctypes work of launching them (about 20 us for three launches). None if fn
    cannot be captured."""
    g = torch.cuda.CUDAGraph()
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(g):
            for _ in range(GRAPH_CALLS):
                fn()
    except Exception:  # the variant stays eager and is marked so
        torch.cuda.synchronize()
        return None
    return g.replay


def compare(name, nbytes, variants, repeats, window_ms):
    """variants: [(label, fn)] or (label, fn, "eager"). Warm up, capture, size the timed window from a probe, alternate the
    variants. Times are per call."""
    iters, run, per = {}, {}, {}
    eager = {v[0] for v in variants if len(v) > 2}
    variants = [v[:2] for v in variants]
    for label, fn in variants:
        for _ in range(5):
            fn()
        replay = None if label in eager else graphed(fn)
        run[label], per[label] = (replay, GRAPH_CALLS) if replay is not None else (fn, 1)
        probe = timed(run[label], 5) / per[label]
        iters[label] = max(20 // per[label] + 1, int(math.ceil(window_ms * 1e3 / max(probe, 1e-3) / per[label])))
    us = {label: [] for label, _ in variants}
    for _ in range(repeats):
        for label, _ in variants:
            us[label].append(timed(run[label], iters[label]) / per[label])
    best = {k: min(v) for k, v in us.items()}
    cells = ["%s%s %8.1f us %5.2f TB/s (spread %4.1f us, %d calls)"
             % (k, "" if per[k] > 1 else " (eager)", best[k], nbytes / best[k] / 1e6, max(us[k]) - best[k],
                iters[k] * per[k]) for k, _ in variants]
    print("%-18s %6.1f MB  %s" % (name, nbytes / 1e6, "   ".join(cells)))
    print("%-18s            fast / generic time %.2f   fast / torch time %.2f   share of the copy rate %.2f"
          % ("", best["fast"] / best["generic"], best["fast"] / best["torch"], best["copy"] / best["fast"]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--only", default="fwd,bwd")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("groupnorm_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd.ops import _plan
    from tensorflow_train_distributed_amd.ops import kernels as K
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    only = args.only.split(",")
    print("batch %d, bf16, G = %d, %d alternating repeats, timed windows of about %.0f ms after 5 warm-up "
          "launches and a probe, each call replayed from a hipGraph of %d; best of the repeats" % (args.batch, GROUPS, args.repeats, args.window_ms, GRAPH_CALLS))
    B, G = args.batch, GROUPS
    for H, C in SHAPES:
        M = H * H
        x = torch.randn(B, M, C, device=dev).to(bf)
        dy = torch.randn(B, M, C, device=dev).to(bf)
        gamma = torch.rand(C, device=dev) + 0.5
        beta = torch.randn(C, device=dev)
        assert _plan.gn_fast_takes(B, M, C, G, True)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = torch.empty(B, G, device=dev), torch.empty(B, G, device=dev)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        fws, bws = K.group_norm_fwd_workspace(B, M, C, dev), K.group_norm_bwd_workspace(B, M, C, dev)
        K.group_norm_fwd(x, gamma, beta, G, EPS, out=y, workspace=fws, stats=(mean, rstd))
        # torch: logical NCHW tensors in channels_last memory (the same NHWC bytes)
        xt = x.view(B, H, H, C).permute(0, 3, 1, 2)
        dyt = dy.view(B, H, H, C).permute(0, 3, 1, 2)
        assert xt.is_contiguous(memory_format=torch.channels_last)
        gb, bb = gamma.to(bf).requires_grad_(True), beta.to(bf).requires_grad_(True)
        xg = xt.detach().requires_grad_(True)
        yt = F.group_norm(xg, G, gb, bb, EPS)  # the graph torch's backward is timed on
        tag = "%dx%dx%d (T = %d)" % (H, H, C, _plan.gn_parts(B, M, C))
        for which, mult in (("fwd", 3), ("bwd", 5)):
            if which not in only:
                continue
            nbytes = mult * x.numel() * 2
            a = torch.randn(nbytes // 4, device=dev).to(bf)
            b = torch.empty_like(a)
            copy = ("copy", lambda: torch.add(a, 1.0, out=b))
            if which == "fwd":
                variants = [
                    ("fast", lambda: K.group_norm_fwd(x, gamma, beta, G, EPS, out=y, workspace=fws, stats=(mean, rstd))),
                    ("generic", lambda: K.group_norm_fwd(x, gamma, beta, G, EPS, out=y, workspace=fws,
                                                         stats=(mean, rstd), form="generic")),
                    ("torch", lambda: F.group_norm(xt, G, gb.detach(), bb.detach(), EPS)), copy]
            else:
                variants = [
                    ("fast", lambda: K.group_norm_bwd(dy, x, gamma, mean, rstd, dg, db, out=dx, workspace=bws)),
                    ("generic", lambda: K.group_norm_bwd(dy, x, gamma, mean, rstd, dg, db, out=dx, workspace=bws,
                                                         form="generic")),
                    # autograd's engine is not recorded into a graph here: timed eagerly, one launch sequence per call
                    ("torch", lambda: torch.autograd.grad(yt, (xg, gb, bb), dyt, retain_graph=True), "eager"), copy]
            compare(tag + " " + which, nbytes, variants, args.repeats, args.window_ms)
            del a, b
        del x, dy, y, dx


if __name__ == "__main__":
    main()
