#!/usr/bin/env python3
"""Standalone depthwise convolution kernels (depthwise.hip) at MobileNet-v1's depthwise layers, bf16,
batch 128, 3x3, TF SAME: time per call (HIP events after warm-up) and achieved bytes/s from the bytes
each kernel must move.

Bytes (bf16, 2 B per element; the fp32 filter and its gradient are not counted):
  forward          x read, y written          (N*H*W*C + N*P*Q*C) * 2
  data gradient    dy read, dx written        the same
  weight gradient  x and dy read              the same

Columns:
  fast     this project's kernels as dispatched (form="auto": the fast form at every layer here)
  generic  this project's kernels under form="generic"
  torch    F.conv2d(groups=C) on channels_last bf16 and aten.convolution_backward for one gradient at
           a time, symmetric padding 1 (TF SAME at stride 2 pads bottom / right only: the same bytes)
  copy     torch.add(a, 1, out=b) over (bytes / 4) bf16 elements: the same bytes, half read and half
           written — the bandwidth yardstick
Neither yardstick is the code under test. The variants alternate inside every repeat.
usage: python tools/dwconv_bench.py [--batch 128] [--repeats 3] [--window-ms 5] [--only fwd,dgrad,wgrad]"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (H = W, C, stride) of MobileNet-v1's depthwise layers at 224x224
LAYERS = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1),
          (14, 512, 2), (7, 1024, 1)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def compare(name, nbytes, variants, repeats, window_ms):
    """variants: [(label, fn)]. Warm up, size the timed window from a probe, alternate the variants."""
    iters = {}
    for label, fn in variants:
        for _ in range(5):
            fn()
        probe = timed(fn, 5)
        iters[label] = max(20, int(math.ceil(window_ms * 1e3 / max(probe, 1e-3))))
    us = {label: [] for label, _ in variants}
    for _ in range(repeats):
        for label, fn in variants:
            us[label].append(timed(fn, iters[label]))
    best = {k: min(v) for k, v in us.items()}
    cells = ["%s %8.1f us %5.2f TB/s (spread %4.1f us, %d it)" % (k, best[k], nbytes / best[k] / 1e6,
                                                                max(us[k]) - best[k], iters[k]) for k, _ in variants]
    print("%-22s %6.1f MB  %s" % (name, nbytes / 1e6, "   ".join(cells)))
    print("%-22s            fast / generic time %.2f   fast / torch time %.2f   share of the copy rate %.2f"
          % ("", best["fast"] / best["generic"], best["fast"] / best["torch"], best["copy"] / best["fast"]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--only", default="fwd,dgrad,wgrad")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dwconv_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd import nn as N
    from tensorflow_train_distributed_amd.ops import _plan
    from tensorflow_train_distributed_amd.ops import kernels as K
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    only = args.only.split(",")
    print("batch %d, bf16, 3x3 SAME, %d alternating repeats, timed windows of about %.0f ms after 5 warm-up "
          "launches and a 5-launch probe; best of the repeats" % (args.batch, args.repeats, args.window_ms))
    B = args.batch
    for H, C, s in LAYERS:
        geom = N._dw_geometry(H, H, 3, 3, (s, s), "SAME", (1, 1))
        P, Q = geom[6], geom[7]
        x = torch.randn(B, H, H, C, device=dev).to(bf)
        dy = torch.randn(B, P, Q, C, device=dev).to(bf)
        w = torch.randn(3, 3, C, 1, device=dev) * 0.3
        g = _plan.dw_geom(tuple(x.shape), tuple(w.shape), *geom)
        assert _plan.dw_fast_takes(g, True)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
        ws = K.dwconv_wgrad_workspace(tuple(x.shape), tuple(w.shape), geom, device=dev)
        nbytes = (x.numel() + dy.numel()) * 2
        a = torch.randn(nbytes // 4, device=dev).to(bf)
        b = torch.empty_like(a)
        # torch: logical NCHW tensors in channels_last memory (the same NHWC bytes)
        xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        wt = w.permute(2, 3, 0, 1).reshape(C, 1, 3, 3).to(bf).contiguous()
        assert xt.is_contiguous(memory_format=torch.channels_last)

        def t_bwd(mask):
            return lambda: torch.ops.aten.convolution_backward(dyt, xt, wt, None, [s, s], [1, 1], [1, 1], False,
                                                               [0, 0], C, mask)

        copy = ("copy", lambda: torch.add(a, 1.0, out=b))
        tag = "%dx%dx%d s%d" % (H, H, C, s)
        if "fwd" in only:
            compare(tag + " fwd", nbytes, [
                ("fast", lambda: K.dwconv_fwd(x, w, geom, out=y)),
                ("generic", lambda: K.dwconv_fwd(x, w, geom, out=y, form="generic")),
                ("torch", lambda: F.conv2d(xt, wt, stride=s, padding=1, groups=C)), copy], args.repeats,
                args.window_ms)
        if "dgrad" in only:
            compare(tag + " dgrad", nbytes, [
                ("fast", lambda: K.dwconv_dgrad(dy, w, tuple(x.shape), geom, out=dx)),
                ("generic", lambda: K.dwconv_dgrad(dy, w, tuple(x.shape), geom, out=dx, form="generic")),
                ("torch", t_bwd([True, False, False])), copy], args.repeats, args.window_ms)
        if "wgrad" in only:
            compare(tag + " wgrad", nbytes, [
                ("fast", lambda: K.dwconv_wgrad(x, dy, tuple(w.shape), geom, out=dw, workspace=ws)),
                ("generic", lambda: K.dwconv_wgrad(x, dy, tuple(w.shape), geom, out=dw, workspace=ws,
                                                   form="generic")),
                ("torch", t_bwd([False, True, False])), copy], args.repeats, args.window_ms)
        del x, dy, y, dx, a, b


if __name__ == "__main__":
    main()
