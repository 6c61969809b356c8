#!/usr/bin/env python3
"""The routing pieces of a mixture-of-experts block (moe_route.hip through ops.moe) against the
torch expressions layers.MixtureOfExperts used for them before; the grouped matmuls are not timed.

  top-k      softmax -> topk -> renormalise, and its backward from dgate and dprobs
  sort       argsort(stable) + argsort + bincount + cumsum + pad  vs  the counting sort
  dispatch   xs = x[order // k] and back dx = d[inv].reshape(T, k, D).sum(1)              (bf16)
  combine    y = (h[inv].reshape(T, k, D).float() * gate[..., None]).sum(1) and its backward for h and
             gate (h bf16, y fp32)

Time per call: HIP events around a window of eager calls on one stream, after 5 warm-up calls and a
probe that sizes the window; the two sides alternate in every repeat; best of the repeats, with the
spread (worst - best). Launches per call are counted once with torch.profiler. For the two
streaming pieces the bytes that must move (every operand read once, every result written once):
  dispatch   x and dxs read, xs and dx written, bf16     2 * (T + T*k) * D * 2
  combine    h read twice and dh written (bf16), y written and dy read (fp32)     3 * T*k*D * 2 + 2 * T*D * 4
usage: python tools/moe_route_bench.py [--repeats 3] [--window-ms 250]"""
import argparse
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(16384, 8, 2, 4096), (16384, 64, 4, 2048)]  # T, E, k, D


def nbytes(piece, T, k, D):
    S = T * k
    if piece == "dispatch":  # x -> xs; dxs -> dx, all bf16
        return 2 * (T * D + S * D) * 2
    if piece == "combine":   # h (bf16) -> y (fp32); dy (fp32), h -> dh (bf16)
        return (S * D * 2 + T * D * 4) + (T * D * 4 + S * D * 2 + S * D * 2)
    return None


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def launches(fn):
    """Kernels one call launches, from a profiler trace; a trace without kernels is an error."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    if n == 0:
        raise RuntimeError("the profiler recorded no kernel: launches per call cannot be counted")
    return n


def compare(name, variants, moved, repeats, window_ms):
    iters = {}
    for label, fn in variants:
        for _ in range(5):
            fn()
        iters[label] = max(10, int(math.ceil(window_ms * 1e3 / max(timed(fn, 5), 1e-3))))
    us = {label: [] for label, _ in variants}
    for _ in range(repeats):
        for label, fn in variants:
            us[label].append(timed(fn, iters[label]))
    best = {k: min(v) for k, v in us.items()}
    for label, fn in variants:
        n = launches(fn)
        rate = "" if moved is None else "  %5.2f TB/s of %6.1f MB" % (moved / best[label] / 1e6, moved / 1e6)
        print("%-10s %-6s %9.1f us (spread %6.1f us, %5d calls)  launches %-4d%s"
              % (name, label, best[label], max(us[label]) - best[label], iters[label], n, rate))
    print("%-10s ours / torch time %.3f" % (name, best["ours"] / best["torch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=250.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_route_bench.py needs a GPU: nothing is measured without one")
    from tensorflow_train_distributed_amd import nn as N
    from tensorflow_train_distributed_amd.ops import moe as M
    dev, bf = torch.device("cuda", 0), torch.bfloat16
    print("eager calls on one stream, %d alternating repeats, windows of about %.0f ms after 5 warm-up calls and a "
          "probe; best of the repeats" % (args.repeats, args.window_ms))
    for T, E, k, D in SHAPES:
        print("T = %d, E = %d, k = %d, D = %d" % (T, E, k, D))
        g = torch.Generator(device=dev).manual_seed(0)
        logits = (4 * torch.randn(T, E, device=dev, generator=g)).requires_grad_()
        dgate, dprobs = torch.randn(T, k, device=dev, generator=g), torch.randn(T, E, device=dev, generator=g)
        x = torch.randn(T, D, device=dev, generator=g).to(bf)
        h = torch.randn(T * k, D, device=dev, generator=g).to(bf).requires_grad_()
        dxs, dy = torch.randn(T * k, D, device=dev, generator=g).to(bf), torch.randn(T, D, device=dev, generator=g)
        probs, expert, gate = M.topk_route(logits.detach(), k)
        offsets, order, inv = M.sort_by_expert(expert, E)
        slots, order64, inv64 = expert.reshape(-1).long(), order.long(), inv.long()
        gate_t = gate.clone().requires_grad_()

        def topk_torch():
            p = torch.softmax(logits, dim=-1)
            gt, _ = torch.topk(p, k, dim=-1)
            gt = gt / gt.sum(-1, keepdim=True)
            return torch.autograd.grad((gt, p), logits, (dgate, dprobs))

        def topk_ours():
            p, e, gt = M.topk_route(logits.detach(), k)
            return M.topk_route_bwd(p, e, gt, dgate, dprobs)

        def sort_torch():
            o = torch.argsort(slots, stable=True)
            return F.pad(torch.cumsum(torch.bincount(slots, minlength=E), 0, dtype=torch.int32), (1, 0)), o, torch.argsort(o)

        def dispatch_torch():
            return x[order64 // k], dxs[inv64].reshape(T, k, D).sum(1)

        def dispatch_ours():
            return M.gather_rows(x, order, k), M.combine_rows(dxs, inv, k, dtype=bf)

        def combine_torch():
            y = (N._GatherRows.apply(h, inv64, order64, 1).reshape(T, k, -1).float() * gate_t.unsqueeze(-1)).sum(1)
            return torch.autograd.grad(y, (h, gate_t), dy)

        def combine_ours():
            return M.combine_rows(h.detach(), inv, k, w=gate), M.gather_rows(dy, order, k, scale=gate, h=h.detach(), dtype=bf)

        for name, ours, ref in (("top-k", topk_ours, topk_torch), ("sort", lambda: M.sort_by_expert(expert, E), sort_torch),
                                ("dispatch", dispatch_ours, dispatch_torch), ("combine", combine_ours, combine_torch)):
            compare(name, [("ours", ours), ("torch", ref)], nbytes(name, T, k, D), args.repeats, args.window_ms)


if __name__ == "__main__":
    main()
