#!/usr/bin/env python3
"""A/B of the halo 3x3 kernels (conv3_halo.hip), interleaved rounds in one process, median us.

Part 1, three arms of the kernels, interleaved per variant and round:

  sched0   the predecessor schedule                      set_conv3_sched(0)
  feed0    the current schedule, generic epilogue        set_conv3_sched(1), set_conv3_feed(0)
  new      the current schedule, prefetched feeding-BN   set_conv3_sched(1), set_conv3_feed(1)
           epilogue of the data gradients

on the launches the ResNet-50 step runs, at stage 2 (56x56, 64 -> 64) and stage 3 (28x28, 128 -> 128):

  fwdbn_c3   BN apply + ReLU prologue, conv, BN statistics     conv3_halo(bn_fwd, stat)
  dg_c3      data gradient with the feeding-BN epilogue        conv3_halo(flip, bn_stat)
  dgrad_c3   (stage 2) the same with the BN backward as prologue (TTD_C3_DGRAD=1)

with, per variant and arm: median us, max - min over the rounds, us per tile per workgroup,
and the two per-tile floors from the shapes (MFMA: 4096 bf16 FLOP/clk/CU at 2.4 GHz; HBM: the
tile's halo, output, side tensors and bits at a 1/CUs share of 5 TB/s), and feed0 -> new judged by
the rule "faster when the new median is below the old one by more than three times the larger
max - min spread of the two arms".

Part 2 (stage 2, as before): the halo kernel against the paths it replaces

  fwd     plain conv + BN statistics                 conv_fwd(stat)                vs conv3_halo(stat)
  fwdbn   BN apply + ReLU, then conv + statistics    bn_apply + conv_fwd(stat)     vs conv3_halo(bn_fwd)
  dgrad   BN bwd-apply, then dgrad w/ BN-stat epi    bn_bwd_apply + conv_dgrad     vs conv3_halo(flip, bn_bwd)

usage: python tools/conv3_bench.py [--batch 1024] [--rounds 5] [--no-paths]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CLK_HZ, MFMA_FLOP_PER_CLK_CU, HBM_BPS = 2.4e9, 4096, 5.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-paths", action="store_true", help="skip part 2")
    args = ap.parse_args()
    from tensorflow_train_distributed_amd.ops import _lib
    from tensorflow_train_distributed_amd.ops import gemm as G
    from tensorflow_train_distributed_amd.ops import kernels as K
    dev = "cuda"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wgs = cus // 8 * 8

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def timeit(fn, n=3):
        s, e = ev(), ev()
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / n * 1e3

    def tensors(B, H, W, C):
        M = B * H * W
        t = {"x": torch.randn(B, H, W, C, device=dev).bfloat16(),
             "w": (torch.randn(C, 3, 3, C, device=dev) / (9 * C) ** 0.5).bfloat16(),
             "sc": torch.rand(C, device=dev) + 0.5, "sh": torch.randn(C, device=dev) * 0.1,
             "hm": torch.empty(M * C // 8, dtype=torch.uint8, device=dev),
             "g": torch.randn(B, H, W, C, device=dev).bfloat16(), "y": torch.randn(B, H, W, C, device=dev).bfloat16(),
             "coef": torch.randn(3, C, device=dev) * 0.1, "fy": torch.randn(B, H, W, C, device=dev).bfloat16(),
             "fm": torch.randint(0, 256, (M * C // 8,), dtype=torch.uint8, device=dev)}
        t["wt"] = K.krsc_to_crsk(t["w"])
        t["h"] = torch.empty_like(t["x"])
        t["dz"] = torch.randn(B, H, W, C, device=dev).bfloat16()
        return t

    # ---- part 1: old vs new schedule on the in-step launches
    B = args.batch
    sched = {}   # (stage, variant) -> (fn, tile rows, HBM bytes per tile)
    keep = []
    for stage, (H, W, C) in ((2, (56, 56, 64)), (3, (28, 28, 128))):
        t = tensors(B, H, W, C)
        keep.append(t)
        px = C * 2  # bytes per pixel of a bf16 NHWC tensor; the ReLU bits are px / 16

        def halo(rows, th):
            return (th + 2) * W / (th * W) * rows * W * px

        r8 = G.conv3_rows(H, W, C, C, 1) // W
        sched[(stage, "fwdbn_c3")] = (
            lambda t=t: G.conv3_halo(t["x"], t["w"], prologue=("bn_fwd", t["sc"], t["sh"], t["h"], t["hm"]), stat=True),
            r8, halo(r8, r8) + r8 * W * (2 * px + px / 16))                # halo in; out, side, side bits out
        sched[(stage, "dg_c3")] = (
            lambda t=t: G.conv3_halo(t["dz"], t["wt"], flip=True, bn_stat=(t["fy"], t["fm"])),
            r8, halo(r8, r8) + r8 * W * (2 * px + px / 16))                # halo, y, bits in; out
        if stage == 2:
            r4 = G.conv3_rows(H, W, C, C, 2) // W
            sched[(stage, "dgrad_c3")] = (
                lambda t=t: G.conv3_halo(t["g"], t["wt"], flip=True, prologue=("bn_bwd", t["y"], None, t["coef"], t["dz"]),
                                         bn_stat=(t["fy"], t["fm"])),
                r4, 2 * halo(r4, r4) + r4 * W * (3 * px + px / 16))        # g, y halos; fy, bits in; dz, out
    arms = (("sched0", False, False), ("feed0", True, False), ("new", True, True))  # (label, sched, feed)
    res = {(k, a[0]): [] for k in sched for a in arms}
    prev = G.set_conv3_sched(True)
    prev_feed = G.set_conv3_feed(True)
    for _ in range(args.rounds):
        for k, (fn, _, _) in sched.items():
            for label, s, f in arms:
                G.set_conv3_sched(s)
                G.set_conv3_feed(f)
                fn()
                res[(k, label)].append(timeit(fn))
    G.set_conv3_sched(prev)
    G.set_conv3_feed(prev_feed)
    print("%-5s %-9s %-6s %9s %8s %12s %10s %9s %7s" % ("stage", "variant", "arm", "median us", "max-min", "us/tile/wg",
                                                           "MFMA floor", "HBM floor", "TF/s"))
    tot = {a[0]: 0.0 for a in arms}
    for (stage, name), (_, rows, nbytes) in sched.items():
        H, W, C = {2: (56, 56, 64), 3: (28, 28, 128)}[stage]
        tiles = -(-B * H // rows)
        per_wg = -(-tiles // wgs)
        f_mfma = 2.0 * rows * W * C * 9 * C / MFMA_FLOP_PER_CLK_CU / CLK_HZ * 1e6
        f_hbm = nbytes / (HBM_BPS / cus) * 1e6
        for label, _, _ in arms:
            v = res[((stage, name), label)]
            med = statistics.median(v)
            if name != "dgrad_c3":
                tot[label] += med
            print("%-5d %-9s %-6s %9.1f %8.1f %12.2f %10.2f %9.2f %7.0f" % (
                stage, name, label, med, max(v) - min(v), med / per_wg, f_mfma, f_hbm,
                2.0 * B * H * W * C * 9 * C / med / 1e6), flush=True)
        o, nw = res[((stage, name), "feed0")], res[((stage, name), "new")]
        gain = statistics.median(o) - statistics.median(nw)
        spread = max(max(o) - min(o), max(nw) - min(nw))
        print("%-5d %-9s feed0 -> new: %+.1f us, spread %.1f us: %s" % (
            stage, name, -gain, spread, "faster" if gain > 3 * spread else "slower" if -gain > spread else "same"),
            flush=True)
    print("sum of the four in-step variants (fwdbn_c3, dg_c3 at both stages): " +
          ", ".join("%s %.1f us" % (a[0], tot[a[0]]) for a in arms), flush=True)
    if args.no_paths:
        return

    # ---- part 2: the halo kernel against the paths it replaces (stage 2)
    t = keep[0]
    H, W, C, N = 56, 56, 64, 64
    M = B * H * W
    x, w, wt, sc, sh, h, hm = t["x"], t["w"], t["wt"], t["sc"], t["sh"], t["h"], t["hm"]
    g, y, coef, dz, fy, fm = t["g"], t["y"], t["coef"], t["dz"], t["fy"], t["fm"]
    bm = 128
    part = torch.empty((-(-M // bm), 2, N), device=dev)
    variants = {
        "fwd_old": lambda: G.conv_fwd(x, w, (1, 1), (1, 1), stat=part, tile=(bm, 64)),
        "fwd_c3": lambda: G.conv3_halo(x, w, stat=True),
        "fwdbn_old": lambda: (K.bn_apply(x.view(M, C), sc, sh, relu=True, out=h.view(M, C), mask=hm),
                              G.conv_fwd(h, w, (1, 1), (1, 1), stat=part, tile=(bm, 64))),
        "fwdbn_c3": lambda: G.conv3_halo(x, w, prologue=("bn_fwd", sc, sh, h, hm), stat=True),
        "dgrad_old": lambda: (_lib.call("ttdk_bn_bwd_apply", g.data_ptr(), None, None, y.data_ptr(), coef.data_ptr(),
                                        dz.data_ptr(), M * N, N, _lib.stream()),
                              G.conv_dgrad(dz, wt, (B, H, W, C), (1, 1), (1, 1), bn_stat=(fy, fm))),
        "dgrad_c3": lambda: G.conv3_halo(g, wt, flip=True, prologue=("bn_bwd", y, None, coef, dz), bn_stat=(fy, fm)),
        "dgrad_c3p0": lambda: (_lib.call("ttdk_bn_bwd_apply", g.data_ptr(), None, None, y.data_ptr(), coef.data_ptr(),
                                         dz.data_ptr(), M * N, N, _lib.stream()),
                               G.conv3_halo(dz, wt, flip=True, bn_stat=(fy, fm))),
        "dg_gemm": lambda: G.conv_dgrad(dz, wt, (B, H, W, C), (1, 1), (1, 1), bn_stat=(fy, fm)),
        "dg_c3": lambda: G.conv3_halo(dz, wt, flip=True, bn_stat=(fy, fm)),
    }
    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            fn()
            res[k].append(timeit(fn))
    flop = 2.0 * M * N * 9 * C
    for k in variants:
        tm = statistics.median(res[k])
        print("%-10s %8.1f us  %6.0f TF/s" % (k, tm, flop / tm / 1e6), flush=True)


if __name__ == "__main__":
    main()
