"""The persistent loop of the halo 3x3 kernels (csrc/kernels/conv3_halo.hip): runs in which some
workgroups walk three or more tiles and others fewer, which tests/test_kernels_conv3.py (at most
one tile per workgroup) never reaches. The prefetch of the next tile's halo, the streamed filter's
double buffer and the halo / staging reuse across tiles are all exercised here only.

Sizes come from the device's CU count (one workgroup per CU). At 256 CUs: 75 images of 56x56x64
(525 tiles of 8 rows, 1050 of 4 rows with the BN-backward prologue) and 147 images of 28x28x128
(515 tiles of 8 flattened rows, tiles straddling images, the last one 4 rows).

Per case:
* output against the fp32 convolution of the same bf16 input (relative to max 1e-2), or, with the
  feeding-BN epilogue, against conv_dgrad(bn_stat=...) (2e-2; sums rtol 2e-2): the tolerances of
  tests/test_kernels_conv3.py;
* side / side_mask of the BN-forward prologue bit-identical to bn_apply, side of the BN-backward
  prologue against ttdk_bn_bwd_apply;
* schedule independence, bit for bit: the output and per-tile statistics rows of the first, a
  middle and the last tile-aligned slice of images equal the same kernel run on that slice alone
  (one tile per workgroup);
* both settings of ops.gemm.set_conv3_sched give bit-identical output, side, bits and statistics.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _ops():
    from tensorflow_train_distributed_amd.ops import _lib
    from tensorflow_train_distributed_amd.ops import gemm as G
    from tensorflow_train_distributed_amd.ops import kernels as K
    return G, K, _lib


def _rand(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def _workgroups():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


# (name, stage, prologue, flip, epilogue)
CASES = [
    ("c3_fwd_stat", 2, None, False, "stat"),
    ("c3_bnfwd_stat", 2, "bn_fwd", False, "stat"),
    ("c3_dgrad_bnstat", 2, None, True, "bn_stat"),
    ("c3_bnbwd_dgrad_bnstat", 2, "bn_bwd", True, "bn_stat"),
    ("c3s_fwd", 3, None, False, "stat"),
    ("c3s_bnfwd_stat", 3, "bn_fwd", False, "stat"),
    ("c3s_dgrad_bnstat", 3, None, True, "bn_stat"),
]


def _geometry(stage, pro):
    """(images, H, W, C, slice length in images, slice starts) with more than two tiles per
    workgroup for some workgroups and fewer for the rest; a slice alone is one tile per workgroup."""
    wg = _workgroups()
    if stage == 2:
        tpi = 14 if pro == "bn_bwd" else 7      # tiles per image (4- / 8-row tiles)
        n = 2 * wg // 7 + 2                     # 7 n tiles of 8 rows in (2 wg, 3 wg)
        k = max(1, min(3, wg // tpi))
        assert 2 * wg < 7 * n < 3 * wg
        return n, 56, 56, 64, k, [0, n // 2, n - k]
    n = (4 * wg // 7 + 1) | 1                   # odd: 28 n rows end in a 4-row tile
    assert -(-28 * n // 8) > 2 * wg and (28 * n) % 8 == 4
    # even image offsets are tile boundaries (56 rows = 7 tiles); the last slice is the odd image
    return n, 28, 28, 128, 2, [0, (n // 2) & ~1, n - 1]


def _inputs(stage, pro, flip, epi):
    n, H, W, C, _, _ = _geometry(stage, pro)
    s = 100 * stage + 10 * (pro is not None) + flip
    d = {"x": _rand((n, H, W, C), seed=s + 1), "w": _rand((C, 3, 3, C), scale=(9 * C) ** -0.5, seed=s + 2)}
    g = torch.Generator(device="cuda").manual_seed(s + 3)
    if pro == "bn_fwd":
        d["sc"] = torch.rand(C, generator=g, device="cuda") + 0.5
        d["sh"] = torch.randn(C, generator=g, device="cuda") * 0.2
    if pro == "bn_bwd":
        d["y"] = _rand((n, H, W, C), seed=s + 4)
        d["coef"] = torch.randn(3, C, generator=g, device="cuda") * torch.tensor([[1.0], [0.1], [0.05]], device="cuda")
    if epi == "bn_stat":
        d["fy"] = _rand((n, H, W, C), seed=s + 5)
        d["fm"] = torch.randint(0, 256, (n * H * W * C // 8,), generator=g, dtype=torch.uint8, device="cuda")
    return d


def _run(d, pro, flip, epi, lo=0, hi=None):
    """The kernel on images [lo, hi) of the inputs d -> dict of everything it writes."""
    G, K, _ = _ops()
    x = d["x"][lo:hi]
    n, H, W, C = x.shape
    px = n * H * W
    p0 = lo * H * W
    w = K.krsc_to_crsk(d["w"]) if flip else d["w"]
    r = {}
    prologue = None
    if pro == "bn_fwd":
        r["side"] = torch.empty_like(x)
        r["side_mask"] = torch.zeros(px * C // 8, dtype=torch.uint8, device="cuda")
        prologue = ("bn_fwd", d["sc"], d["sh"], r["side"], r["side_mask"])
    elif pro == "bn_bwd":
        r["side"] = torch.empty_like(x)
        prologue = ("bn_bwd", d["y"][lo:hi], None, d["coef"], r["side"])
    kw = {"stat": True} if epi == "stat" else {"bn_stat": (d["fy"][lo:hi], d["fm"][p0 * C // 8:(p0 + px) * C // 8])}
    r["out"], r["part"], r["T"] = G.conv3_halo(x, w, prologue=prologue, flip=flip, **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name,stage,pro,flip,epi", CASES, ids=[c[0] for c in CASES])
def test_conv3_persistent_loop(name, stage, pro, flip, epi):
    G, K, _lib = _ops()
    n, H, W, C, k, starts = _geometry(stage, pro)
    d = _inputs(stage, pro, flip, epi)
    prev_s3 = G.set_conv3_s3(True)
    prev = G.set_conv3_sched(True)
    try:
        new = _run(d, pro, flip, epi)
        G.set_conv3_sched(False)
        old = _run(d, pro, flip, epi)
        G.set_conv3_sched(True)
        bm = G.conv3_rows(H, W, C, C, {None: 0, "bn_fwd": 1, "bn_bwd": 2}[pro])
        T = -(-n * H * W // bm)
        assert new["T"] == T and T > 2 * _workgroups()

        # both schedules, bit for bit
        for key in new:
            if key != "T":
                assert torch.equal(new[key], old[key]), "old vs new schedule: " + key

        # side / side_mask against the standalone pass
        a = d["x"]
        if pro == "bn_fwd":
            want = torch.empty_like(a)
            want_mask = torch.zeros(a.numel() // 8, dtype=torch.uint8, device="cuda")
            K.bn_apply(a.view(-1, C), d["sc"], d["sh"], relu=True, out=want.view(-1, C), mask=want_mask)
            torch.cuda.synchronize()
            assert torch.equal(new["side"], want)
            assert torch.equal(new["side_mask"], want_mask)
            a = want
        elif pro == "bn_bwd":
            want = torch.empty_like(a)
            _lib.call("ttdk_bn_bwd_apply", a.data_ptr(), None, None, d["y"].data_ptr(), d["coef"].data_ptr(),
                      want.data_ptr(), a.numel(), C, _lib.stream())
            torch.cuda.synchronize()
            torch.testing.assert_close(new["side"].float(), want.float(), rtol=8e-3, atol=1e-5)
            a = want

        # output and sums against the oracle
        if epi == "stat":
            wf = d["w"].float().permute(0, 3, 1, 2)
            af = a.float().permute(0, 3, 1, 2)
            ref = (F.conv_transpose2d(af, wf, padding=1) if flip else F.conv2d(af, wf, padding=1)).permute(0, 2, 3, 1)
            assert _rel(new["out"], ref) < 1e-2
            o = new["out"].float().reshape(-1, C)
            torch.testing.assert_close(new["part"][:, 0].sum(0), o.sum(0), rtol=1e-3, atol=1e-1)
            torch.testing.assert_close(new["part"][:, 1].sum(0), (o * o).sum(0), rtol=1e-3, atol=1e-1)
        else:
            ref, rpart, _ = G.conv_dgrad(a, K.krsc_to_crsk(d["w"]), (n, H, W, C), (1, 1), (1, 1),
                                         bn_stat=(d["fy"], d["fm"]))
            torch.cuda.synchronize()
            assert _rel(new["out"], ref) < 2e-2
            torch.testing.assert_close(new["part"].sum(0), rpart.sum(0), rtol=2e-2, atol=2.0)

        # schedule independence: a slice of the big run == the slice run alone (one tile per workgroup)
        for lo in starts:
            hi = min(lo + k, n)
            assert (lo * H * W) % bm == 0
            alone = _run(d, pro, flip, epi, lo, hi)
            assert alone["T"] <= _workgroups()
            t0 = lo * H * W // bm
            where = "%s images [%d, %d)" % (name, lo, hi)
            assert torch.equal(new["out"][lo:hi], alone["out"]), where
            assert torch.equal(new["part"][t0:t0 + alone["T"]], alone["part"]), where
            if "side" in new:
                assert torch.equal(new["side"][lo:hi], alone["side"]), where
            if "side_mask" in new:
                q0, q1 = lo * H * W * C // 8, hi * H * W * C // 8
                assert torch.equal(new["side_mask"][q0:q1], alone["side_mask"]), where
    finally:
        G.set_conv3_sched(prev)
        G.set_conv3_s3(prev_s3)
