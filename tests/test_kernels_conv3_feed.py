"""The prefetched feeding-BN epilogue of the halo 3x3 data gradients (csrc/kernels/conv3_halo.hip,
template parameter FEED; stream_epi.h: feed_batch_load / feed_batch_rows) against the generic row
loop it replaces (epi_rows), through ops.gemm.set_conv3_feed, bit for bit: output, per-tile
statistics rows, side and side_mask.

Cases (prologue, flip, epilogue): c3 dgrad + bn_stat, c3 bn_bwd dgrad + bn_stat, c3s dgrad +
bn_stat, c3 bn_fwd + stat, c3s bn_fwd + stat. Only the data gradients have a second form: the two
forward cases run the same kernel under both settings (the switch must leave them alone).

Shapes:
* smallest, at most one tile per workgroup: 1 image of 56x56x64 (7 tiles of 8 rows, 14 of 4 rows
  with the BN-backward prologue, whose 4-row tiles give a thread 4 epilogue rows, the last one
  guarded) and 3 images of 28x28x128 (84 flattened rows: a tile straddles two images and the
  last tile has 4 rows, so the row guard of the epilogue and its zero-page loads are exercised);
* persistent, sized from the CU count as tests/test_kernels_conv3_pipeline.py does: some
  workgroups walk three or more tiles. The first batch of the epilogue's loads is issued under the
  tap loop, in stage 3 counted into the waits that retire the streamed filter and the next tile's
  halo; that interplay across tiles exists only here.

The data gradients are also compared with conv_dgrad(bn_stat=...) at the tolerances of
tests/test_kernels_conv3.py (output 2e-2 relative to the maximum, sums rtol 2e-2), and one small
data gradient per kernel runs with the ReLU bits absent.
"""
import pytest
import torch

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
    ("c3_dgrad_bnstat", 2, None, True, "bn_stat"),
    ("c3_bnbwd_dgrad_bnstat", 2, "bn_bwd", True, "bn_stat"),
    ("c3s_dgrad_bnstat", 3, None, True, "bn_stat"),
    ("c3_bnfwd_stat", 2, "bn_fwd", False, "stat"),
    ("c3s_bnfwd_stat", 3, "bn_fwd", False, "stat"),
]


def _images(stage, size):
    """Number of images: `small` = at most one tile per workgroup; `persistent` = more than two
    tiles per workgroup for some workgroups and fewer for the rest."""
    if size == "small":
        return 1 if stage == 2 else 3
    wg = _workgroups()
    if stage == 2:
        n = 2 * wg // 7 + 2                     # 7 n tiles of 8 rows in (2 wg, 3 wg)
        assert 2 * wg < 7 * n < 3 * wg
        return n
    n = (4 * wg // 7 + 1) | 1                   # odd: 28 n rows end in a 4-row tile
    assert -(-28 * n // 8) > 2 * wg and (28 * n) % 8 == 4
    return n


def _inputs(stage, pro, flip, epi, size, mask=True):
    n = _images(stage, size)
    H, W, C = (56, 56, 64) if stage == 2 else (28, 28, 128)
    s = 1000 + 100 * stage + 10 * (pro is not None) + flip
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
        d["fm"] = (torch.randint(0, 256, (n * H * W * C // 8,), generator=g, dtype=torch.uint8, device="cuda")
                   if mask else None)
    return d


def _run(d, pro, flip, epi):
    """The kernel on the inputs d -> dict of everything it writes."""
    G, K, _ = _ops()
    x = d["x"]
    n, H, W, C = x.shape
    w = K.krsc_to_crsk(d["w"]) if flip else d["w"]
    r = {}
    prologue = None
    if pro == "bn_fwd":
        r["side"] = torch.empty_like(x)
        r["side_mask"] = torch.zeros(n * H * W * C // 8, dtype=torch.uint8, device="cuda")
        prologue = ("bn_fwd", d["sc"], d["sh"], r["side"], r["side_mask"])
    elif pro == "bn_bwd":
        r["side"] = torch.empty_like(x)
        prologue = ("bn_bwd", d["y"], None, d["coef"], r["side"])
    kw = {"stat": True} if epi == "stat" else {"bn_stat": (d["fy"], d["fm"])}
    r["out"], r["part"], r["T"] = G.conv3_halo(x, w, prologue=prologue, flip=flip, **kw)
    torch.cuda.synchronize()
    return r


def _old_new(d, pro, flip, epi):
    G, _, _ = _ops()
    prev_s3 = G.set_conv3_s3(True)
    prev_sched = G.set_conv3_sched(True)
    prev = G.set_conv3_feed(True)
    try:
        new = _run(d, pro, flip, epi)
        assert G.set_conv3_feed(False) is True
        old = _run(d, pro, flip, epi)
    finally:
        G.set_conv3_feed(prev)
        G.set_conv3_sched(prev_sched)
        G.set_conv3_s3(prev_s3)
    for key in new:
        if key != "T":
            assert torch.equal(new[key], old[key]), "prefetched vs generic epilogue: " + key
    assert new["T"] == old["T"]
    return new


def _check_dgrad_oracle(d, pro, new):
    """Output and sums of a feeding data gradient against conv_dgrad(bn_stat=...)."""
    G, K, _lib = _ops()
    a = d["x"]
    n, H, W, C = a.shape
    if pro == "bn_bwd":
        want = torch.empty_like(a)
        _lib.call("ttdk_bn_bwd_apply", a.data_ptr(), None, None, d["y"].data_ptr(), d["coef"].data_ptr(),
                  want.data_ptr(), a.numel(), C, _lib.stream())
        torch.cuda.synchronize()
        torch.testing.assert_close(new["side"].float(), want.float(), rtol=8e-3, atol=1e-5)
        a = want
    ref, rpart, _ = G.conv_dgrad(a, K.krsc_to_crsk(d["w"]), (n, H, W, C), (1, 1), (1, 1), bn_stat=(d["fy"], d["fm"]))
    torch.cuda.synchronize()
    assert _rel(new["out"], ref) < 2e-2
    torch.testing.assert_close(new["part"].sum(0), rpart.sum(0), rtol=2e-2, atol=2.0)


@pytest.mark.parametrize("size", ["small", "persistent"])
@pytest.mark.parametrize("name,stage,pro,flip,epi", CASES, ids=[c[0] for c in CASES])
def test_conv3_feed_old_vs_new(name, stage, pro, flip, epi, size):
    G, _, _ = _ops()
    d = _inputs(stage, pro, flip, epi, size)
    new = _old_new(d, pro, flip, epi)
    n, H, W, C = d["x"].shape
    bm = G.conv3_rows(H, W, C, C, {None: 0, "bn_fwd": 1, "bn_bwd": 2}[pro])
    T = -(-n * H * W // bm)
    assert new["T"] == T
    if size == "small":
        assert T <= _workgroups()
    else:
        assert T > 2 * _workgroups()
    if epi == "bn_stat":
        _check_dgrad_oracle(d, pro, new)


@pytest.mark.parametrize("stage", [2, 3], ids=["c3", "c3s"])
def test_conv3_feed_without_relu_bits(stage):
    """bn_stat=(y, None): every element kept; the absent bits read the zero page and are ignored."""
    d = _inputs(stage, None, True, "bn_stat", "small", mask=False)
    new = _old_new(d, None, True, "bn_stat")
    _check_dgrad_oracle(d, None, new)
