"""Launch plans of the GEMM / convolution kernels (csrc/kernels/gemm_plan.h through libttd_rt.so),
checked on the CPU: the launchers and ops.gemm share these functions, so what is pinned here is
what runs.

tests/golden/launch_plan_parent.json holds what the Python copies of these rules answered, under
the default environment, at the commit before they were replaced by the shared header: every
conv of ResNet-50 v1.5 at 224 x 224 (per-GPU batch 32, 256, 1024), the smoke network (64 x 64,
batch 16) and the BERT-Large GEMMs (128 x 512 and 32 x 512 tokens)."""
import ctypes
import json
import os

import pytest

from tensorflow_train_distributed_amd.ops import _lib, _plan
from tensorflow_train_distributed_amd.ops import gemm as G

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "launch_plan_parent.json")
SPLITS = (1, 2, 7, 64, 10 ** 6)
STAGES_50 = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))
STAGES_SMOKE = ((64, 1, 1), (128, 1, 2), (256, 1, 2), (512, 1, 2))


def resnet_convs(batch, size, stages):
    """(N, H, W, C, K, R, stride, pad) of every conv of the bottleneck ResNet (stride on the 3x3,
    stem input stored with 8 channels), in network order."""
    out = [(batch, size, size, 8, 64, 7, 2, 3)]
    h = size // 4  # stem /2, max pool /2
    cin = 64
    for mid, n, stride in stages:
        for b in range(n):
            s = stride if b == 0 else 1
            out.append((batch, h, h, cin, mid, 1, 1, 0))
            out.append((batch, h, h, mid, mid, 3, s, 1))
            if s != 1 or cin != mid * 4:
                out.append((batch, h, h, cin, mid * 4, 1, s, 0))
            h //= s
            out.append((batch, h, h, mid, mid * 4, 1, 1, 0))
            cin = mid * 4
    return out


def workload_convs():
    seen, out = set(), []
    for cfg in ([c for b in (32, 256, 1024) for c in resnet_convs(b, 224, STAGES_50)]
                + resnet_convs(16, 64, STAGES_SMOKE)):
        if cfg not in seen:
            seen.add(cfg)
            out.append(cfg)
    return out


def workload_gemms():
    """(M, N, K) of the BERT-Large dense layers: forward / data gradients (tokens x features) and
    weight gradients (features x features over tokens)."""
    out = []
    for T in (128 * 512, 32 * 512):
        for a, b in ((1024, 1024), (3072, 1024), (4096, 1024), (1024, 4096), (1024, 3072)):
            out += [(T, a, b), (a, b, T)]
    return out


def conv_row(cfg, tile, phases):
    """Everything the plan answers for one conv. tile(M, N) -> (bm, bn); phases(g) -> the
    non-empty phase pairs as [[r0, T, n] rows, [r0, T, n] columns], in launch order."""
    N, H, W, C, K, R, s, p = cfg
    x, w, wt = (N, H, W, C), (K, R, R, C), (C, R, R, K)
    st, pd = (s, s), (p, p)
    g = G.conv_geom(x, w, st, pd)
    fwd = (N * g.P * g.Q, K, R * R * C)
    dgr = (N * H * W, C, R * R * K)
    wgr = (K, R * R * C, N * g.P * g.Q)
    row = {
        "big_bn": [G.big_bn(*fwd), G.big_bn(*dgr), G.big_bn(*wgr)],
        "big_bn_wgrad": G.big_bn_wgrad(*wgr),
        "tile": [list(tile(*fwd[:2])), list(tile(*dgr[:2])), list(tile(*wgr[:2]))],
        "wgrad_splits": G.wgrad_splits(g),
        "gemm_wgrad_splits": G.gemm_wgrad_splits(*wgr),
        "wgrad4t_splits": G.conv_wgrad4t_splits(g),
        "wgrad4t_rows": G.wgrad4t_rows(K),
        "stat_tile": G.dgrad_stat_tile(x, wt, st, pd),
        "stat_tile_nopad": G.dgrad_stat_tile(x, wt),  # as conv_dgrad calls it
        "stat_rows": G.dgrad_stat_rows(x, wt, st, pd),
        "ok": [int(v) for v in (
            G.conv_fwd4w_ok(x, w, st, pd), G.conv_fwd4w_pays(x, w, st, pd), G.conv_dgrad4w_pays(x, wt, st, pd),
            G.conv_fwd_bnpro_ok(x, w), G.conv_wgrad_fp8_ok(x, w, st, pd), G.conv_wgrad_bn_fusable(x, w, st, pd),
            G.conv_fwd4k8_ok(x, w, st, pd), G.conv_fwd4k8_pays(x, w, st, pd), G.conv_dgrad_fp8_ok(x, wt, st, pd),
            G.dgrad_bnpro_ok(x, wt, st, pd))],
    }
    row["stat_tile"] = row["stat_tile"] and list(row["stat_tile"])
    row["stat_tile_nopad"] = list(row["stat_tile_nopad"])
    if G._subpixel_ok(g, R, R, st, pd):
        row["phases"] = phases(g)
    return row


def gemm_row(M, N, K, tile):
    return {"big_bn": G.big_bn(M, N, K), "big_fits": int(G.big_fits(M, N, K)), "big_bn_wgrad": G.big_bn_wgrad(M, N, K),
            "tile": list(tile(M, N)), "gemm_wgrad_splits": G.gemm_wgrad_splits(M, N, K)}


def table(tile, phases):
    convs, gemms = workload_convs(), workload_gemms()
    ks = set(k for _, _, k in gemms)
    for N, H, W, C, K, R, s, p in convs:
        P = (H + 2 * p - R) // s + 1
        ks.update((R * R * C, R * R * K, N * P * P))
    return {
        "convs": [[list(c), conv_row(c, tile, phases)] for c in convs],
        "gemms": [[list(m), gemm_row(*m, tile)] for m in gemms],
        "splits": [[k, [[G.effective_splits(k, s, bk) for s in SPLITS] for bk in (64, 128)]] for k in sorted(ks)],
    }


def _phases(g):
    return [[[r.r0, r.T, r.n], [c.r0, c.T, c.n]] for r, c in _plan.subpixel_phases(g)]


def test_workload_plans_match_parent_table():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(table(_plan.pick_tile, _phases)))
    for key in ("convs", "gemms", "splits"):
        assert len(got[key]) == len(want[key])
        for g_, w_ in zip(got[key], want[key]):
            assert g_ == w_, (key, g_[0])


def _phase_rows(cfg):
    N, H, W, C, K, R, s, p = cfg
    g = G.conv_geom((N, H, W, C), (K, R, R, C), (s, s), (p, p))
    rows = 0
    for r, c in _plan.subpixel_phases(g):
        M, Kg = N * r.n * c.n, r.T * c.T * K
        bm = 256 if (G.big_bn(M, C, Kg) and K % 64 == 0) else _plan.pick_tile(M, C)[0]
        rows += -(-M // bm)
    return rows


@pytest.mark.parametrize("cfg", [
    # the four configurations of test_conv_dgrad_subpixel_phases, and stride 2 on an extent of 1
    (2, 15, 13, 32, 64, 3, 2, 1),
    (2, 12, 12, 16, 64, 3, 3, 1),
    (2, 9, 9, 16, 64, 5, 2, 2),
    (8, 56, 56, 128, 128, 3, 2, 1),
    (2, 1, 7, 16, 64, 3, 2, 1),
])
def test_subpixel_phases_partition(cfg):
    N, H, W, C, K, R, s, p = cfg
    g = G.conv_geom((N, H, W, C), (K, R, R, C), (s, s), (p, p))
    pairs = _plan.subpixel_phases(g)
    assert len(pairs) == min(s, H) * min(s, W)
    for axis, extent in ((0, H), (1, W)):
        phases = _axis(pairs, axis, s, extent)
        covered = sorted(s * i + a for a, ph in enumerate(phases) for i in range(ph.n))
        assert covered == list(range(extent))  # the phases partition [0, extent)
        if extent >= s:
            assert sum(ph.T for ph in phases) == R  # every tap belongs to exactly one phase
        for a, ph in enumerate(phases):
            assert ph.r0 + (ph.T - 1) * s < R and ph.off * s + ph.r0 == a + p
    assert G.dgrad_stat_rows((N, H, W, C), (C, R, R, K), (s, s), (p, p)) == _phase_rows(cfg)
    assert _plan.subpixel_stat_rows(g) == _phase_rows(cfg)


def _axis(pairs, axis, s, extent):
    """The phases along one axis in phase order a = 0 .. min(s, extent) - 1."""
    seen = []
    for pr in pairs:
        if pr[axis] not in seen:
            seen.append(pr[axis])
    assert len(seen) == min(s, extent)
    return seen


def _geom(x, w, s=1, p=0):
    return G.conv_geom(x, w, (s, s), (p, p))


def test_drift_cases():
    """One case per rule on which the Python copies had drifted from the launchers; the expected
    value is the launcher's condition."""
    # ttdk_conv_fwd4w: (K + 256) * R*S*C * 2 < 2^32 — 3x3, C = 8192, K = 28928: 29184 * 73728 * 2 = 2^32 + 8.4e6
    x, w = (1, 8, 8, 8192), (28928, 3, 3, 8192)
    assert (28928 + 256) * 9 * 8192 * 2 >= 1 << 32
    assert not G.conv_fwd4w_ok(x, w, (1, 1), (1, 1))
    assert G.conv_fwd4w_ok(x, (28672, 3, 3, 8192), (1, 1), (1, 1))  # 28928 * 73728 * 2 < 2^32
    # ... and M * K * 2 < 2^40: 2^22 pixels x 2^17 channels
    assert not G.conv_fwd4w_ok((64, 256, 256, 128), (1 << 17, 1, 1, 128))
    assert G.conv_fwd4w_ok((64, 256, 256, 128), (1 << 16, 1, 1, 128))
    # ttdk_conv_dgrad4w: (C + 256) * R*S*K * 2 < 2^32, R * S <= 32
    big_c = (1, 8, 8, 28928)
    assert not _plan.takes("conv_dgrad4w", _geom(big_c, (8192, 3, 3, 28928), 1, 1))
    assert _plan.takes("conv_dgrad4w", _geom((1, 8, 8, 28672), (8192, 3, 3, 28672), 1, 1))
    assert not _plan.takes("conv_dgrad4w", _geom((2, 16, 16, 256), (256, 7, 7, 256), 1, 3))  # 49 taps
    assert not G.conv_dgrad4w_pays((2, 16, 16, 256), (256, 7, 7, 256), (1, 1), (3, 3))
    assert G.conv_dgrad4w_pays((2, 16, 16, 256), (256, 5, 5, 256), (1, 1), (2, 2))
    # ttdk_conv_fwd4k8: M * C < 2^32 is asked of pointwise convs only (where xb = M * C < 2^31
    # already implies it). A non-pointwise conv with M * C >= 2^32 and xb = N*H*W*C < 2^31 has more
    # than twice as many output as input pixels, which takes padding beyond the filter's reach:
    # 1x1 with padding 1 on 2 x 2 inputs (4 x 4 outputs).
    n = 1 << 19
    g = _geom((n, 2, 2, 512), (256, 1, 1, 512), 1, 1)
    assert g.P == 4 and n * 16 * 512 >= 1 << 32 and n * 4 * 512 + 3 * 512 < 1 << 31
    assert _plan.takes("conv_fwd4k8", g) and G.conv_fwd4k8_ok((n, 2, 2, 512), (256, 1, 1, 512), (1, 1), (1, 1))
    assert not G.conv_fwd4k8_ok((1 << 16, 16, 16, 256), (256, 1, 1, 256))  # pointwise, M * C = 2^32
    assert G.conv_fwd4k8_ok((1 << 14, 16, 16, 256), (256, 1, 1, 256))
    # ttdk_conv_dgrad4k8: a 3x3 data gradient with padding 3 (pho = R - 1 - ph < 0) is refused by
    # the 4-wave launcher, so conv_dgrad_fp8 takes the 8-wave kernel; with padding 1 the 4-wave one
    x, wt = (8, 16, 16, 256), (256, 3, 3, 256)
    assert not _plan.takes("conv_dgrad4k8", _geom(x, (256, 3, 3, 256), 1, 3))
    assert G.conv_dgrad_fp8_path(x, wt, (1, 1), (3, 3), beta=0, stat=True, beta_s2=False) == "8-wave"
    assert G.conv_dgrad_fp8_path(x, wt, (1, 1), (1, 1), beta=0, stat=True, beta_s2=False) == "4-wave"
    assert G.conv_dgrad_fp8_path(x, wt, (1, 1), (1, 1), beta=1, stat=True, beta_s2=False) == "8-wave"  # policy
    assert G.conv_dgrad_fp8_path(x, (64, 3, 3, 256), (1, 1), (1, 1), beta=0, stat=False, beta_s2=False) == "8-wave"
    # g4t_bm / wgrad4t_rows: the switch is an argument, read once by each caller
    assert [_plan.g4t_bm(m, False, True) for m in (64, 128, 129)] == [128, 128, 256]
    assert _plan.g4t_bm(128, True, True) == 256 and _plan.g4t_bm(128, False, False) == 256
    assert G.wgrad4t_rows(128) == _plan.g4t_bm(128, False, G._G4T_BM128)


def test_split_clamps():
    for kt in (1, 2, 3, 7, 64, 1000):
        for s in (-3, 0, 1, 2, 7, 64, 10 ** 6):
            got = _plan.clamp_splits(kt, s)
            per = -(-kt // got)
            assert 1 <= got <= max(1, min(s, kt)) and per * (got - 1) < kt <= per * got  # no empty split
            got4 = _plan.clamp_splits_4t(kt, s)
            per4 = -(-kt // got4)
            assert 1 <= got4 <= max(1, min(s, kt // 2)) and per4 * (got4 - 1) < kt <= per4 * got4
            assert got4 == 1 or kt - per4 * (got4 - 1) >= 1 and per4 >= 2


def test_conv_geom_struct_size():
    assert ctypes.sizeof(_lib.ConvGeom) == _plan._fn("conv_size")() == 15 * 4
