"""Group normalisation without a GPU: `ttd.nn.group_norm` and `layers.GroupNormalization` on CPU
tensors against the float64 oracle (groupnorm_oracle.py), the layer's variables and flags, the
refusals, and the launch plan (csrc/kernels/groupnorm_plan.h) pinned through ops/_plan.py."""
import pytest
import torch

import groupnorm_oracle as O
from tensorflow_train_distributed_amd import layers as L
from tensorflow_train_distributed_amd import nn as N
from tensorflow_train_distributed_amd.ops import _plan
from tensorflow_train_distributed_amd.utils.errors import InvalidArgumentError

F64 = O.F64


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------ ttd.nn on CPU tensors
@pytest.mark.parametrize("affine", ["both", "gamma", "beta", "none"])
@pytest.mark.parametrize("shape,G", [((5, 12), 3), ((3, 7, 12), 1), ((2, 3, 5, 12), 12), ((2, 2, 3, 2, 12), 4)],
                         ids=lambda v: str(v))
def test_nn_group_norm_cpu_matches_oracle(shape, G, affine):
    gen = torch.Generator().manual_seed(21 + len(shape))
    C = shape[-1]
    x0 = torch.randn(shape, generator=gen) * 2 + 1
    dy = torch.randn(shape, generator=gen)
    g0 = torch.rand(C, generator=gen) + 0.5 if affine in ("both", "gamma") else None
    b0 = torch.randn(C, generator=gen) if affine in ("both", "beta") else None
    x = x0.clone().requires_grad_(True)
    gm = g0.clone().requires_grad_(True) if g0 is not None else None
    bt = b0.clone().requires_grad_(True) if b0 is not None else None
    y = N.group_norm(x, gm, bt, groups=G, eps=1e-3)
    assert y.dtype == torch.float32 and y.shape == x.shape
    y.backward(dy)
    x3, dy3 = x0.reshape(shape[0], -1, C), dy.reshape(shape[0], -1, C)
    mean, _, rstd = O.stats_def(x3, G, 1e-3)
    want_dx, want_dg, want_db = O.backward_def(dy3, x3, mean, rstd, g0)
    assert _rel(y.detach().reshape(x3.shape), O.apply(x3, mean, rstd, g0, b0)) <= 1e-5
    assert _rel(x.grad.reshape(x3.shape), want_dx) <= 1e-4
    if gm is not None:
        assert _rel(gm.grad, want_dg) <= 1e-5
    if bt is not None:
        assert _rel(bt.grad, want_db) <= 1e-5


def test_nn_group_norm_cpu_returns_the_inputs_dtype_and_defaults():
    x = torch.randn(2, 4, 4, 64).bfloat16()
    y = N.group_norm(x, torch.ones(64), torch.zeros(64))  # groups = 32, eps = 1e-3
    assert y.dtype == torch.bfloat16
    mean, _, rstd = O.stats_def(x.reshape(2, 16, 64), 32, 1e-3)
    want = O.apply(x.reshape(2, 16, 64), mean, rstd, None, None)
    assert float((y.double().reshape(2, 16, 64) - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


def test_nn_group_norm_refusals_on_cpu():
    x = torch.randn(2, 4, 4, 8)
    g8 = torch.ones(8)
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x[0, 0, 0], g8, None, groups=2)  # rank 1
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, g8, None, groups=3)  # G does not divide C
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, g8, None, groups=0)
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, g8, None, groups=-1)  # -1 is the layer's convention, not the function's
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, torch.ones(4), None, groups=2)
    with pytest.raises(InvalidArgumentError):
        N.group_norm(x, None, torch.ones(2, 8), groups=2)


# ------------------------------------------------------------------ the layer
def test_group_normalization_layer_variables_flags_and_values():
    L.reset_naming(0)
    x = torch.randn(2, 5, 5, 12) * 3 + 1
    full, inst = L.GroupNormalization(groups=4), L.GroupNormalization(groups=-1)
    no_beta, no_gamma = L.GroupNormalization(groups=3, center=False), L.GroupNormalization(groups=3, scale=False)
    bare = L.GroupNormalization(groups=2, center=False, scale=False, name="gn_bare")
    with torch.no_grad():
        ys = [m(x) for m in (full, inst, no_beta, no_gamma, bare)]
    assert full.epsilon == 1e-3 and L.GroupNormalization().groups == 32
    assert [(n, tuple(t.shape)) for n, t in full.named_variables()] == [("group_normalization/gamma", (12,)),
                                                                       ("group_normalization/beta", (12,))]
    assert torch.equal(full.gamma.detach(), torch.ones(12)) and torch.equal(full.beta.detach(), torch.zeros(12))
    assert [n for n, _ in inst.named_variables()] == ["group_normalization_1/gamma", "group_normalization_1/beta"]
    assert [n for n, _ in no_beta.named_variables()] == ["group_normalization_2/gamma"]
    assert [n for n, _ in no_gamma.named_variables()] == ["group_normalization_3/beta"]
    assert bare.named_variables() == [] and bare.layer_name == "gn_bare"
    x3 = x.reshape(2, 25, 12)
    for y, G in zip(ys, (4, 12, 3, 3, 2)):
        mean, _, rstd = O.stats_def(x3, G, 1e-3)
        assert _rel(y.reshape(x3.shape), O.apply(x3, mean, rstd, None, None)) <= 1e-5
    # no moving statistics and no dependence on `training`
    with torch.no_grad():
        assert torch.equal(full(x, training=False), full(x, training=True))
    assert all(t.requires_grad for t in full.variables)


def test_group_normalization_layer_gradients_and_refusals():
    L.reset_naming(0)
    x = (torch.randn(3, 4, 6) * 2).requires_grad_(True)
    layer = L.GroupNormalization(groups=2)
    dy = torch.randn(3, 4, 6)
    layer(x).backward(dy)
    x3 = x.detach()
    mean, _, rstd = O.stats_def(x3, 2, 1e-3)
    dx, dg, db = O.backward_def(dy, x3, mean, rstd, None)
    assert _rel(x.grad, dx) <= 1e-4 and _rel(layer.gamma.grad, dg) <= 1e-5 and _rel(layer.beta.grad, db) <= 1e-5
    with pytest.raises(InvalidArgumentError):
        L.GroupNormalization(groups=5)(torch.randn(2, 3, 12))
    with pytest.raises(InvalidArgumentError):
        L.GroupNormalization(groups=0)
    with pytest.raises(InvalidArgumentError):
        L.GroupNormalization(groups=-2)


# ------------------------------------------------------------------ the plan
def test_plan_admission_truth_table():
    for C, G in O.FAST_CG:
        assert _plan.gn_fast_takes(3, 7, C, G, True) and not _plan.gn_fast_takes(3, 7, C, G, False)
    assert _plan.gn_fast_takes(32, 4096, 320, 32, True)  # Cg = 10, the diffusion UNet case
    assert _plan.gn_fast_takes(32, 3136, 64, 32, True)   # Cg = 2, ResNet-GN at 64 channels
    for C, G in O.GENERIC_CG + [(12, 3), (4, 4), (2052, 1)]:
        assert _plan.gn_valid(3, 7, C, G)
        assert not _plan.gn_fast_takes(3, 7, C, G, True) and not _plan.gn_fast_takes(3, 7, C, G, False)
    for bad in ((0, 7, 8, 2), (3, 0, 8, 2), (3, 7, 0, 1), (3, 7, 8, 0), (3, 7, 8, 3), (3, 7, 8, -1), (-1, 7, 8, 2)):
        assert not _plan.gn_valid(*bad) and not _plan.gn_fast_takes(*bad, True)


def test_plan_lanes_and_rows_per_block():
    for C, lanes, rows in ((8, 1, 256), (16, 2, 128), (64, 8, 32), (256, 32, 8), (264, 17, 15), (320, 20, 12),
                           (2048, 32, 8), (2056, 29, 8)):
        assert (_plan.gn_lanes(C, True), _plan.gn_rows_per_block(C, True)) == (lanes, rows), C
        assert lanes * rows <= 256 and lanes * -(-(C // 8) // lanes) >= C // 8
    for C in (1, 3, 64, 65, 2056):
        assert (_plan.gn_lanes(C, False), _plan.gn_rows_per_block(C, False)) == (64, 4)
    assert [_plan.gn_part_stride(C) for C in (1, 3, 4, 5, 8, 65)] == [4, 4, 4, 8, 8, 68]


def _partition(N_, M, C):
    T = _plan.gn_parts(N_, M, C)
    rows = [_plan.gn_slab_rows(N_, M, C, t) for t in range(T)]
    return T, rows


@pytest.mark.parametrize("N_,C", [(1, 8), (3, 16), (32, 64), (7, 2056), (600, 8), (1, 1 << 14), (4, 1 << 20)])
def test_plan_slabs_cover_every_row_exactly_once(N_, C):
    cap = O.CAP // N_
    ps = _plan.gn_part_stride(C)
    by_bytes = _plan.gn_max_ws_floats() // (N_ * 2 * ps)
    cap = max(1, min(cap, by_bytes))
    Ms = {1, 2, 3}
    for k in (1, 2, 3):  # around every boundary where the rows per slab step up
        Ms |= {k * cap - 1, k * cap, k * cap + 1}
    for M in sorted(m for m in Ms if m >= 1):
        T, rows = _partition(N_, M, C)
        per = _plan.gn_rows_per_slab(N_, M, C)
        assert per == -(-M // cap) and T == -(-M // per) and 1 <= T <= cap, (M, T, per)
        assert rows[0][0] == 0 and rows[-1][1] == M
        for t, (r0, r1) in enumerate(rows):
            assert r0 < r1 and r1 - r0 <= per, (M, t, r0, r1)  # never an empty slab
            assert t == 0 or rows[t - 1][1] == r0
        assert _plan.gn_slab_rows(N_, M, C, T) == (M, M)
        assert _plan.gn_fwd_ws_floats(N_, M, C) == (T + 2) * N_ * 2 * ps
        assert _plan.gn_bwd_ws_floats(N_, M, C) == (T + 4) * N_ * 2 * ps


def test_plan_caps():
    """At most 512 partial rows and 16 MiB of them, unless N * C alone exceeds that: then one slab
    per image and a workspace of what N rows need."""
    assert O.CAP == 512 and _plan.gn_max_ws_floats() == 1 << 22
    for N_, M, C in ((1, 10 ** 6, 8), (3, 10 ** 6, 16), (32, 3136, 64), (32, 49, 2048), (512, 100, 8), (5, 9999, 2056)):
        T = _plan.gn_parts(N_, M, C)
        assert N_ * T <= 512 and N_ * T * 2 * _plan.gn_part_stride(C) <= 1 << 22, (N_, M, C, T)
    assert _plan.gn_parts(32, 3136, 64) == 16 and _plan.gn_parts(32, 49, 2048) == 13
    # the byte cap binds before the row cap: 4 * 2 * 2^16 floats per slab of the batch
    assert _plan.gn_parts(4, 1000, 1 << 16) == 8
    for N_, M, C in ((513, 100, 8), (4096, 7, 16), (2, 100, 1 << 21), (64, 9, 1 << 16)):
        assert _plan.gn_parts(N_, M, C) == 1 and _plan.gn_slab_rows(N_, M, C, 0) == (0, M)
        assert _plan.gn_fwd_ws_floats(N_, M, C) == 3 * N_ * 2 * _plan.gn_part_stride(C)
        assert _plan.gn_bwd_ws_floats(N_, M, C) == 5 * N_ * 2 * _plan.gn_part_stride(C)
