"""The statements of tests/elementwise_oracle.py, checked on the CPU against independent ones:
Philox4x32-10 against the published known-answer vectors and a scalar restatement on Python
integers, the activations and their derivatives against torch under float64 autograd (limits
included), the fp8 encode of every bf16 pattern against a brute-force search of the decode table,
the decode table against torch, the layouts against permute and slicing, the float32 column sum
against the float64 one; then the oracle run in float32 against itself in float64 on the case tables
of tests/test_elementwise_kernels.py: those maxima, times O.MARGIN, are the bars of the GPU tests
(run with -s to see them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


# ------------------------------------------------------------------ Philox
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _philox_ints(c, k):
    """The same generator on Python integers, one counter at a time."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w[0]) for w in O.philox4x32_10(counter, key)) == want
    assert _philox_ints(counter, key) == want


def test_philox_vectorised_equals_scalar():
    ctr = np.array([0, 1, 2, 0xffffffff, 12345], dtype=np.uint64)
    got = O.philox4x32_10((ctr, ctr[::-1].copy(), 5, 0xdeadbeef), (7, 0x80000000))
    for i in range(len(ctr)):
        want = _philox_ints((int(ctr[i]), int(ctr[::-1][i]), 5, 0xdeadbeef), (7, 0x80000000))
        assert tuple(int(w[i]) for w in got) == want


@pytest.mark.parametrize("seed,offset", O.SEEDS)
def test_keep_mask_by_hand(seed, offset):
    """Element idx: word idx & 3 of counter (idx >> 2, offset) under key seed, each split into its
    low and high 32 bits; kept when float32(r >> 8) * 2^-24 >= float32(rate)."""
    n, rate = 23, 0.25
    got = O.keep_mask(n, rate, seed, offset)
    for idx in range(n):
        r = _philox_ints(((idx >> 2) & 0xffffffff, (idx >> 2) >> 32, offset & 0xffffffff, offset >> 32),
                         (seed & 0xffffffff, seed >> 32))[idx & 3]
        assert bool(got[idx]) == bool(np.float32(r >> 8) * np.float32(2.0 ** -24) >= np.float32(rate)), idx
    assert O.keep_mask(0, rate, seed, offset).shape == (0,)
    assert not O.keep_mask(4099, 1.0, seed, offset).any() and O.keep_mask(4099, 0.0, seed, offset).all()
    big = O.keep_mask(1 << 18, rate, seed, offset)
    assert abs(big.mean() - 0.75) < 0.005
    # other (seed, offset) pairs, and the two swapped, give another mask
    assert (big != O.keep_mask(1 << 18, rate, seed + 1, offset)).mean() > 0.3
    assert (big != O.keep_mask(1 << 18, rate, offset + 1, seed)).mean() > 0.3


def test_drop_scale_is_float32():
    assert O.drop_scale(0.0) == 1.0 and O.drop_scale(1.0) == float("inf")
    assert O.drop_scale(0.01) == float(np.float32(1) / (np.float32(1) - np.float32(0.01)))
    assert O.drop_scale(0.01) != 1 / 0.99


# ------------------------------------------------------------------ activations
_TORCH_ACT = {O.ACT_NONE: lambda t: t, O.ACT_RELU: F.relu, O.ACT_GELU: lambda t: F.gelu(t, approximate="tanh"),
              O.ACT_ELU: F.elu}
_LIMITS = (0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 1e4, -1e4, 1e20, -1e20)


@pytest.mark.parametrize("kind", O.ACTS)
def test_activations_match_torch_double_autograd(kind):
    z = torch.cat([torch.randn(4096, generator=O._gen(1), dtype=F64) * 3, torch.tensor(_LIMITS + O.PLANTED, dtype=F64)])
    za = z.clone().requires_grad_(True)
    y = _TORCH_ACT[kind](za)
    (g,) = torch.autograd.grad(y.sum(), za) if kind != O.ACT_NONE else (torch.ones_like(z),)
    # 1e-12 of the value, and for GELU's 1 + tanh and 1 - tanh^2 near saturation two roundings of a
    # term of size 1 times what multiplies it: 0.5 |z|, and 0.5 |z| k0 (1 + 3 k1 z^2) in the derivative
    # (far less than 1e-12 of anything at the planted 1e-30; the far limits are in test_activation_limits)
    slack = 2.0 ** -51 * z.abs() * (1 + 3 * O.K1 * z * z)
    for got, want in ((O.act(z, kind), y.detach()), (O.dact(z, kind), g)):
        assert not bool(torch.isnan(got).any())
        assert bool(((got - want).abs() <= 1e-12 * want.abs() + slack).all()), kind


def test_activation_limits():
    lim = torch.tensor(_LIMITS, dtype=F64)
    for dtype in (F64, F32):
        d = {k: O.dact(lim.to(F32), k, dtype).tolist() for k in O.ACTS}
        assert d[O.ACT_RELU][:2] == [0, 0] and d[O.ACT_ELU][:2] == [1, 1] and d[O.ACT_GELU][:2] == [0.5, 0.5]
        assert d[O.ACT_GELU][-2:] == [1, 0] and d[O.ACT_GELU][-4:-2] == [1, 0]      # no 0 * inf
        assert d[O.ACT_RELU][-2:] == [1, 0] and d[O.ACT_ELU][-2:] == [1, 0]
        y = {k: O.act(lim.to(F32), k, dtype) for k in O.ACTS}
        assert not any(bool(torch.isnan(v).any()) for v in y.values())
        assert y[O.ACT_GELU][-2:].tolist() == [float(lim[-2].to(F32)), 0] and y[O.ACT_ELU][-1].item() == -1


def test_bias_act_dropout_statement_by_hand():
    """n = 5, C = 2, ReLU, rate 0.5: z = x + bias[idx % 2] in float32; kept elements are doubled."""
    x = torch.tensor([1.0, -1.0, 0.25, 3.0, -0.5])
    bias = torch.tensor([0.5, 2.0])
    keep = torch.tensor([True, False, True, True, False])
    y, z = O.bias_act_dropout_fwd(x, bias, 2, O.ACT_RELU, 0.5, keep)
    assert z.tolist() == [1.5, 1.0, 0.75, 5.0, 0.0] and z.dtype == F32
    assert y.tolist() == [3.0, 0.0, 1.5, 10.0, 0.0]
    dy = torch.tensor([1.0, 1.0, -2.0, 4.0, 8.0])
    dx, _ = O.bias_act_dropout_bwd(dy, x, bias, 2, O.ACT_RELU, 0.5, keep)
    assert dx.tolist() == [2.0, 0.0, -4.0, 8.0, 0.0]
    # z rounds in float32: 1 + 2^-30 is 1 there, so ELU takes its positive side exactly
    y, z = O.bias_act_dropout_fwd(torch.tensor([1.0]), torch.tensor([2.0 ** -30]), 1, O.ACT_ELU)
    assert z.item() == 1.0 and y.item() == 1.0
    # rate 1: everything dropped, no NaN from the infinite scale
    y, _ = O.bias_act_dropout_fwd(x, bias, 2, O.ACT_GELU, 1.0, torch.zeros(5, dtype=torch.bool))
    assert y.tolist() == [0.0] * 5


# ------------------------------------------------------------------ fp8
@pytest.mark.parametrize("e5m2", (False, True))
def test_fp8_decode_table_matches_torch(e5m2):
    table = O.fp8_decode_table(e5m2)
    ref = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(O.FP8_TORCH[e5m2]).to(F64).numpy()
    assert np.array_equal(np.isnan(table), np.isnan(ref))
    ok = ~np.isnan(table)
    assert np.array_equal(table[ok], ref[ok]) and np.array_equal(np.signbit(table[ok]), np.signbit(ref[ok]))
    assert np.nanmax(table[np.isfinite(table)]) == O.FP8_LIM[e5m2]
    assert int(np.isnan(table).sum()) == (6 if e5m2 else 2)


@pytest.mark.parametrize("e5m2", (False, True))
def test_fp8_encode_every_bf16_pattern_by_brute_force(e5m2):
    """The oracle's quantiser (float32 product, clamp, torch's cast) against the nearest table value
    with ties to the even code, for every bf16 pattern under every scale of the GPU test; the
    saturation at +-lim, +-inf and the NaN rule separately."""
    x = O.all_bf16()
    lim = O.FP8_LIM[e5m2]
    top, nan_code = (0x7B, 0xFB) if e5m2 else (0x7E, 0xFE)
    ties = 0
    for scale in O.fp8_scales():
        got = O.quant_fp8(x, scale, e5m2).numpy()
        v = (x.to(F32) * torch.tensor(scale, dtype=F32)).to(F64).numpy()
        nan = np.isnan(v)
        vc = np.clip(np.where(nan, -lim, v), -lim, lim)
        want = O.fp8_nearest(vc, e5m2)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (scale, hex(int(bad[0])), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
        assert (got[nan] == nan_code).all() and nan.sum() == 254
        assert (got[v >= lim] == top).all() and (got[v <= -lim] == (top | 0x80)).all()
        assert (got[np.isposinf(v)] == top).all() and (got[np.isneginf(v)] == (top | 0x80)).all()
        ties += int((O.fp8_nearest(vc, e5m2, half_up=True) != want).sum())
    assert ties > 100  # the patterns hold exact ties: a round-half-up encode differs there
    assert O.quant_fp8(torch.tensor([500.0, -500.0, 448.0, 464.0, 0.0, -0.0]).bfloat16(), 1.0, False).tolist() == \
        [0x7E, 0xFE, 0x7E, 0x7E, 0x00, 0x80]


@pytest.mark.parametrize("e5m2", (False, True))
def test_fp8_dequant_statement(e5m2):
    q = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    table = torch.from_numpy(O.fp8_decode_table(e5m2))
    for scale in O.fp8_scales():
        got = O.dequant_fp8(q, scale, e5m2)
        inv = (torch.tensor(1.0, dtype=F32) / torch.tensor(scale, dtype=F32)).to(F64)
        want = (table * inv).to(F32).to(BF16)        # the float64 product of two float32 rounds once to float32
        nan = torch.isnan(table)
        assert torch.equal(torch.isnan(got.float()), nan)
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), scale
    assert O.amax(torch.tensor([1.0, float("nan"), -3.0, float("-inf")]).bfloat16()) == float("inf")
    assert O.amax(torch.tensor([1.0, float("nan"), -3.0]).bfloat16()) == 3.0
    assert O.amax(torch.tensor([float("nan")]).bfloat16(), start=2.0) == 2.0


# ------------------------------------------------------------------ layouts
def test_layout_statements_match_torch():
    for C, Cp in O.PAD_CCP:
        for rows in O.PAD_ROWS:
            x = O.ramp_bf16(rows * C).view(torch.int16)
            y = O.pad_channels(x, rows, C, Cp).view(rows, Cp)
            assert torch.equal(y[:, :C], x.view(rows, C)) and bool((y[:, C:] == 0).all())
            assert torch.equal(O.unpad_channels(y.reshape(-1), rows, Cp, C), x)
    for B, A, C in O.ACA_B + tuple((1, a, c) for a, c in O.ACA_B1):
        x = O.ramp_bf16(A * B * C).view(torch.int16)
        assert torch.equal(O.transpose_aca(x, A, B, C).view(C, B, A), x.view(A, B, C).permute(2, 1, 0))
    for R, C in O.T2D:
        x = torch.arange(R * C, dtype=torch.int32)
        assert torch.equal(O.transpose2d(x, R, C).view(C, R), x.view(R, C).t())
    K, R, S, C = 5, 3, 3, 4
    x = torch.arange(K * R * S * C, dtype=torch.int32)
    w = x.view(K, R, S, C)
    assert torch.equal(O.wprep_entry(x, K, R, S, C, 1, 0, R, 0, S).view(C, R, S, K), w.permute(3, 1, 2, 0))
    assert torch.equal(O.wprep_entry(x, K, R, S, C, 2, 1, 1, 0, 2).view(C, 1, 2, K), w[:, 1::2, 0::2].permute(3, 1, 2, 0))
    # a ramp holds no two equal elements: a swapped pair inside an 8 x 8 block shows
    x = O.ramp_bf16(64).view(torch.int16)
    t = O.transpose_aca(x, 8, 1, 8).clone()
    t[[10, 17]] = t[[17, 10]]
    assert not torch.equal(t, x.view(8, 8).t().reshape(-1))


# ------------------------------------------------------------------ column sums
def test_colsum_plan_covers_what_the_cases_name():
    P = O.colsum_plan
    assert [P(r, 8, True)[0] for r in (1, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    assert P(4224, 8, True) == (66, 64) and P(65536, 8, True) == (1024, 64) and P(65536, 264, True)[0] == 512
    assert [P(r, 12, False)[0] for r in (1, 128, 129, 4224, 32768, 40000)] == [1, 1, 2, 33, 256, 255]
    assert P(0, 8, True) == (1, 1) and P(0, 3, False) == (1, 1) and O.colsum_ws_floats(0, 8) == 0
    assert O.colsum_ws_floats(64, 8) == 0 and O.colsum_ws_floats(129, 8) == 3 * 8 and O.colsum_ws_floats(4224, 12) == 66 * 12
    # the row loop of the vector form ends in each of its phases: whole 32-row trips, 8-row steps, a partial step
    assert {P(r, 8, True)[1] % 32 for r in O.COLSUM_VEC_ROWS} >= {0, 1, 7, 8, 9, 31}


def test_colsum_f32_is_a_column_sum_in_every_order():
    for rows, C in ((1, 8), (129, 8), (4224, 12), (1000, 3)):
        x = torch.randint(-8, 9, (rows, C), generator=O._gen(rows, C)).float()
        out0 = torch.randint(-8, 9, (C,), generator=O._gen(C)).float()
        want = x.double().sum(0)
        for vec in (False, True):
            for fold4 in (False, True):
                got = O.colsum_f32(x.numpy(), vec, fold4)        # small integers: exact in any order
                assert np.array_equal(got.astype(np.float64), want.numpy()), (rows, C, vec, fold4)
                got = O.colsum_f32(x.numpy(), vec, fold4, out0.numpy())
                assert np.array_equal(got.astype(np.float64), (want + out0.double()).numpy())
                if O.colsum_plan(rows, C, vec)[0] > 1:
                    assert not np.array_equal(O.colsum_f32(x.numpy(), vec, fold4, drop_last_slice=True), got)
    assert O.colsum_f32(np.zeros((0, 8), np.float32), True, True).tolist() == [0.0] * 8
    assert O.colsum(torch.zeros(0, 3))[0].tolist() == [0.0] * 3


# ------------------------------------------------------------------ float32 against float64
_maxima = {}


def _hold(figs, label):
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    for k, v in figs.items():
        _maxima[k] = max(_maxima.get(k, 0.0), v)
        assert O.bar_holds(k, v), (label, k, v, O.BARS[k])


def _fp32_act(x, bias, dy, C, kind, rate=0.0, keep=None):
    want, z = O.bias_act_dropout_fwd(x, bias, C, kind, rate, keep)
    dwant, _ = O.bias_act_dropout_bwd(dy, x, bias, C, kind, rate, keep)
    sy, sdx = O.act_scales(z, dy, rate)
    got, _ = O.bias_act_dropout_fwd(x, bias, C, kind, rate, keep, dtype=F32)
    dgot, _ = O.bias_act_dropout_bwd(dy, x, bias, C, kind, rate, keep, dtype=F32)
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(dgot).any())
    return {"act_y": O.figure(got, want, sy), "act_dx": O.figure(dgot, dwant, sdx)}


@pytest.mark.parametrize("kind", O.ACTS)
@pytest.mark.parametrize("dtype", (F32, BF16))
def test_fp32_bias_act_within_bars(dtype, kind):
    figs = {"act_y": 0.0, "act_dx": 0.0}
    for n, C, wb in O.act_cases():
        x, bias, dy = O.act_inputs(n, C, dtype, wb)
        f = _fp32_act(x, bias, dy, C, kind)
        figs = {k: max(figs[k], f[k]) for k in figs}
    _hold(figs, ("act", dtype, kind))


@pytest.mark.parametrize("rate", O.RATES[:-1])
def test_fp32_dropout_within_bars(rate):
    figs = {"act_y": 0.0, "act_dx": 0.0}
    for n, dtype, kind, (seed, offset) in O.drop_cases():
        x, bias, dy = O.drop_inputs(n, 3, dtype)
        keep = torch.from_numpy(O.keep_mask(n, rate, seed, offset))
        f = _fp32_act(x, bias, dy, 3, kind, rate, keep)
        figs = {k: max(figs[k], f[k]) for k in figs}
    _hold(figs, ("dropout", rate))


def test_fp32_colsum_in_kernel_order_within_bars():
    fig = 0.0
    for rows, C, dtype, form in O.colsum_cases():
        x, out0 = O.colsum_inputs(rows, C, dtype)
        for beta in (0, 1):
            base = out0 if beta else None
            want, mag = O.colsum(x, base)
            for fold4 in ((True, False) if C % 4 == 0 else (False,)):
                got = O.colsum_f32(x.float().numpy(), form == "vec", fold4, None if base is None else base.numpy())
                fig = max(fig, O.figure(torch.from_numpy(got), want, mag))
            if form == "vec":   # the same input from a pointer that is not 16-byte aligned: the scalar form
                got = O.colsum_f32(x.float().numpy(), False, False, None if base is None else base.numpy())
                fig = max(fig, O.figure(torch.from_numpy(got), want, mag))
    _hold({"colsum": fig}, "colsum")


def test_zz_report_fp32_maxima():
    """Runs last in this file: the float32 maxima of the tests above beside their bars; every bar
    has a measured figure."""
    for k in sorted(_maxima):
        print("%-10s fp32 max %.3e   bar %.1e" % (k, _maxima[k], O.BARS[k]))
    assert set(_maxima) == set(O.BARS)
    for k, v in _maxima.items():
        assert O.MARGIN * max(v, O.FLOOR) <= O.BARS[k]
