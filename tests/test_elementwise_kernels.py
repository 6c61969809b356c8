"""The kernels of csrc/kernels/elementwise.hip (casts, channel pads, filter transposes and the
filter-preparation gather, bias + activation + Philox dropout forward and backward, the bias-gradient
column sums, add_bf16, amax, the fp8 quantiser and dequantiser) against the statements of
tests/elementwise_oracle.py, at the smallest shapes at which each can still go wrong: every vector
body with its scalar tail, one trip round each grid-stride loop, every kernel a dispatch can pick
(aligned and misaligned pointers included), every slice count and fold of the column sums.

What moves or selects bits is compared exactly: the casts (any NaN standing for a NaN), add_bf16
(bit for bit: with the coefficients used both products are exact in float32, so the one rounding of
the sum is the same whether or not the compiler contracts it to an FMA), the layouts on distinct bit
patterns, the set of dropped positions against an independent Philox4x32-10, amax, every fp8 code of
every bf16 pattern, every bf16 of every fp8 code, and every column sum against itself when repeated.
What is computed is compared element-wise, |got - want| <= half a bf16 ulp of want (bf16 outputs
only: the store) + bar * scale. A bar is 16 x the largest value the same figure takes when the
oracle itself runs in float32 (for colsum: in the kernels' order;
tests/test_elementwise_oracle_cpu.py), never less than 16 x 2^-24. Outputs and workspaces sit
between guard elements of a fixed byte pattern that must survive, and start out as the pattern.

Pinned as it is (a NaN is laundered, not propagated): quant_fp8 clamps with fminf(fmaxf(v, -lim),
lim), which returns -lim for a NaN, so a NaN input is stored as the code of -lim (0xfe e4m3, 0xfb
e5m2); amax passes over NaNs (fmaxf again).

Largest figure of any case on an MI355X, beside its bar (fp32: the float32 oracle):

  figure     MI355X     fp32      bar
  act_y      1.42e-7    1.43e-7   3e-6   (both at rate 0.01: the rounding of act(z) and of the scale)
  act_dx     2.14e-7    2.33e-7   4e-6   (GELU's 1 - tanh^2 near saturation, times its polynomial)
  colsum     9.9e-8     9.9e-8    2e-6   (the same value: the float32 run adds in the kernels' order)
"""
import pytest
import torch

import elementwise_oracle as O
from tensorflow_train_distributed_amd.ops import _lib
from tensorflow_train_distributed_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, U8, I16, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int16, torch.int32
PATTERN = 0x5A
DT = {F32: 0, BF16: 1}

_seen = {}


def _check(figs, label):
    for k, v in figs.items():
        _seen[k] = max(_seen.get(k, 0.0), v) if v == v else v
    print(label, {k: "%.2e" % v for k, v in figs.items()})
    return O.check(figs, label)


class Guarded:
    """A flat tensor `t` of n elements with at least O.GUARD elements of the byte PATTERN on either
    side in one allocation, starting `offset` elements past a 16-byte boundary; `t` starts out as
    the pattern too, so what a kernel leaves unwritten shows."""

    def __init__(self, n, dtype, offset=0):
        item = torch.empty((), dtype=dtype).element_size()
        self.n = int(n) * item
        self.g = (O.GUARD * item + 15) // 16 * 16 + offset * item
        self.raw = torch.full((2 * self.g + self.n,), PATTERN, dtype=U8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.g:self.g + self.n].view(dtype)

    def intact(self):
        return bool((self.raw[:self.g] == PATTERN).all()) and bool((self.raw[self.g + self.n:] == PATTERN).all())

    def untouched(self):
        return bool((self.raw == PATTERN).all())


def _offset_copy(t, offset=1):
    """A copy of flat `t` that starts `offset` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8 + offset, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + t.numel()]
    out.copy_(t)
    return out


def _bits(t):
    t = t.contiguous()
    return t.view({BF16: I16, F32: I32, U8: U8, I16: I16, I32: I32}[t.dtype])


def _same_bits(a, b):
    return torch.equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def _same_values(got, ref):
    """Bit for bit, any NaN standing for any NaN."""
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return torch.equal(gn, rn) and bool((gn | (_bits(got) == _bits(ref))).all())


def _p(t):
    return None if t is None else t.data_ptr()


def _call(name, *args):
    _lib.call(name, *args, _lib.stream())


def _refused(name, *args):
    with pytest.raises(_lib.HipKernelError):
        _call(name, *args)


# ------------------------------------------------------------------ casts, add
def _random_f32_bits(n):
    """Every exponent, denormals, infinities and NaNs: random 32-bit patterns."""
    gen = torch.Generator(device=DEV).manual_seed(n % 9973)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, device=DEV, dtype=torch.int64).to(I32).view(F32)


@pytest.mark.parametrize("n", O.CAST_N + (O.CAST_WRAP,))
def test_f32_to_bf16(n):
    """The 4-wide body and the scalar tail; CAST_WRAP: five elements past one trip of 16384 blocks."""
    x = _random_f32_bits(n)
    if n >= 7:
        x[:7] = torch.tensor([0.0, -0.0, float("inf"), float("nan"), 1.00390625, 1.01171875, 3.3e38], device=DEV)
    y = Guarded(n, BF16)
    _call("ttdk_f32_to_bf16", _p(x), _p(y.t), n)
    assert y.intact()
    assert _same_values(y.t, x.to(BF16))
    if n:
        assert _same_bits(K.f32_to_bf16(x), y.t)


def test_bf16_to_f32_every_pattern():
    x = O.all_bf16(DEV)
    y = Guarded(65536, F32)
    _call("ttdk_bf16_to_f32", _p(x), _p(y.t), 65536)
    assert y.intact()
    assert torch.equal(_bits(y.t), torch.arange(65536, dtype=I32, device=DEV) << 16)   # NaN payloads too
    y0 = Guarded(0, F32)
    _call("ttdk_bf16_to_f32", _p(x), _p(y0.t), 0)
    assert y0.untouched()


@pytest.mark.parametrize("n", O.ADD_N)
def test_add_bf16(n):
    gen = torch.Generator().manual_seed(n)
    a = (torch.randn(n, generator=gen) * 4).bfloat16().to(DEV)
    b = (torch.randn(n, generator=gen) * 4).bfloat16().to(DEV)
    a[:4] = torch.tensor([3.0, -0.0, 1e30, 256.0], device=DEV).bfloat16()
    b[:4] = torch.tensor([3.0, 0.0, 1e30, 1.0], device=DEV).bfloat16()       # 3 - 3, a cancelled pair, 256 + 1: a tie
    for alpha, beta in O.ADD_COEF:
        y = Guarded(n, BF16)
        _call("ttdk_add_bf16", _p(a), _p(b), _p(y.t), n, alpha, beta)
        assert y.intact()
        want = (alpha * a.float() + beta * b.float()).to(BF16)   # both products exact: one float32 rounding, then RNE
        assert _same_bits(y.t, want), (n, alpha, beta)
        inplace = a.clone()
        _call("ttdk_add_bf16", _p(inplace), _p(b), _p(inplace), n, alpha, beta)
        assert _same_bits(inplace, want), (n, alpha, beta)
    y = Guarded(16, BF16)
    _refused("ttdk_add_bf16", _p(a), _p(b), _p(y.t), 12, 1.0, 1.0)
    torch.cuda.synchronize()
    assert y.untouched()


# ------------------------------------------------------------------ channel pads
def _payloads(n):
    """n distinct bf16 patterns (n < 65536) that run through +inf, the NaNs and -0."""
    return O.ramp_bf16(n, DEV, start=0x7F00)


@pytest.mark.parametrize("C,Cp", O.PAD_CCP)
def test_pad_unpad_channels(C, Cp):
    for rows in O.PAD_ROWS:
        x = _payloads(rows * C)
        y = Guarded(rows * Cp, BF16)
        _call("ttdk_pad_channels", _p(x), _p(y.t), rows, C, Cp)
        assert y.intact()
        want = O.pad_channels(_bits(x), rows, C, Cp)
        assert torch.equal(_bits(y.t), want), (rows, C, Cp)
        assert bool((_bits(y.t).view(rows, Cp)[:, C:] == 0).all())       # the pad lanes: +0 exactly
        back = Guarded(rows * C, BF16)
        _call("ttdk_unpad_channels", _p(y.t), _p(back.t), rows, Cp, C)
        assert back.intact()
        assert torch.equal(_bits(back.t), O.unpad_channels(want, rows, Cp, C))
        assert _same_bits(back.t, x), (rows, C, Cp)                       # the round trip
        if rows:
            assert _same_bits(K.pad_channels(x.view(rows, C), Cp), y.t)


@pytest.mark.parametrize("rows", (8, 816, 8 * 257))
def test_pad3to8_fast_and_generic_agree(rows):
    """3 -> 8 with rows % 8 == 0: the 16-byte kernel from an aligned source into an aligned
    destination, the generic kernel when either is one element off; the same bits."""
    x = _payloads(rows * 3)
    want = O.pad_channels(_bits(x), rows, 3, 8)
    outs = []
    for src, off in ((x, 0), (_offset_copy(x), 0), (x, 1)):
        assert (src.data_ptr() % 16 == 0) == (src is x)
        y = Guarded(rows * 8, BF16, offset=off)
        _call("ttdk_pad_channels", _p(src), _p(y.t), rows, 3, 8)
        assert y.intact()
        assert torch.equal(_bits(y.t), want), (rows, src is x, off)
        outs.append(y.t)
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])


# ------------------------------------------------------------------ transposes
def _aca(src, A, B, C, offset=0):
    dst = Guarded(A * B * C, BF16, offset=offset)
    _call("ttdk_transpose_aca_bf16", _p(src), _p(dst.t), A, B, C)
    assert dst.intact()
    return dst.t


@pytest.mark.parametrize("B,A,C", tuple((1, a, c) for a, c in O.ACA_B1) + O.ACA_B + ((1, 256, 384),))
def test_transpose_aca(B, A, C):
    """B = 1: the 128 x 128 tile kernel (multiples of 128), the 8 x 8 register-block kernel
    (multiples of 8), the 32 x 32 LDS-tile kernel (the rest, and every B > 1), each at its smallest
    shape, one past it and with partial tiles; distinct bit patterns."""
    src = O.ramp_bf16(A * B * C, DEV)
    want = O.transpose_aca(_bits(src), A, B, C)
    assert torch.equal(_bits(_aca(src, A, B, C)), want)
    if B == 1 and A % 8 == 0 and C % 8 == 0:
        # a source or a destination that is not 16-byte aligned takes the LDS-tile kernel: still exact
        assert torch.equal(_bits(_aca(_offset_copy(src), A, B, C)), want)
        assert torch.equal(_bits(_aca(src, A, B, C, offset=1)), want)
    assert _same_bits(K.krsc_to_crsk(src.view(A, 1, B, C)), want)


@pytest.mark.parametrize("R,C", O.T2D)
def test_transpose2d_f32(R, C):
    src = (torch.arange(R * C, dtype=I32, device=DEV) + 0x7F7FFFF0).view(F32)   # distinct; +inf and NaNs among them
    dst = Guarded(R * C, F32)
    _call("ttdk_transpose2d_f32", _p(src), _p(dst.t), R, C)
    assert dst.intact()
    assert torch.equal(_bits(dst.t), O.transpose2d(_bits(src), R, C))


def test_transpose_batch_per_entry():
    shapes = [(128, 256), (256, 128), (128, 128)]
    src = [O.ramp_bf16(a * c, DEV, start=1 + 7 * i).view(a, c) for i, (a, c) in enumerate(shapes)]
    dst = [Guarded(a * c, BF16) for a, c in shapes]
    K.TransposeBatch([(s_, d_.t.view(s_.shape[1], s_.shape[0])) for s_, d_ in zip(src, dst)]).run()
    for (a, c), s_, d_ in zip(shapes, src, dst):
        assert d_.intact()
        assert torch.equal(_bits(d_.t), O.transpose_aca(_bits(s_), a, 1, c)), (a, c)


def test_weight_prep_entries_by_index():
    """K = 40, C = 24, 3 x 3 (partial 32 x 32 tiles both ways) from an unaligned offset: the plain
    [C][R][S][K] transpose and the four stride-2 phase filters, every table row against the gather
    written out by index."""
    Kc, R, S, C = 40, 3, 3, 24
    n = Kc * R * S * C
    flat = O.ramp_bf16(n + 3, DEV)
    wp = K.WeightPrep(flat)
    wp.add("w", 3, (Kc, R, S, C))
    wp.add("w/phases", 3, (Kc, R, S, C), sub=(2, 1, 1, 15, 13))
    wp.build()
    buf = Guarded(wp.buf.numel(), BF16)
    wp.buf = buf.t
    wp.run()
    assert buf.intact() and buf.n == 2 * n * 2          # the phases partition the nine taps
    w = _bits(flat[3:])
    taps = []
    for off, dst, k_, r_, s_, c_, s, r0, Tr, s0, Ts, _ in wp._rows:
        assert (off, k_, r_, s_, c_) == (3, Kc, R, S, C)
        want = O.wprep_entry(w[:n], Kc, R, S, C, s, r0, Tr, s0, Ts)
        assert torch.equal(_bits(buf.t[dst:dst + want.numel()]), want), (s, r0, Tr, s0, Ts)
        if s == 2:
            taps += [(r0 + tr * s, s0 + ts * s) for tr in range(Tr) for ts in range(Ts)]
    assert sorted(taps) == [(r, q) for r in range(R) for q in range(S)]
    assert torch.equal(_bits(wp.crsk("w")).reshape(-1), O.transpose_aca(w[:n], Kc, R * S, C))


# ------------------------------------------------------------------ bias + activation + dropout
def _bad(x, bias, dy, n, C, kind, rate, seed, offset):
    """(y, dx) of the two kernels on flat device tensors, through the entry points themselves."""
    y, dx = Guarded(n, x.dtype), Guarded(n, x.dtype)
    _call("ttdk_bias_act_dropout_fwd", _p(x), _p(bias), _p(y.t), n, C, kind, float(rate), seed, offset, DT[x.dtype])
    _call("ttdk_bias_act_dropout_bwd", _p(dy), _p(x), _p(bias), _p(dx.t), n, C, kind, float(rate), seed, offset, DT[x.dtype])
    assert y.intact() and dx.intact()
    return y.t, dx.t


def _act_figures(y, dx, x, bias, dy, C, kind, rate=0.0, keep=None):
    want, z = O.bias_act_dropout_fwd(x, bias, C, kind, rate, keep)
    dwant, _ = O.bias_act_dropout_bwd(dy, x, bias, C, kind, rate, keep)
    sy, sdx = O.act_scales(z, dy, rate)
    bf = x.dtype == BF16
    return {"act_y": O.figure(y, want, sy, bf16_store=bf), "act_dx": O.figure(dx, dwant, sdx, bf16_store=bf)}


@pytest.mark.parametrize("kind", O.ACTS)
@pytest.mark.parametrize("dtype", (F32, BF16))
def test_bias_act_rate0(dtype, kind):
    figs = {"act_y": 0.0, "act_dx": 0.0}
    for n, C, wb in O.act_cases():
        x, bias, dy = (None if t is None else t.to(DEV) for t in O.act_inputs(n, C, dtype, wb))
        y, dx = _bad(x, bias, dy, n, C, kind, 0.0, 0, 0)
        assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(dx).any()), (n, C, wb)
        f = _act_figures(y, dx, x, bias, dy, C, kind)
        figs = {k: max(figs[k], f[k]) if f[k] == f[k] else f[k] for k in figs}
        if n == 1023 and not (wb and C == 1):
            # the branches at the planted zeros: exactly the stated side
            z0 = O.dact(torch.zeros(1), kind).item()
            assert dx[0].item() == dy[0].item() * z0 and dx[C].item() == dy[C].item() * z0, (C, wb)
    _check(figs, ("rate0", dtype, kind))


@pytest.mark.parametrize("dtype", (F32, BF16))
def test_gelu_derivative_far_out(dtype):
    """Where z*z overflows float32 (|z| above 1.8e19) the derivative is 1 and 0, not 0 * inf."""
    x = torch.tensor([1e20, -1e20, 2e19, -2e19, 3e38, -3e38, 1e13, -1e13], device=DEV).to(dtype)
    dy = torch.tensor([1.0, 1.0, -2.0, -2.0, 3.0, 3.0, 0.5, 0.5], device=DEV).to(dtype)
    y, dx = _bad(x, None, dy, 8, 1, O.ACT_GELU, 0.0, 0, 0)
    assert dx.tolist() == [1.0, 0.0, -2.0, 0.0, 3.0, 0.0, 0.5, 0.0]
    assert y[0::2].tolist() == x[0::2].tolist() and y[1::2].tolist() == [0.0] * 4


@pytest.mark.parametrize("rate", O.RATES)
def test_dropout_mask_equals_philox(rate):
    """The set of zeroed positions is the complement of keep_mask, position by position, in the
    forward and in the backward; the kept values are within the bars; rate 1 leaves zeros."""
    figs = {"act_y": 0.0, "act_dx": 0.0}
    for n, dtype, kind, (seed, offset) in O.drop_cases():
        x, bias, dy = (t.to(DEV) for t in O.drop_inputs(n, 3, dtype))
        y, dx = _bad(x, bias, dy, n, 3, kind, rate, seed, offset)
        keep = torch.from_numpy(O.keep_mask(n, rate, seed, offset)).to(DEV)
        label = (rate, n, dtype, kind, seed, offset)
        assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(dx).any()), label
        assert torch.equal(y != 0, keep), (label, (y != 0).nonzero()[:8].flatten().tolist(), keep.nonzero()[:8].flatten().tolist())
        assert torch.equal(dx != 0, keep), label
        if rate < 1.0:
            f = _act_figures(y, dx, x, bias, dy, 3, kind, rate, keep)
            figs = {k: max(figs[k], f[k]) if f[k] == f[k] else f[k] for k in figs}
        else:
            assert not bool(keep.any())
    if rate < 1.0:
        _check(figs, ("dropout", rate))


def test_dropout_mask_past_one_grid_trip():
    """16384 x 256 + 1027 ones at rate 0.25: element idx >= 2^22 takes counter idx >> 2 all the
    same; y is exactly keep * float32(1 / 0.75), and the wrapper gives the same."""
    n, rate, seed, offset = O.ACT_WRAP, 0.25, 7, 3
    x = torch.ones(n, device=DEV)
    y, dx = _bad(x, None, x, n, 8, O.ACT_NONE, rate, seed, offset)
    keep = torch.from_numpy(O.keep_mask(n, rate, seed, offset)).to(DEV)
    want = torch.where(keep, torch.full_like(x, O.drop_scale(rate)), torch.zeros_like(x))
    assert torch.equal(y, want) and torch.equal(dx, want)
    assert torch.equal(K.bias_act_dropout(x[:4096].view(-1, 8), None, K.ACT_NONE, rate=rate, seed=seed, offset=offset).view(-1),
                       want[:4096])


# ------------------------------------------------------------------ column sums
def _colsum(x2d, rows, C, out, beta, ws):
    _call("ttdk_colsum", _p(x2d), rows, C, _p(out.t), beta, DT[x2d.dtype], _p(ws.t))
    assert out.intact() and ws.intact()
    return out.t.clone()


def _colsum_case(rows, C, dtype, x_offset=0, out_offset=0):
    """Both beta values on one input: the bar, twice the same bits, guards around out and around a
    workspace of exactly the floats asked for; returns the largest figure."""
    xc, out0 = O.colsum_inputs(rows, C, dtype)
    x = xc.to(DEV)
    if x_offset:
        x = _offset_copy(x.reshape(-1), x_offset).view(rows, C)
    nws = _lib.query("ttdk_colsum_ws_floats", rows, C, DT[dtype])
    assert nws == O.colsum_ws_floats(rows, C), (rows, C, nws)
    fig = 0.0
    for beta in (0, 1):
        base = out0.to(DEV) if beta else None
        want, mag = O.colsum(x, base)
        got = []
        for _ in range(2):
            out, ws = Guarded(C, F32, offset=out_offset), Guarded(nws, F32)
            if beta:
                out.t.copy_(base)
            got.append(_colsum(x, rows, C, out, beta, ws))
        assert _same_bits(got[0], got[1]), (rows, C, dtype, beta)
        f = O.figure(got[0], want, mag)
        assert f == f, (rows, C, dtype, beta)
        fig = max(fig, f)
    return fig


@pytest.mark.parametrize("C", O.COLSUM_VEC_C)
def test_colsum_vector_form(C):
    """bf16, C % 8 == 0: one, two and three slices, the row loop ending in each of its phases."""
    fig = max(_colsum_case(rows, C, BF16) for rows in O.COLSUM_VEC_ROWS)
    _check({"colsum": fig}, ("colsum vec", C))


@pytest.mark.parametrize("rows,C", O.COLSUM_VEC_BIG)
def test_colsum_vector_form_many_slices(rows, C):
    """66 slices (more than the 32 lanes of the parallel fold) and the cap of 1024."""
    _check({"colsum": _colsum_case(rows, C, BF16)}, ("colsum vec", rows, C))


@pytest.mark.parametrize("C", O.COLSUM_SCALAR_C)
@pytest.mark.parametrize("dtype", (F32, BF16))
def test_colsum_scalar_form(dtype, C):
    """One and two slices, 33 slices (into the parallel fold at C = 12, the serial fold elsewhere)
    and the cap of 256."""
    fig = max(_colsum_case(rows, C, dtype) for rows in O.COLSUM_SCALAR_ROWS)
    _check({"colsum": fig}, ("colsum scalar", dtype, C))


def test_colsum_misaligned_pointers():
    """bf16 with C % 8 == 0 one element off a 16-byte boundary takes the scalar kernels; `out` one
    float off takes the serial fold."""
    fig = max(_colsum_case(rows, C, BF16, x_offset=1) for C in (8, 264) for rows in (129, 4224))
    fig = max(fig, _colsum_case(4224, 8, BF16, out_offset=1), _colsum_case(4224, 12, F32, out_offset=1),
              _colsum_case(129, 264, BF16, out_offset=1))
    _check({"colsum": fig}, "colsum misaligned")


@pytest.mark.parametrize("dtype", (F32, BF16))
def test_colsum_of_no_rows(dtype):
    """rows == 0: zeros with beta = 0, `out` as it was with beta = 1, no workspace."""
    for C in (8, 3):
        assert _lib.query("ttdk_colsum_ws_floats", 0, C, DT[dtype]) == 0
        x = torch.empty(0, C, dtype=dtype, device=DEV)
        planted = torch.arange(1, C + 1, dtype=F32, device=DEV)
        for beta in (0, 1):
            out, ws = Guarded(C, F32), Guarded(0, F32)
            out.t.copy_(planted)
            got = _colsum(x, 0, C, out, beta, ws)
            assert got.tolist() == (planted.tolist() if beta else [0.0] * C), (C, beta)
        assert K.colsum(x).tolist() == [0.0] * C


# ------------------------------------------------------------------ amax
def _amax(x, start=None):
    """reset unless `start` is given; the result sits between guards."""
    out = Guarded(1, F32)
    if start is not None:
        out.t.fill_(start)
    _call("ttdk_amax_bf16", _p(x), x.numel(), _p(out.t), int(start is None))
    assert out.intact()
    return out.t.item()


@pytest.mark.parametrize("n", O.AMAX_N)
def test_amax(n):
    x = (torch.randn(n, generator=O._gen(n, 9)) * 3).bfloat16().to(DEV)
    assert _amax(x) == O.amax(x)
    assert _amax(x, 1000.0) == 1000.0 and _amax(x, 0.0078125) == O.amax(x, 0.0078125)    # reset=False
    if n:
        x[n // 2] = -50.0
        assert _amax(x) == 50.0 and K.amax(x).item() == 50.0
        x[n - 1] = float("nan")      # passed over: fmaxf(m, NaN) is m, in the loop and in the wave reduction
        assert _amax(x) == O.amax(x) and (n == 1 or _amax(x) == 50.0)
        x[0] = float("-inf")
        assert _amax(x) == float("inf")
        assert _amax(torch.full((n,), -0.0, device=DEV).bfloat16()) == 0.0


# ------------------------------------------------------------------ fp8
def _scale_t(scale):
    return torch.tensor([scale], dtype=F32, device=DEV)


@pytest.mark.parametrize("e5m2", (False, True))
def test_quant_fp8_every_pattern(e5m2):
    """Every bf16 pattern under every scale, bit for bit: ties, the fp8 subnormals, signed zeros,
    saturation, +-inf -> +-max. A NaN input is stored as the code of -lim (0xfe / 0xfb): the clamp
    fminf(fmaxf(v, -lim), lim) returns -lim for a NaN. The tensor-list quantiser of fp8.hip clamps
    the same way."""
    x = O.all_bf16(DEV)
    nan = torch.isnan(x)
    for scale in O.fp8_scales():
        q = Guarded(65536, U8)
        _call("ttdk_quant_fp8", _p(x), _p(q.t), 65536, _p(_scale_t(scale)), int(e5m2))
        assert q.intact()
        want = O.quant_fp8(x.cpu(), scale, e5m2).to(DEV)
        bad = (q.t != want).nonzero().flatten()
        assert bad.numel() == 0, (scale, bad.numel(), [(hex(int(i)), hex(int(q.t[i])), hex(int(want[i]))) for i in bad[:8]])
        assert bool((q.t[nan] == (0xFB if e5m2 else 0xFE)).all())
    # a tail past the patterns, the wrapper, and nothing at all
    n = O.FP8_TAIL
    xt = torch.cat([x, x[0x3F80:0x3F83]])
    q = Guarded(n, U8)
    s = _scale_t(3.0)
    _call("ttdk_quant_fp8", _p(xt), _p(q.t), n, _p(s), int(e5m2))
    assert q.intact() and torch.equal(q.t, O.quant_fp8(xt.cpu(), 3.0, e5m2).to(DEV))
    assert torch.equal(K.quant_fp8(xt, s, e5m2=e5m2), q.t)
    q0 = Guarded(0, U8)
    _call("ttdk_quant_fp8", _p(xt), _p(q0.t), 0, _p(s), int(e5m2))
    assert q0.untouched()


@pytest.mark.parametrize("e5m2", (False, True))
def test_dequant_fp8_every_code(e5m2):
    codes = torch.arange(256, dtype=I32, device=DEV).to(U8)
    for scale in O.fp8_scales():
        x = Guarded(256, BF16)
        _call("ttdk_dequant_fp8", _p(codes), _p(x.t), 256, _p(_scale_t(scale)), int(e5m2))
        assert x.intact()
        assert _same_values(x.t, O.dequant_fp8(codes.cpu(), scale, e5m2).to(DEV)), scale
        assert int(torch.isnan(x.t).sum()) == (6 if e5m2 else 2)
    n = O.FP8_TAIL
    q = (torch.arange(n, dtype=I32, device=DEV) % 256).to(U8)
    x = Guarded(n, BF16)
    s = _scale_t(0.5)
    _call("ttdk_dequant_fp8", _p(q), _p(x.t), n, _p(s), int(e5m2))
    assert x.intact() and _same_values(x.t, O.dequant_fp8(q.cpu(), 0.5, e5m2).to(DEV))
    assert _same_values(K.dequant_fp8(q, s, e5m2=e5m2), x.t)
    x0 = Guarded(0, BF16)
    _call("ttdk_dequant_fp8", _p(q), _p(x0.t), 0, _p(s), int(e5m2))
    assert x0.untouched()


def test_zz_report_gpu_maxima():
    """Runs last in this file: the largest figure of the tests above beside its bar."""
    for k in sorted(_seen):
        print("%-10s gpu max %.3e   bar %.1e" % (k, _seen[k], O.BARS[k]))
    assert set(_seen) == set(O.BARS)
