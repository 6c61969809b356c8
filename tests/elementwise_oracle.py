"""What tests/test_elementwise_kernels.py (GPU) and tests/test_elementwise_oracle_cpu.py share (a
plain module, imported by them): plain statements of the operations of csrc/kernels/elementwise.hip,
written from the definitions below and not from the kernels (numpy / torch, whole tensors, float64
unless `dtype=` says otherwise: the float32 run is how the bars are set), the case tables, the
seeded inputs and the bars. figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and
check() are those of tests/transformer_oracle.py; BARS below is entered into its table.

Definitions:

  dropout mask   element idx is kept when uniform(r[idx & 3]) >= rate, r = Philox4x32-10 of the
                 counter (lo32(idx >> 2), hi32(idx >> 2), lo32(offset), hi32(offset)) under the key
                 (lo32(seed), hi32(seed)); uniform(r) = float32(r >> 8) * 2^-24; rate is a C float
  bias_act_dropout  z = float32(x) + float32(bias[idx % C]) (one float32 addition: every branch
                 on z is then on the kernel's side), y = keep ? act(z) * s : 0 with
                 s = float32(1 / (1 - rate)) (1 at rate 0), dx = (keep ? dy * s : 0) * act'(z);
                 act: none, ReLU, tanh-GELU 0.5 z (1 + tanh(k0 (z + k1 z^3))), ELU (expm1 for z <= 0);
                 act'(0) is 0 for ReLU and 1 for ELU; the GELU derivative is 1 / 0 far out on the
                 positive / negative side (where 1 - tanh^2 is 0 the second term is 0, whatever
                 the polynomial beside it)
  colsum         out[c] = (beta ? out[c] : 0) + sum_r x[r][c]
  quant_fp8      code = RNE-encode(fmin(fmax(float32(x) * scale, -lim), lim)), lim = 448 (e4m3fn) or
                 57344 (e5m2); fmax / fmin return their other argument for a NaN, so a NaN input
                 gives the code of -lim (0xfe / 0xfb); +-inf saturate to +-lim
  dequant_fp8    x = bf16-RNE(decode(code) * float32(1 / scale)); the NaN codes give NaN
  amax           max |x| (a maximum of bf16 magnitudes: exact); NaNs are passed over
  layouts        pad / unpad of the channel axis, [A][B][C] -> [C][B][A], fp32 [R][C] -> [C][R], and
                 the filter-preparation gather dst[c][tr][ts][k] = src[k][r0 + tr*s][s0 + ts*s][c],
                 each by index arithmetic on the flat buffers, on bit patterns

Figures (element-wise, max |got - want| / scale, half a bf16 ulp of `want` taken off for a bf16
store): act_y on max(1, |z|) / (1 - rate), act_dx on |dy| max(1, |z|) / (1 - rate), colsum on
sum_r |x| + |out0|. Everything else is compared exactly and has no bar."""
import numpy as np
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
K0, K1 = 0.7978845608028654, 0.044715
ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU = 0, 1, 2, 3
ACTS = (ACT_NONE, ACT_RELU, ACT_GELU, ACT_ELU)

# ------------------------------------------------------------------ Philox4x32-10
_M32 = np.uint64(0xFFFFFFFF)
_PH_M0, _PH_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PH_W0, _PH_W1 = 0x9E3779B9, 0xBB67AE85
_SH32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC11): ten rounds of
        (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
    the key bumped by the Weyl constants (W0, W1) after each round. counter4: four 32-bit words
    (ints or equal-length arrays), key2: two ints. Returns four uint64 arrays of 32-bit values."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _M32 for w in counter4]
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _PH_M0 * c[0], _PH_M1 * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _SH32) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> _SH32) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + _PH_W0) & 0xFFFFFFFF, (k1 + _PH_W1) & 0xFFFFFFFF
    return c


def keep_mask(n, rate, seed, offset):
    """bool numpy [n]: True where element idx survives dropout at `rate` (see the module's text)."""
    if n == 0:
        return np.zeros(0, dtype=bool)
    ctr = np.arange((n + 3) // 4, dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    zero = np.zeros_like(ctr)
    r = philox4x32_10((ctr & _M32, ctr >> _SH32, zero + np.uint64(offset & 0xFFFFFFFF), zero + np.uint64(offset >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    words = np.stack(r, axis=1).reshape(-1)[:n]    # element idx takes word idx & 3 of counter idx >> 2
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(rate)


def drop_scale(rate):
    """float32 1 / (1 - rate) as a Python float (1 at rate 0, inf at rate 1)."""
    rate = np.float32(rate)
    if not rate > 0:
        return 1.0
    with np.errstate(divide="ignore"):
        return float(np.float32(1.0) / (np.float32(1.0) - rate))


# ------------------------------------------------------------------ bias + activation + dropout
def pre_activation(x, bias, C):
    """z float32 [n]: float32(x) + float32(bias[idx % C]), one float32 addition."""
    z = x.reshape(-1).to(F32)
    if bias is not None:
        z = z + bias.to(F32)[torch.arange(z.numel(), device=z.device) % C]
    return z


def act(z, kind, dtype=F64):
    z = z.to(dtype)
    if kind == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if kind == ACT_GELU:
        return 0.5 * z * (1 + torch.tanh(K0 * (z + K1 * z * z * z)))
    if kind == ACT_ELU:
        return torch.where(z > 0, z, torch.expm1(z))
    return z


def dact(z, kind, dtype=F64):
    z = z.to(dtype)
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if kind == ACT_RELU:
        return torch.where(z > 0, one, zero)
    if kind == ACT_GELU:
        t = torch.tanh(K0 * (z + K1 * z * z * z))
        s = 1 - t * t
        # where tanh has reached +-1 the second term is 0: z * s * (a polynomial in z) -> 0 faster
        # than any power grows, and must not be formed as 0 * inf
        zz = torch.where(s == 0, zero, z)
        return 0.5 * (1 + t) + 0.5 * zz * s * K0 * (1 + 3 * K1 * zz * zz)
    if kind == ACT_ELU:
        return torch.where(z > 0, one, torch.exp(z))
    return one


def _mask_scale(v, keep, rate, dtype):
    if not rate > 0:
        return v
    s = torch.tensor(drop_scale(rate), dtype=dtype, device=v.device)
    return torch.where(keep, v * s, torch.zeros_like(v))


def bias_act_dropout_fwd(x, bias, C, kind, rate=0.0, keep=None, dtype=F64):
    """(y [n] in `dtype`, z float32 [n]); keep: bool tensor [n] (keep_mask) when rate > 0."""
    z = pre_activation(x, bias, C)
    return _mask_scale(act(z, kind, dtype), keep, rate, dtype), z


def bias_act_dropout_bwd(dy, x, bias, C, kind, rate=0.0, keep=None, dtype=F64):
    """(dx [n] in `dtype`, z float32 [n])."""
    z = pre_activation(x, bias, C)
    g = _mask_scale(dy.reshape(-1).to(dtype), keep, rate, dtype)
    return g * dact(z, kind, dtype), z


def act_scales(z, dy, rate):
    """(scale of act_y, scale of act_dx) float64 [n]."""
    m = z.to(F64).abs().clamp_min(1.0) * drop_scale(rate)
    return m, (m * dy.reshape(-1).to(F64).abs() if dy is not None else None)


# ------------------------------------------------------------------ column sums
def colsum_plan(rows, C, vec):
    """(slices, rows per slice) of a column sum, restated to pick shapes and the float32 order:
    the vector form aims at 1024 blocks with at least 64 rows a slice, the scalar form at 128
    rows a slice and at most 256 slices; an empty input is one empty slice."""
    if vec:
        cblocks = (C + 255) // 256
        sl = min((1024 + cblocks - 1) // cblocks, (rows + 63) // 64)
    else:
        sl = min((rows + 127) // 128, 256)
    sl = max(sl, 1)
    per = max((rows + sl - 1) // sl, 1)
    return max((rows + per - 1) // per, 1), per


def colsum_ws_floats(rows, C):
    sl = max(colsum_plan(rows, C, True)[0], colsum_plan(rows, C, False)[0])
    return sl * C if sl > 1 else 0


def colsum(x, out0=None):
    """(float64 column sums (+ out0), sum_r |x| + |out0|) of x [rows, C]."""
    v = x.to(F64)
    s, mag = v.sum(0), v.abs().sum(0)
    if out0 is not None:
        s, mag = s + out0.to(F64), mag + out0.to(F64).abs()
    return s, mag


def _seq(a):
    """float32 sum over axis 0 in index order, starting from 0."""
    acc = np.zeros(a.shape[1:], dtype=np.float32)
    for i in range(a.shape[0]):
        acc = acc + a[i]
    return acc


def _pad0(a, n):
    """`a` with zeros appended along axis 0 up to n entries (s + 0 = s: the order is unchanged)."""
    return a if a.shape[0] == n else np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:], dtype=a.dtype)])


def colsum_f32(x, vec, fold4, out0=None, drop_last_slice=False):
    """The column sum in float32 in the order of the kernels. x: float32 numpy [rows, C]; vec:
    eight row lanes per slice (lane l takes rows l, l + 8, ... of the slice in order, the lanes
    are folded 0..7), else one sequential run per slice; one slice adds out0 itself, more slices
    are folded serially, or (fold4) by 32 lanes (lane l takes slices l, l + 32, ...) folded 0..31.
    drop_last_slice: a deliberately wrong fold, for the tests of the tests."""
    x = np.asarray(x, dtype=np.float32)
    rows, C = x.shape
    slices, per = colsum_plan(rows, C, vec)
    xs = _pad0(x, slices * per).reshape(slices, per, C)
    if vec:
        steps = (per + 7) // 8
        lanes = _pad0(xs.transpose(1, 0, 2), steps * 8).reshape(steps, 8, slices, C)
        part = _seq(_seq(lanes))                       # [8, slices, C] -> [slices, C]
    else:
        part = _seq(xs.transpose(1, 0, 2))
    base = np.zeros(C, dtype=np.float32) if out0 is None else np.asarray(out0, dtype=np.float32)
    if slices == 1:
        return part[0] + base
    if drop_last_slice:
        part = part[:-1]
    if fold4:
        n32 = (part.shape[0] + 31) // 32
        lane = _seq(_pad0(part, n32 * 32).reshape(n32, 32, C))
        t = lane[0]
        for k in range(1, 32):
            t = t + lane[k]
        return t + base if out0 is not None else t
    return _seq(part) + base


# ------------------------------------------------------------------ fp8
FP8_LIM = {False: 448.0, True: 57344.0}
FP8_TORCH = {False: torch.float8_e4m3fn, True: torch.float8_e5m2}


def fp8_decode_table(e5m2):
    """float64 numpy [256] from the formats' definitions: e4m3fn = 1-4-3, bias 7, no infinities,
    S.1111.111 the only NaN; e5m2 = 1-5-2, bias 15, IEEE infinities and NaNs."""
    ebits, mbits, bias = (5, 2, 15) if e5m2 else (4, 3, 7)
    out = np.zeros(256)
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e, m = (code >> mbits) & ((1 << ebits) - 1), code & ((1 << mbits) - 1)
        if e5m2 and e == 31:
            v = np.inf if m == 0 else np.nan
        elif not e5m2 and e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m / (1 << mbits) * 2.0 ** (1 - bias)
        else:
            v = (1 + m / (1 << mbits)) * 2.0 ** (e - bias)
        out[code] = sign * v
    return out


def fp8_clamp(v, e5m2):
    """fmin(fmax(v, -lim), lim) of float32 v with C's NaN rule: a NaN gives -lim."""
    lim = FP8_LIM[bool(e5m2)]
    return torch.where(torch.isnan(v), torch.full_like(v, -lim), v.clamp(-lim, lim))


def fp8_encode(v, e5m2, half_up=False):
    """uint8 codes of float32 `v` already within +-lim, round to nearest, ties to even (torch's CPU
    cast; it does not saturate, hence the clamp first). half_up: a deliberately wrong encode (ties
    away from zero) by brute force, for the tests of the tests."""
    if not half_up:
        return v.to(F32).cpu().to(FP8_TORCH[bool(e5m2)]).view(torch.uint8).to(v.device)
    return torch.from_numpy(fp8_nearest(v.to(F64).cpu().numpy(), e5m2, half_up=True)).to(v.device)


def fp8_nearest(v, e5m2, half_up=False):
    """uint8 numpy codes by brute force: the nearest finite table value of float64 `v` (within
    +-lim), of two equally near the one with the even code; the sign bit is v's."""
    table = fp8_decode_table(e5m2)
    top = 0x7B if e5m2 else 0x7E
    pos = table[:top + 1]                               # ascending
    a = np.abs(v)
    d = np.abs(a[:, None] - pos[None, :])
    best = d.min(1)
    near = d == best[:, None]
    lo = near.argmax(1)
    hi = top - near[:, ::-1].argmax(1)
    code = np.where(lo == hi, lo, hi if half_up else np.where(lo % 2 == 0, lo, hi))
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def quant_fp8(x, scale, e5m2):
    """uint8 codes of bf16 x under the float32 `scale` (a Python float that float32 holds)."""
    v = x.to(F32) * torch.tensor(scale, dtype=F32, device=x.device)
    return fp8_encode(fp8_clamp(v, e5m2), e5m2)


def dequant_fp8(q, scale, e5m2):
    """bf16 of uint8 codes: decode, times float32(1 / scale), rounded to nearest even."""
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(scale, dtype=F32)
    v = q.cpu().view(FP8_TORCH[bool(e5m2)]).to(F32) * inv
    return v.to(BF16).to(q.device)


def amax(x, start=0.0):
    """max(start, max |x| over the elements that are no NaN) as a Python float."""
    v = x.to(F64).abs().reshape(-1)
    v = v[~torch.isnan(v)]
    return max(float(start), float(v.max()) if v.numel() else 0.0)


def all_bf16(device="cpu"):
    """Every bf16 bit pattern 0 .. 0xffff, in order."""
    return torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(BF16)


FP8_SCALES = (1.0, 0.5, 3.0, 2.0 ** -20, 2.0 ** 20)   # and 448 / amax of fp8_random_tensor()


def fp8_random_tensor():
    return (torch.randn(4096, generator=_gen(8, 8)) * 3).bfloat16()


def fp8_scales():
    """FP8_SCALES and float32(448 / amax) of a random tensor (the delayed-scaling recipe)."""
    am = torch.tensor(amax(fp8_random_tensor()), dtype=F32)
    return FP8_SCALES + (float(torch.tensor(448.0, dtype=F32) / am),)


# ------------------------------------------------------------------ layouts (on bit patterns)
def _ar(n, like):
    return torch.arange(n, dtype=torch.int64, device=like.device)


def pad_channels(x, rows, C, Cp):
    """flat [rows*Cp] from flat x [rows*C] (an integer view): element i is x[r*C + c] with
    r = i // Cp, c = i % Cp where c < C, else 0."""
    i = _ar(rows * Cp, x)
    r, c = i // Cp, i % Cp
    src = torch.cat([x.reshape(-1), torch.zeros(1, dtype=x.dtype, device=x.device)])
    return src[torch.where(c < C, r * C + c, torch.full_like(i, rows * C))]


def unpad_channels(x, rows, Cp, C):
    """flat [rows*C] from flat x [rows*Cp]: element i is x[r*Cp + c], r = i // C, c = i % C."""
    i = _ar(rows * C, x)
    return x.reshape(-1)[(i // C) * Cp + i % C]


def transpose_aca(x, A, B, C):
    """flat [C][B][A] from flat x [A][B][C]: element (c*B + b)*A + a is x[(a*B + b)*C + c]."""
    j = _ar(A * B * C, x)
    a, b, c = j % A, (j // A) % B, j // (A * B)
    return x.reshape(-1)[(a * B + b) * C + c]


def transpose2d(x, R, C):
    """flat [C][R] from flat x [R][C]: element c*R + r is x[r*C + c]."""
    return transpose_aca(x, R, 1, C)


def wprep_entry(x, K, R, S, C, s, r0, Tr, s0, Ts):
    """flat [C][Tr][Ts][K] from a flat filter x [K][R][S][C]: the taps r0 + tr*s, s0 + ts*s."""
    j = _ar(C * Tr * Ts * K, x)
    k, ts, tr, c = j % K, (j // K) % Ts, (j // (K * Ts)) % Tr, j // (K * Ts * Tr)
    return x.reshape(-1)[((k * R + r0 + tr * s) * S + s0 + ts * s) * C + c]


def ramp_bf16(n, device="cpu", start=1):
    """n bf16 elements of distinct bit patterns while n < 65536 (an index ramp viewed as bf16; it
    wraps after that), so that a swapped pair shows."""
    return ((torch.arange(n, dtype=torch.int64, device=device) + start) % 65536).to(torch.int32).to(torch.int16).view(BF16)


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run (for colsum: in the kernels' order) is compared
# with its float64 run on the case tables below (tests/test_elementwise_oracle_cpu.py prints them
# and asserts the relation).
BARS = {
    #                    scale of the figure                                   fp32
    "act_y": 3e-6,     # max(1, |z|) / (1 - rate); bf16                        1.43e-7
    "act_dx": 4e-6,    # |dy| max(1, |z|) / (1 - rate); bf16                   2.33e-7
    "colsum": 2e-6,    # sum_r |x| + |out0|                                    9.9e-8
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
CAST_N = (0, 1, 2, 3, 4, 5, 7, 1023, 1025)
CAST_WRAP = 4 * 256 * 16384 + 5
ADD_N = (8, 16, 8 * 257)
ADD_COEF = ((1.0, 1.0), (1.0, -1.0), (0.5, 2.0), (0.0, 1.0))

PAD_CCP = ((1, 8), (3, 8), (5, 16), (8, 8), (7, 8))
PAD_ROWS = (0, 1, 7, 8, 9, 45, 816)

ACA_B1 = ((128, 128), (128, 136), (8, 8), (8, 16), (40, 264), (1, 1), (31, 33), (32, 32), (33, 31))
ACA_B = ((1, 31, 33), (9, 33, 31), (49, 5, 70), (9, 40, 24))      # (B, A, C)
T2D = ((1, 1), (1, 33), (31, 33), (32, 32), (33, 65), (100, 7))

ACT_C = (1, 3, 8, 200)
ACT_N = (1, 3, 4, 5, 1023)
ACT_WRAP = 16384 * 256 + 1027
PLANTED = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 1e4, -1e4, 1e20, -1e20)
RATES = (0.01, 0.25, 0.5, 1.0)
SEEDS = ((0, 0), (7, 3), (2 ** 63 + 11, 2 ** 32 + 5))
DROP_N = (1, 5, 1023, 70001)

COLSUM_VEC_C = (8, 248, 256, 264)
COLSUM_VEC_ROWS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 128, 129)
COLSUM_VEC_BIG = ((4224, 8), (65536, 8))
COLSUM_SCALAR_C = (1, 3, 12, 90, 257)
COLSUM_SCALAR_ROWS = (1, 127, 128, 129, 4224, 32768, 40000)

AMAX_N = (0, 1, 63, 64, 65, 2048 * 256 + 17)
FP8_TAIL = 65536 + 3


# ------------------------------------------------------------------ seeded inputs
def act_inputs(n, C, dtype, with_bias, planted=True):
    """(x [n], bias float32 [C] or None, dy [n]) CPU tensors of `dtype` (values N(0, 2), dy
    N(0, 1)). Where `planted`, the first elements of column 0 hold PLANTED, and bias[0] is 0 so
    that z is exactly the planted value there (with a bias on one column only, C = 1, nothing is
    planted: the bias stays random). bf16 rounds 1e-30, 1e4 and 1e20 to their bf16 neighbours."""
    gen = _gen(n % 100003, C, dtype == BF16, with_bias, 21)
    x = (torch.randn(n, generator=gen) * 2).to(dtype)
    dy = torch.randn(n, generator=gen).to(dtype)
    bias = torch.randn(C, generator=gen) if with_bias else None
    if planted and not (with_bias and C == 1):
        if with_bias:
            bias[0] = 0.0
        pos = torch.arange(len(PLANTED)) * C
        pos = pos[pos < n]
        x[pos] = torch.tensor(PLANTED, dtype=F32)[:pos.numel()].to(dtype)
    return x, bias, dy


def drop_inputs(n, C, dtype, key=0):
    """(x, bias, dy): z = x + bias within [0.5, 2.5] and |dy| within [0.5, 1.5], so that neither y
    nor dx is 0 at a kept element under any of the activations."""
    gen = _gen(n % 100003, C, dtype == BF16, key, 22)
    x = (torch.rand(n, generator=gen) + 0.75).to(dtype)
    bias = torch.rand(C, generator=gen) * 0.5 - 0.25
    dy = ((torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).to(dtype)
    return x, bias, dy


def colsum_inputs(rows, C, dtype, key=0):
    """(x [rows, C] of `dtype`, out0 float32 [C]): N(0, 1); column 0 the constant 1."""
    gen = _gen(rows, C, dtype == BF16, key, 23)
    x = torch.randn(rows, C, generator=gen)
    x[:, 0] = 1.0
    return x.to(dtype), torch.randn(C, generator=gen) * 3


def act_cases():
    """(n, C, with_bias), run for each dtype and activation: the small sizes under every C with and
    without bias, and one wrap of the grid-stride loop (C = 200, with bias)."""
    return [(n, C, wb) for wb in (False, True) for C in ACT_C for n in ACT_N] + [(ACT_WRAP, 200, True)]


def drop_cases():
    """(n, dtype, kind, (seed, offset)) of one rate; C = 3 throughout."""
    return [(n, dt, kind, so) for so in SEEDS for dt in (F32, BF16) for kind in ACTS for n in DROP_N]


def colsum_cases():
    """(rows, C, dtype, form): form "vec" or "scalar" by what an aligned input takes."""
    cases = [(r, C, BF16, "vec") for C in COLSUM_VEC_C for r in COLSUM_VEC_ROWS]
    cases += [(r, C, BF16, "vec") for r, C in COLSUM_VEC_BIG]
    cases += [(r, C, dt, "scalar") for dt in (F32, BF16) for C in COLSUM_SCALAR_C for r in COLSUM_SCALAR_ROWS]
    return cases
