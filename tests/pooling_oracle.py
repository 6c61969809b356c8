"""What tests/test_pooling_kernels.py (GPU) and tests/test_pooling_oracle_cpu.py share (a plain
module, imported by them):

* plain statements of the operations of csrc/kernels/pool.hip and of the pooling kernels of
  csrc/kernels/nn_generic.hip, written from the definitions below and not from the kernels: torch,
  whole tensors, no blocks, no lanes, float64 unless `dtype=` says otherwise (the float32 run is how
  the bars are set);
* the case tables, the seeded inputs, the figures the bars apply to and the bars themselves.
  figure(), the bf16 half-ulp allowance, MARGIN, FLOOR, bar_holds() and check() are those of
  tests/transformer_oracle.py; BARS below is entered into its table so that they see it.

Definitions (NHWC, window R x S, strides sh, sw, top / left padding ph, pw, output P x Q given
explicitly; TF SAME puts its extra row and column at the bottom and right):

  max pooling  y[n,p,q,c] = the maximum over the taps (r,s) whose input pixel
               (p*sh - ph + r, q*sw - pw + s) lies inside the input; arg = r*S + s of the first such
               tap, in row-major order, that holds the maximum, and y is that tap's value (so of
               +0 and -0, which compare equal, y is the first one met). A NaN tap inside the input
               makes y NaN and arg names a NaN tap inside the input (which one is not pinned). arg
               always names a tap inside the input: when all of them are -inf, the first one.
  backward     dx[n,h,w,c] = the sum of dy[n,p,q,c] over the windows whose arg names (h,w), summed
               in float64 and rounded once for a bf16 output
  global avg   y[n,c] = sum_hw x / HW, dx = dy / HW
  stem         pooled = maxpool 3/2/1 of a = bf16(relu(y*scale + shift)); the mask bit of an element
               is [a > 0], bit j of byte i for element 8*i + j; g = bf16(mask * maxpool_bwd(dpooled));
               the rows of `partial` sum to (sum g, sum g*y) of the stored g, per channel

What is a pure selection is compared exactly and has no bar: y of max pooling, arg, the mask.
Staging: arg is checked first (arg_ok()); dx is then compared with maxpool_bwd() on the kernel's
own arg, and the stem's partial sums with the sums of the kernel's own stored g.

Figures. Every comparison is element-wise: figure = max |got - want| / scale; for a bf16 output
half a bf16 ulp of `want` is taken off the error first. The scales are written out beside BARS.
The float32 run uses the same definitions with dtype=torch.float32; no formula had to be changed
for it."""
import torch

import transformer_oracle as _TO
from transformer_oracle import F64, FLOOR, GUARD, MARGIN, _gen, bar_holds, bf16_half_ulp, check, figure  # noqa: F401

F32, BF16 = torch.float32, torch.bfloat16
NEG_INF, NAN = float("-inf"), float("nan")


# ------------------------------------------------------------------ geometry
def pool_out(H, k, s, p):
    """Output extent of a window k, stride s, symmetric padding p."""
    return (H + 2 * p - k) // s + 1


def explicit(H, W, k, s, p):
    """The geometry (R, S, sh, sw, ph, pw, P, Q) of a square window with symmetric padding."""
    return (k, k, s, s, p, p, pool_out(H, k, s, p), pool_out(W, k, s, p))


def same(H, W, R, S, sh, sw):
    """TF SAME: P = ceil(H / sh); of the (P-1)*sh + R - H padded rows the smaller half is on top."""
    P, Q = -(-H // sh), -(-W // sw)
    return (R, S, sh, sw, max((P - 1) * sh + R - H, 0) // 2, max((Q - 1) * sw + S - W, 0) // 2, P, Q)


def valid(H, W, R, S, sh, sw):
    return (R, S, sh, sw, 0, 0, (H - R) // sh + 1, (W - S) // sw + 1)


def accepted(geom):
    """What the entry points take: an output, the argmax in a byte, the padding smaller than the
    window."""
    R, S, sh, sw, ph, pw, P, Q = geom
    return P > 0 and Q > 0 and R * S <= 255 and ph < R and pw < S


def _tap_index(n_in, n_out, stride, pad, r, device):
    i = torch.arange(n_out, device=device) * stride - pad + r
    return i, (i >= 0) & (i < n_in)


# ------------------------------------------------------------------ max pooling
def taps(x, geom, dtype=F64):
    """(vals [R*S, N, P, Q, C] in `dtype`, inside [R*S, 1, P, Q, 1] bool): the value of every tap
    of every window (anything where the tap lies outside the input)."""
    R, S, sh, sw, ph, pw, P, Q = geom
    N, H, W, C = x.shape
    x = x.to(dtype)
    vals, inside = [], []
    for r in range(R):
        h, hin = _tap_index(H, P, sh, ph, r, x.device)
        for s in range(S):
            w, win = _tap_index(W, Q, sw, pw, s, x.device)
            vals.append(x[:, h.clamp(0, H - 1)][:, :, w.clamp(0, W - 1)])
            inside.append((hin[:, None] & win[None, :])[None, :, :, None])
    return torch.stack(vals), torch.stack(inside)


def maxpool(x, geom, dtype=F64):
    """(y, arg uint8, holds): holds [R*S, N, P, Q, C] marks the taps `arg` may name: the taps
    inside the input that are NaN where the window has one, else that equal the maximum."""
    vals, inside = taps(x, geom, dtype)
    T = vals.shape[0]
    nan_tap = inside & torch.isnan(vals)
    has_nan = nan_tap.any(0)
    lowest = torch.full_like(vals, NEG_INF)
    y = torch.where(inside & ~nan_tap, vals, lowest).amax(0)
    holds = torch.where(has_nan[None], nan_tap, inside & (vals == y[None]))
    index = torch.arange(T, device=x.device).view(T, 1, 1, 1, 1).expand_as(holds)
    first = torch.where(holds, index, torch.full_like(index, T)).amin(0)
    # y is the value of the tap arg names: of +0 and -0, which compare equal, the first one met
    y = vals.gather(0, first.clamp(0, T - 1)[None])[0]
    return y, first.to(torch.uint8), holds


def arg_ok(arg, first, holds, y):
    """arg by the rule: a tap that `holds`, and the first of them where the window has no NaN."""
    named = holds.gather(0, arg.long().clamp(0, holds.shape[0] - 1)[None])[0] & (arg.long() < holds.shape[0])
    return bool(named.all()) and bool((torch.isnan(y) | (arg == first)).all())


def maxpool_bwd(dy, arg, x_shape, geom, dtype=F64):
    """(dx, the same sum of |dy|: the scale of its figure). A gradient whose arg names a tap
    outside the input goes nowhere."""
    R, S, sh, sw, ph, pw, P, Q = geom
    N, H, W, C = x_shape
    d = dy.to(dtype)
    dx = torch.zeros((N, H, W, C), dtype=dtype, device=dy.device)
    mag = torch.zeros_like(dx)
    zero = torch.zeros_like(d)
    for r in range(R):
        h, hin = _tap_index(H, P, sh, ph, r, dy.device)
        for s in range(S):
            w, win = _tap_index(W, Q, sw, pw, s, dy.device)
            if not (bool(hin.any()) and bool(win.any())):
                continue
            part = torch.where(arg == r * S + s, d, zero)[:, hin][:, :, win]
            hi, wi = h[hin][:, None], w[win][None, :]   # distinct pixels: one window each per tap
            dx[:, hi, wi] += part
            mag[:, hi, wi] += part.abs()
    return dx, mag


# ------------------------------------------------------------------ global average pooling
def gap(x, dtype=F64):
    """(y [N, C], sum|x| / HW)."""
    N, C = x.shape[0], x.shape[-1]
    v = x.to(dtype).reshape(N, -1, C)
    return v.sum(1) / v.shape[1], v.abs().sum(1).to(F64) / v.shape[1]


def gap_bwd(dy, x_shape, dtype=F64):
    """(dx, |dy| / HW)."""
    N, H, W, C = x_shape
    d = (dy.to(dtype) / (H * W))[:, None, None, :].expand(N, H, W, C)
    return d, d.abs().to(F64)


# ------------------------------------------------------------------ stem fusions
STEM = (3, 3, 2, 2, 1, 1)


def stem_geom(H, W):
    return STEM + (H // 2, W // 2)


def stem_activation(y, scale, shift, dtype=F64):
    f = y.to(dtype) * scale.to(dtype) + shift.to(dtype)
    return torch.where(f > 0, f, torch.zeros_like(f)).to(BF16)


_BITS = (1, 2, 4, 8, 16, 32, 64, 128)


def mask_bits(a):
    """uint8 [numel/8]: bit j of byte i is [a.flatten()[8*i + j] > 0]."""
    b = (a.to(F64) > 0).reshape(-1, 8).to(torch.int32)
    return (b * torch.tensor(_BITS, dtype=torch.int32, device=a.device)).sum(1).to(torch.uint8)


def mask_bools(mask, shape):
    w = torch.tensor(_BITS, dtype=torch.int32, device=mask.device)
    return ((mask.to(torch.int32)[:, None] & w) != 0).reshape(shape)


def stem_bwd(dpooled, arg, keep, dtype=F64):
    """(g before the bf16 store, its scale); keep: bool like the input."""
    H, W = keep.shape[1], keep.shape[2]
    dx, mag = maxpool_bwd(dpooled, arg, keep.shape, stem_geom(H, W), dtype)
    return torch.where(keep, dx, torch.zeros_like(dx)), mag


def stem_sums(g, y, dtype=F64):
    """((sum g, sum g*y) [2, C] of a stored g, the same sums of the magnitudes)."""
    C = g.shape[-1]
    g, y = g.to(dtype).reshape(-1, C), y.to(dtype).reshape(-1, C)
    return torch.stack([g.sum(0), (g * y).sum(0)]), torch.stack([g.abs().sum(0), (g * y).abs().sum(0)]).to(F64)


# ------------------------------------------------------------------ bars
# figure name -> bar = MARGIN * max(fp32, 2^-24), rounded up to one digit. `fp32` is the largest
# value of that figure when this module's float32 run is compared with its float64 run on the case
# tables below (tests/test_pooling_oracle_cpu.py prints them and asserts the relation).
BARS = {
    #                          scale of the figure                                     fp32
    "pool_dx": 1e-6,         # sum |dy| of the windows that name the pixel; bf16       4.1e-8
    "gap_y": 1e-6,           # sum_hw |x| / HW; bf16                                   4.0e-8
    "gap_dx": 1e-6,          # |dy| / HW; bf16                                         5.4e-8
    "stem_g": 1e-6,          # sum |dpooled| of the windows that name the pixel; bf16  0
    "stem_partial": 1e-6,    # sum |g| and sum |g*y| of the stored g                   0
}
_TO.BARS.update(BARS)  # bar_holds() and check() look names up there

# ------------------------------------------------------------------ case tables
N_IMAGES = 2
VARIANTS = ("randn", "const", "neginf", "nan", "border")   # what image 1 of an input holds

FAST_KSP = ((3, 2, 1), (3, 1, 1), (2, 2, 0), (3, 2, 0), (5, 3, 2))
FAST_HW = ((9, 8), (8, 9), (1, 1), (2, 7))
FAST_C = (8, 24, 64)
FAST_CASES = [(ksp, hw, C) for ksp in FAST_KSP for hw in FAST_HW for C in FAST_C]

# just past 16384 blocks of 256 eight-channel groups on the output side
WRAP = {"N": 2, "H": 1026, "W": 1024, "C": 64, "ksp": (2, 2, 0)}

GENERIC_C = (1, 3, 5, 16)
# (label, H, W, geometry)
GENERIC_GEOMS = [
    ("same_3x2_s2x1_even", 8, 6, same(8, 6, 3, 2, 2, 1)),     # ph = 0: the overhang is at the bottom
    ("same_3x2_s2x1_odd", 9, 7, same(9, 7, 3, 2, 2, 1)),      # ph = 1
    ("same_3x3_s2_even", 8, 8, same(8, 8, 3, 3, 2, 2)),       # ph = pw = 0, bottom / right overhang
    ("same_3x3_s2_odd", 9, 9, same(9, 9, 3, 3, 2, 2)),        # ph = pw = 1
    ("valid_3x2_s2x1", 9, 8, valid(9, 8, 3, 2, 2, 1)),
    ("valid_2x2_s2", 7, 7, valid(7, 7, 2, 2, 2, 2)),          # the last row and column are never read
    ("explicit_3x2_s2x1_p1x1", 5, 4, (3, 2, 2, 1, 1, 1, 3, 5)),
]

AVG_HW = (1, 49, 50, 12544)
AVG_C = (8, 24, 512, 520)
AVG_N = (1, 3)
AVG_CASES = [(N, HW, C) for C in AVG_C for HW in AVG_HW for N in AVG_N]

GAP_C = (1, 3, 63, 64, 65)
GAP_HW = (1, 3, 4, 5, 49)
GAP_N = 2
GAP_CASES = [(HW, C) for C in GAP_C for HW in GAP_HW]

STEM_SHAPES = ((2, 4, 4, 8), (2, 12, 10, 32), (1, 2, 2, 2048), (1, 6, 4, 128))


# ------------------------------------------------------------------ seeded inputs
def pool_inputs(H, W, C, variant, key=0):
    """(x, dy-source) float32 CPU tensors [2, H, W, C] whose values are bf16 numbers. x is N(0,1)
    rounded to bf16 and then to 1/4 steps in image 0 channel 0 (many ties); image 1 by `variant`:
    randn as image 0, const 1.5 everywhere, neginf everywhere, nan one NaN at the centre pixel of
    channel 0, border -inf on the outermost pixels. The second tensor is N(0,1) in bf16: cut to
    the output's shape it is the incoming gradient."""
    gen = _gen(H, W, C, VARIANTS.index(variant), key)
    x = torch.randn(N_IMAGES, H, W, C, generator=gen).bfloat16().float()
    x[0, :, :, 0] = (x[0, :, :, 0] * 4).round() / 4
    if variant == "const":
        x[1] = 1.5
    elif variant == "neginf":
        x[1] = NEG_INF
    elif variant == "nan":
        x[1, H // 2, W // 2, 0] = NAN
    elif variant == "border":
        x[1, 0], x[1, H - 1], x[1, :, 0], x[1, :, W - 1] = NEG_INF, NEG_INF, NEG_INF, NEG_INF
    return x, torch.randn(N_IMAGES, max(H, 1) + 4, max(W, 1) + 4, C, generator=gen).bfloat16().float()


def cut(d, P, Q):
    """The leading [N, P, Q, C] of pool_inputs' second tensor, contiguous."""
    return d[:, :P, :Q].contiguous()


def wrap_inputs(device):
    """x [2, 1026, 1024, 64]: small integers by a cheap rule, many ties; dy [2, 513, 512, 64]: 1, 2
    or 3, so that every sum is exact."""
    N, H, W, C = WRAP["N"], WRAP["H"], WRAP["W"], WRAP["C"]
    n = torch.arange(N, device=device).view(N, 1, 1, 1)
    h = torch.arange(H, device=device).view(1, H, 1, 1)
    w = torch.arange(W, device=device).view(1, 1, W, 1)
    c = torch.arange(C, device=device).view(1, 1, 1, C)
    x = ((h * 7 + w * 13 + c * 3 + n * 5) % 251 - 125).to(BF16)
    k, s, p = WRAP["ksp"]
    P, Q = pool_out(H, k, s, p), pool_out(W, k, s, p)
    dy = ((h[:, :P] * 3 + w[:, :, :Q] + c + n) % 3 + 1).to(BF16)
    return x, dy


def avg_inputs(N, HW, C):
    """(x [N, HW, 1, C], dy [N, C]) bf16: N(0,1); channel 0 the constant 3, channel 1 zeros (where C
    has them)."""
    gen = _gen(N, HW, C, 5)
    x = torch.randn(N, HW, 1, C, generator=gen)
    x[..., 0] = 3.0
    if C > 1:
        x[..., 1] = 0.0
    return x.bfloat16(), torch.randn(N, C, generator=gen).bfloat16()


def stem_inputs(shape):
    """y [N, H, W, C] in steps of 1/16 within +-7.9, scale in steps of 1/8 (some negative, one 0),
    shift in steps of 1/16: y*scale + shift is then exact in float32 however it is evaluated, so the
    bf16 activation of a kernel and of the float64 statement are the same numbers and the exact
    comparisons of pooled, arg and mask are fair. dpooled N(0,1) in bf16."""
    N, H, W, C = shape
    gen = _gen(N, H, W, C, 6)
    y = ((torch.randn(shape, generator=gen) * 2 * 16).round() / 16).clamp(-7.875, 7.875)
    scale = torch.randint(4, 13, (C,), generator=gen).float() / 8
    scale[1], scale[2] = -scale[1], 0.0
    shift = torch.randint(-16, 17, (C,), generator=gen).float() / 16
    dpooled = torch.randn(N, H // 2, W // 2, C, generator=gen).bfloat16()
    return {"y": y.bfloat16(), "scale": scale, "shift": shift, "dpooled": dpooled}
