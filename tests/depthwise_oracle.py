"""Float64 statement of the depthwise convolution and its two gradients (not a test).

    y[n,p,q,c*M+m]  = sum_{r,s} x[n, p*sh-ph+r*dh, q*sw-pw+s*dw, c] * k[r,s,c,m]
    dx[n,h,w,c]     = sum_{r,s,m} dy[n,p,q,c*M+m] * k[r,s,c,m]   over the (p,q) whose tap (r,s) reads (h,w)
    dk[r,s,c,m]     = sum_{n,p,q} x[n, p*sh-ph+r*dh, q*sw-pw+s*dw, c] * dy[n,p,q,c*M+m]

written as explicit loops over the taps (r, s) and the output rows p, with the out-of-range test of
every input coordinate written out (a row as a skipped iteration, the columns of one output row as
a mask). Nothing here calls a convolution routine. `geometry` is TF's SAME / VALID rule."""
import torch

# (N, H, W, C, M, (R, S), strides, dilations, padding, dtype), the shapes of the depthwise tests
FAST_SHAPES = [
    (2, 10, 12, 8, 1, (3, 3), (2, 2), (1, 1), "SAME", torch.bfloat16),
    (2, 9, 7, 24, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.bfloat16),
    (1, 1, 1, 8, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.bfloat16),
    (1, 2, 3, 72, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.bfloat16),
    (3, 17, 33, 264, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.bfloat16),
    (2, 11, 9, 16, 1, (3, 3), (2, 2), (1, 1), "VALID", torch.bfloat16),
    (2, 9, 7, 24, 1, (3, 3), (1, 1), (1, 1), (2, 0), torch.bfloat16),
]
GENERIC_SHAPES = [
    (2, 11, 9, 5, 3, (5, 5), (2, 1), (1, 1), "SAME", torch.float32),
    (2, 13, 13, 5, 2, (3, 3), (1, 1), (2, 2), "SAME", torch.float32),
    (1, 14, 14, 16, 1, (7, 7), (1, 1), (1, 1), "SAME", torch.bfloat16),
    (2, 9, 7, 24, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.float32),
    (2, 9, 7, 12, 1, (3, 3), (1, 1), (1, 1), "SAME", torch.bfloat16),
]


def geometry(H, W, R, S, strides, padding, dilations=(1, 1)):
    """(sh, sw, ph, pw, dh, dw, P, Q). SAME: P = ceil(H / sh), total padding split with the extra
    row at the bottom / right (ph = total // 2). VALID: no padding. (ph, pw): explicit, symmetric."""
    (sh, sw), (dh, dw) = strides, dilations
    eh, ew = (R - 1) * dh + 1, (S - 1) * dw + 1
    if padding == "VALID":
        return sh, sw, 0, 0, dh, dw, (H - eh) // sh + 1, (W - ew) // sw + 1
    if padding == "SAME":
        P, Q = (H + sh - 1) // sh, (W + sw - 1) // sw
        th, tw = max((P - 1) * sh + eh - H, 0), max((Q - 1) * sw + ew - W, 0)
        return sh, sw, th // 2, tw // 2, dh, dw, P, Q
    ph, pw = padding
    return sh, sw, ph, pw, dh, dw, (H + 2 * ph - eh) // sh + 1, (W + 2 * pw - ew) // sw + 1


def make_inputs(shape, seed=0):
    """x, kernel, dy in float64 with values on the bf16 grid (every dtype reads the same numbers),
    and the geometry, for one row of the shape lists."""
    n, h, w, c, m, (r, s), strides, dil, padding, _ = shape
    geom = geometry(h, w, r, s, strides, padding, dil)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g).bfloat16().double()
    k = (torch.randn(r, s, c, m, generator=g) * 0.5).bfloat16().double()
    dy = torch.randn(n, geom[6], geom[7], c * m, generator=g).bfloat16().double()
    return x, k, dy, geom


def _columns(Q, W, sw, pw, s, dw):
    """Output columns q whose tap s reads an input column inside the image, and those columns."""
    q = torch.arange(Q)
    w = q * sw - pw + s * dw
    inside = (w >= 0) & (w < W)
    return q[inside], w[inside]


def forward(x, k, geom):
    """y float64 [N,P,Q,C*M] of x [N,H,W,C], k [R,S,C,M] (any float dtype; read as float64)."""
    sh, sw, ph, pw, dh, dw, P, Q = geom
    x, k = x.detach().cpu().double(), k.detach().cpu().double()
    N, H, W, C = x.shape
    R, S, _, M = k.shape
    y = torch.zeros(N, P, Q, C, M, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            q, w = _columns(Q, W, sw, pw, s, dw)
            for p in range(P):
                h = p * sh - ph + r * dh
                if h < 0 or h >= H:
                    continue
                y[:, p, q] += x[:, h, w][..., None] * k[r, s]
    return y.reshape(N, P, Q, C * M)


def dgrad(dy, k, x_shape, geom):
    """dx float64 [N,H,W,C] of dy [N,P,Q,C*M]."""
    sh, sw, ph, pw, dh, dw, P, Q = geom
    N, H, W, C = x_shape
    k = k.detach().cpu().double()
    R, S, _, M = k.shape
    dy = dy.detach().cpu().double().reshape(N, P, Q, C, M)
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            q, w = _columns(Q, W, sw, pw, s, dw)  # w is strictly increasing: no index repeats
            for p in range(P):
                h = p * sh - ph + r * dh
                if h < 0 or h >= H:
                    continue
                dx[:, h, w] += (dy[:, p, q] * k[r, s]).sum(-1)
    return dx


def wgrad(x, dy, k_shape, geom):
    """dk float64 [R,S,C,M]."""
    sh, sw, ph, pw, dh, dw, P, Q = geom
    x = x.detach().cpu().double()
    N, H, W, C = x.shape
    R, S, _, M = k_shape
    dy = dy.detach().cpu().double().reshape(N, P, Q, C, M)
    dk = torch.zeros(R, S, C, M, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            q, w = _columns(Q, W, sw, pw, s, dw)
            for p in range(P):
                h = p * sh - ph + r * dh
                if h < 0 or h >= H:
                    continue
                dk[r, s] += (x[:, h, w][..., None] * dy[:, p, q]).sum((0, 1))
    return dk


def rel_err(got, want):
    """max |got - want| / max |want| (the measure of test_nn_gpu_ops.py)."""
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp(min=1e-30))
